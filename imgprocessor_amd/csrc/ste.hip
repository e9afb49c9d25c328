// ste.hip — single-time-effect (STE) removal over a stack of equivalent exposures on gfx950:
//   ipa_ste_dev                   features/SingleTimeEffectDetection.py:13-75 given a noise level
//                                 function (camera/NoiseLevelFunction.py:94-107 boundedFunction)
//   ipa_remove_single_pixels_dev  filters/removeSinglePixels.py:4-30
//
// Per pixel the reference keeps a masked running mean (avg, count) and a threshold thr fixed by
// the first pair of frames.  Frame k's decision at a pixel needs its 8 neighbours' averages after
// frame k-1, so a launch that walks F frames makes each workgroup recompute a halo of F pixels
// around its output tile: the state of the whole tile (output + halo) stays in registers from
// the first frame to the last, and the frames are the only thing read per step.
//
// Tile: 128 x 64 pixels, 8 waves of 8 rows; a lane owns one column in each 64-wide half.  A row's
// STE candidates are two 64-bit ballots, so the 3x3 neighbour test is scalar bit arithmetic on
// whole rows; only the first and last row of each wave go through LDS to the waves above and
// below.  Pixels outside the image are never set, and nothing outside the tile is looked at:
// after step k the outer k rings of the tile are stale, which is why the halo is F wide.
//
// Every operation is a float64 compare, subtraction, division or square root, each correctly
// rounded: results equal numpy's bits.  FP contraction is off for this file (Makefile + pragma)
// because numpy never fuses and a fused `x - a * sqrt(..)` would not round like it.
#include "common.hpp"
#include "frame_args.hpp"
#include "launch.hpp"
#include "nlf_fn.hpp"

#pragma clang fp contract(off)

namespace ipa {
namespace {

constexpr int kSteHalves = 2;                 // 64-wide halves of a tile row
constexpr int kSteW = 64 * kSteHalves;        // tile width (output + halo)
constexpr int kSteWaves = 8;
constexpr int kSteRowsPerWave = 8;
constexpr int kSteH = kSteWaves * kSteRowsPerWave;   // tile height (output + halo)
constexpr int kSteMaxF = 8;                   // frames per launch of the halo kernel

typedef unsigned long long u64;

struct Row128 {
  u64 lo, hi;   // bit c of lo: column c, bit c of hi: column 64 + c
};
__device__ inline Row128 shl1(Row128 r) { return {r.lo << 1, (r.hi << 1) | (r.lo >> 63)}; }
__device__ inline Row128 shr1(Row128 r) { return {(r.lo >> 1) | (r.hi << 63), r.hi >> 1}; }
__device__ inline Row128 dilate(Row128 r) {   // a column or its left / right neighbour set
  const Row128 a = shl1(r), b = shr1(r);
  return {r.lo | a.lo | b.lo, r.hi | a.hi | b.hi};
}

struct SteArgs {
  const void* frames;       // frame 0 of this launch
  long pitch, frame_stride;
  int h, w, steps, first_pair;
  double min_y, ax, ay, nstd;
  int nlf;                  // 1: thr from the NLF (first pair), 0: thr read from d_thr
  const double* avg_in;     // NULL on the first pair
  const int* count_in;
  long in_pitch;
  double* avg_out;
  int* count_out;
  long out_pitch;
  double* thr;              // read (nlf == 0) or written (first pair with an NLF)
  long thr_pitch;
  const unsigned char* mask;
  unsigned char* mask_ste;
  unsigned char* mask_clean;
  long mask_pitch;
};

template <typename T>
__device__ inline double load_px(const T* base, long off) {
  return (double)base[off];
}

// One launch: `steps` (<= F) frames; with first_pair the first step consumes frames 0 and 1.
template <typename T, int F>
__global__ void __launch_bounds__(64 * kSteWaves)
ste_kernel(SteArgs a) {
  __shared__ Row128 edge[2][kSteWaves][2];   // [step parity][wave][top, bottom row]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int halo = a.steps;
  const int x0 = blockIdx.x * (kSteW - 2 * halo) - halo;
  const int y0 = blockIdx.y * (kSteH - 2 * halo) - halo;
  const int ty0 = wave * kSteRowsPerWave;
  // clamped coordinates: every load is inside the frame; `in` masks what is not the pixel itself
  int xc[kSteHalves];
  bool xin[kSteHalves];
#pragma unroll
  for (int hf = 0; hf < kSteHalves; hf++) {
    const int x = x0 + hf * 64 + lane;
    xin[hf] = x >= 0 && x < a.w;
    xc[hf] = min(max(x, 0), a.w - 1);
  }
  int yc[kSteRowsPerWave];
  bool yin[kSteRowsPerWave];
#pragma unroll
  for (int i = 0; i < kSteRowsPerWave; i++) {
    const int y = y0 + ty0 + i;
    yin[i] = y >= 0 && y < a.h;
    yc[i] = min(max(y, 0), a.h - 1);
  }

  double avg[kSteRowsPerWave][kSteHalves], thr[kSteRowsPerWave][kSteHalves];
  int cnt[kSteRowsPerWave][kSteHalves];
  unsigned keep = 0, ste = 0, clean_last = 0;   // bit i * 2 + hf
  const T* fr = (const T*)a.frames;

#pragma unroll
  for (int i = 0; i < kSteRowsPerWave; i++)
#pragma unroll
    for (int hf = 0; hf < kSteHalves; hf++) {
      const int b = i * 2 + hf;
      if (a.mask == nullptr || a.mask[(long)yc[i] * a.mask_pitch + xc[hf]]) keep |= 1u << b;
      if (a.first_pair) {
        const long off = (long)yc[i] * a.pitch + xc[hf];
        const double f0 = load_px(fr, off), f1 = load_px(fr, off + a.frame_stride);
        avg[i][hf] = np_min(f0, f1);   // the pair's minimum is the first sample (:39)
        cnt[i][hf] = 1;
      } else {
        avg[i][hf] = a.avg_in[(long)yc[i] * a.in_pitch + xc[hf]];
        cnt[i][hf] = a.count_in[(long)yc[i] * a.in_pitch + xc[hf]];
      }
      if (a.nlf)
        thr[i][hf] = bounded_nlf(avg[i][hf], a.min_y, a.ax, a.ay) * a.nstd;
      else
        thr[i][hf] = a.thr[(long)yc[i] * a.thr_pitch + xc[hf]];
    }

  const int nsteps = F == 1 ? 1 : a.steps;
#pragma unroll 1
  for (int k = 0; k < nsteps; k++) {
    // frame of this step: max(f0, f1) on the first pair, then frame k (+1 after the pair)
    const bool pair = a.first_pair && k == 0;
    const T* g = fr + (long)(k + a.first_pair) * a.frame_stride;
    double gv[kSteRowsPerWave][kSteHalves];
    Row128 s[kSteRowsPerWave];
#pragma unroll
    for (int i = 0; i < kSteRowsPerWave; i++) {
#pragma unroll
      for (int hf = 0; hf < kSteHalves; hf++) {
        const long off = (long)yc[i] * a.pitch + xc[hf];
        double v = load_px(g, off);
        if (pair) v = np_max(load_px(fr, off), v);
        gv[i][hf] = v;
      }
      const bool s0 = yin[i] && xin[0] && gv[i][0] - avg[i][0] > thr[i][0];
      const bool s1 = yin[i] && xin[1] && gv[i][1] - avg[i][1] > thr[i][1];
      s[i] = {(u64)__ballot(s0), (u64)__ballot(s1)};
    }
    const int p = k & 1;   // two LDS slots: a wave writing step k+2 has passed step k+1's barrier
    if (lane == 0) {
      edge[p][wave][0] = s[0];
      edge[p][wave][1] = s[kSteRowsPerWave - 1];
    }
    __syncthreads();
    const Row128 zero = {0, 0};
    const Row128 above = wave > 0 ? edge[p][wave - 1][1] : zero;
    const Row128 below = wave < kSteWaves - 1 ? edge[p][wave + 1][0] : zero;
#pragma unroll
    for (int i = 0; i < kSteRowsPerWave; i++) {
      const Row128 up = dilate(i > 0 ? s[i - 1] : above);
      const Row128 dn = dilate(i < kSteRowsPerWave - 1 ? s[i + 1] : below);
      const Row128 l = shl1(s[i]), r = shr1(s[i]);
      // removeSinglePixels: keep a candidate only when one of its 8 neighbours is one too
      const u64 lo = s[i].lo & (up.lo | dn.lo | l.lo | r.lo);
      const u64 hi = s[i].hi & (up.hi | dn.hi | l.hi | r.hi);
#pragma unroll
      for (int hf = 0; hf < kSteHalves; hf++) {
        const int b = i * 2 + hf;
        const bool sp = (((hf ? hi : lo) >> lane) & 1) != 0;
        if (sp) {
          ste |= 1u << b;
          clean_last &= ~(1u << b);
        } else {
          clean_last |= 1u << b;
        }
        if (!sp && (keep >> b & 1)) {   // clean and allowed by the caller's mask: one more sample (:65-70)
          const int c = cnt[i][hf] + 1;
          cnt[i][hf] = c;
          avg[i][hf] = avg[i][hf] + (gv[i][hf] - avg[i][hf]) / (double)c;
        }
      }
    }
  }

  // the output tile: the pixels at least `halo` from the tile border
#pragma unroll
  for (int i = 0; i < kSteRowsPerWave; i++) {
    const int ty = ty0 + i;
    if (!yin[i] || ty < halo || ty >= kSteH - halo) continue;
#pragma unroll
    for (int hf = 0; hf < kSteHalves; hf++) {
      const int tx = hf * 64 + lane;
      if (!xin[hf] || tx < halo || tx >= kSteW - halo) continue;
      const int b = i * 2 + hf;
      const long so = (long)yc[i] * a.out_pitch + xc[hf];
      a.avg_out[so] = avg[i][hf];
      a.count_out[so] = cnt[i][hf];
      if (a.nlf) a.thr[(long)yc[i] * a.thr_pitch + xc[hf]] = thr[i][hf];
      const long mo = (long)yc[i] * a.mask_pitch + xc[hf];
      if (a.mask_ste && (ste >> b & 1)) a.mask_ste[mo] = 1;
      if (a.mask_clean) a.mask_clean[mo] = (unsigned char)(clean_last >> b & 1);
    }
  }
}

__global__ void __launch_bounds__(256)
remove_single_pixels_kernel(const unsigned char* __restrict__ in, int h, int w, long pitch,
                            unsigned char* __restrict__ out, long out_pitch) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= w || y >= h) return;
  unsigned char v = in[(long)y * pitch + x] ? 1 : 0;
  if (v) {
    bool nb = false;
    for (int yy = max(y - 1, 0); yy <= min(y + 1, h - 1); yy++)
      for (int xx = max(x - 1, 0); xx <= min(x + 1, w - 1); xx++)
        if ((yy != y || xx != x) && in[(long)yy * pitch + xx]) nb = true;
    v = nb ? 1 : 0;
  }
  out[(long)y * out_pitch + x] = v;
}

}  // namespace
}  // namespace ipa

using namespace ipa;

extern "C" {

int ipa_ste_dev(ipa_ctx* ctx, const void* d_frames, int dtype, int n, int h, int w, long pitch,
                long frame_stride, int first_pair, const double* nlf, double nstd, double* d_avg,
                int* d_count, double* d_thr, long state_pitch, const unsigned char* d_mask,
                unsigned char* d_mask_ste, unsigned char* d_mask_clean, long mask_pitch) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  IPA_REQUIRE(ctx, d_frames && d_avg && d_count, "ste: null pointer");
  IPA_REQUIRE(ctx, d_thr, "ste: d_thr is NULL: the threshold is always kept in the state");
  IPA_REQUIRE(ctx, h > 0 && w > 0, "ste: empty image");
  IPA_REQUIRE(ctx, first_pair ? n >= 2 : n >= 1, "ste: the first pair needs n >= 2 frames (got %d)", n);
  IPA_REQUIRE(ctx, pitch >= w && state_pitch >= w, "ste: pitch smaller than width");
  IPA_REQUIRE(ctx, !(d_mask || d_mask_ste || d_mask_clean) || mask_pitch >= w,
              "ste: mask pitch smaller than width");
  IPA_REQUIRE(ctx, n == 1 || frame_stride >= (long)(h - 1) * pitch + w, "ste: frames overlap");
  if (!known_dtype(dtype))
    IPA_UNSUPPORTED(ctx, "ste: frames are uint8 / uint16 / float32 / float64 (got dtype %d)", dtype);
  const size_t es = ipa_dtype_size(dtype);
  // the first five are written; none may overlap another array of the call
  const Span spans[] = {span2d(d_avg, h, w, state_pitch, 8),
                        span2d(d_count, h, w, state_pitch, 4),
                        span2d(d_thr, h, w, state_pitch, 8),
                        span2d(d_mask_ste, h, w, mask_pitch, 1),
                        span2d(d_mask_clean, h, w, mask_pitch, 1),
                        span_stack(d_frames, n, h, w, pitch, frame_stride, es),
                        span2d(d_mask, h, w, mask_pitch, 1)};
  IPA_REQUIRE(ctx, !written_overlaps(spans, 5), "ste: state, masks and frames overlap");

  const int steps = first_pair ? n - 1 : n;
  const int fmax = ctx->tune.ste_frames <= 1 ? 1 : kSteMaxF;
  const int launches = (steps + fmax - 1) / fmax;
  // A launch reads the state of its halo, which neighbouring workgroups of the SAME launch write:
  // input and output state are never the same buffer.  The launches alternate between the
  // caller's state and the workspace so that the last one writes the caller's.
  const bool need_copy = !first_pair && (launches & 1);
  double* ws_avg = nullptr;
  int* ws_cnt = nullptr;
  if (launches > 1 || need_copy) {
    int rc = ipa_ws_reserve(ctx, (size_t)h * w * 12);
    if (rc) return rc;
    ws_avg = (double*)ctx->ws;
    ws_cnt = (int*)((char*)ctx->ws + (size_t)h * w * 8);
  }
  IPA_HIP(ctx, hipSetDevice(ctx->device));
  if (need_copy) {
    IPA_HIP(ctx, hipMemcpy2DAsync(ws_avg, (size_t)w * 8, d_avg, (size_t)state_pitch * 8,
                                  (size_t)w * 8, h, hipMemcpyDeviceToDevice, ctx->stream));
    IPA_HIP(ctx, hipMemcpy2DAsync(ws_cnt, (size_t)w * 4, d_count, (size_t)state_pitch * 4,
                                  (size_t)w * 4, h, hipMemcpyDeviceToDevice, ctx->stream));
  }
  const double* in_avg = need_copy ? ws_avg : d_avg;
  const int* in_cnt = need_copy ? ws_cnt : d_count;
  long in_pitch = need_copy ? w : state_pitch;
  int done = 0;   // steps done
  for (int l = 0; l < launches; l++) {
    const int st = min(fmax, steps - done);
    const bool to_user = ((launches - 1 - l) & 1) == 0;
    SteArgs a;
    a.frames = (const char*)d_frames +
               (size_t)(done + (first_pair && l > 0 ? 1 : 0)) * frame_stride * es;
    a.pitch = pitch;
    a.frame_stride = frame_stride;
    a.h = h;
    a.w = w;
    a.steps = st;
    a.first_pair = first_pair && l == 0;
    a.nlf = a.first_pair && nlf;
    a.min_y = nlf ? nlf[0] : 0.0;
    a.ax = nlf ? nlf[1] : 0.0;
    a.ay = nlf ? nlf[2] : 0.0;
    a.nstd = nstd;
    a.avg_in = a.first_pair ? nullptr : in_avg;
    a.count_in = a.first_pair ? nullptr : in_cnt;
    a.in_pitch = in_pitch;
    a.avg_out = to_user ? d_avg : ws_avg;
    a.count_out = to_user ? d_count : ws_cnt;
    a.out_pitch = to_user ? state_pitch : w;
    a.thr = d_thr;
    a.thr_pitch = state_pitch;
    a.mask = d_mask;
    a.mask_ste = d_mask_ste;
    a.mask_clean = l == launches - 1 ? d_mask_clean : nullptr;
    a.mask_pitch = mask_pitch;
    dim3 grid((w + kSteW - 2 * st - 1) / (kSteW - 2 * st), (h + kSteH - 2 * st - 1) / (kSteH - 2 * st));
    // (listed last first: pick instantiates, and the code object lays out, from the back)
    const int rc = pick<kSteMaxF, 1>(fmax, [&](auto F) {
      return by_dtype(dtype, [&](auto e) {
        return launch(ctx, ste_kernel<decltype(e), F()>, grid, dim3(64 * kSteWaves), 0, a);
      });
    });
    if (rc) return rc;
    in_avg = a.avg_out;
    in_cnt = a.count_out;
    in_pitch = a.out_pitch;
    done += st;
  }
  return IPA_OK;
}

int ipa_remove_single_pixels_dev(ipa_ctx* ctx, const unsigned char* d_in, int h, int w, long pitch,
                                 unsigned char* d_out, long out_pitch) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  IPA_REQUIRE(ctx, d_in && d_out, "remove_single_pixels: null pointer");
  IPA_REQUIRE(ctx, h > 0 && w > 0, "remove_single_pixels: empty image");
  IPA_REQUIRE(ctx, pitch >= w && out_pitch >= w, "remove_single_pixels: pitch smaller than width");
  IPA_REQUIRE(ctx, !overlap(span2d(d_in, h, w, pitch, 1), span2d(d_out, h, w, out_pitch, 1)),
              "remove_single_pixels does not run in place");
  return launch(ctx, remove_single_pixels_kernel, dim3((w + 63) / 64, (h + 3) / 4), dim3(64, 4), 0, d_in, h, w,
                pitch, d_out, out_pitch);
}

}  // extern "C"
