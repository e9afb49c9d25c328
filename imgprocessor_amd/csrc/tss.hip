// tss.hip — temporal signal stability on gfx950: what uncertainty/temporalSignalStability.py needs
// after the per-pixel line fit (ipa_stack_linregress_dev of dark.hip).
//   ipa_tss_event_length_dev  uncertainty/temporalSignalStability.py:56-66 and _calcAvgLen :83-107
//                             (fn_imgs, diff, median_filter(diff, 5), evt, the run lengths)
//   ipa_tss_finish_dev        uncertainty/temporalSignalStability.py:72-78 (maximum_filter(i, 3),
//                             avlen[i] = 0, maximum_filter(avlen, 3), median_filter(avlen, 3))
//
// The 5 x 5 x 5 median is never formed.  It is compared with +-c, c = 0.5 * error of the CENTRE
// pixel, the same for every frame; the median of 125 finite values is above c exactly when at least
// 63 of them are, and below -c exactly when at least 63 are below -c.  The count over the window is
// the sum of five plane counts (the 5 x 5 window of one frame against +-c), so a workgroup walks
// the frames once and a pixel carries the counts of the last five planes.
//
// Event kernel: a workgroup of 256 lanes owns a 64 x 16 tile, a lane four vertically adjacent
// pixels of it.  Per frame the 68 x 20 residuals of the tile and its 2-pixel halo (scipy `reflect`
// beyond the image, with the halo pixel's own offset and ascent) go to LDS as float64, double
// buffered, one barrier per frame; the next frame's samples are requested before the counting
// starts.  A lane reads 8 x 5 residuals for its four pixels (10 LDS reads a pixel instead of 25) and
// counts each sign with a compare and an add-with-carry; a plane's two counts are then packed into
// one word.  The z axis needs no stored planes either: for T >= 2 the
// reflected planes -2, -1, T, T + 1 are planes 1, 0, T - 1, T - 2, which are at hand when they are
// needed.  Run statistics stay in registers; avlen is written once.  No (T, h, w) intermediate, no
// workspace.
//
// Everything is float64, every operation correctly rounded and unfused (Makefile + pragma).
// NaN samples: undefined (scipy's own selection is order dependent there).  A NaN error compares
// false everywhere: no event, length 0.
#include "common.hpp"
#include "frame_args.hpp"
#include "launch.hpp"
#include "nlf_fn.hpp"

#pragma clang fp contract(off)

namespace ipa {
namespace {

constexpr int kTssMaxT = 64;
constexpr int kTssThreads = 256;
constexpr int kTssTileW = 64, kTssTileH = 16;   // output pixels of a workgroup
constexpr int kTssPx = 4;                       // rows of a lane
constexpr int kTssHalo = 2;
constexpr int kTssLdsW = kTssTileW + 2 * kTssHalo, kTssLdsH = kTssTileH + 2 * kTssHalo;
constexpr int kTssCells = kTssLdsW * kTssLdsH;
constexpr int kTssSlots = (kTssCells + kTssThreads - 1) / kTssThreads;   // staged cells of a lane
constexpr unsigned kTssMajority = 63;               // rank 62 of 125, counted from 0, is the median
static_assert(kTssTileH == kTssPx * (kTssThreads / kTssTileW), "a lane owns kTssPx rows of the tile");

struct TssTimes {
  double x[kTssMaxT];
};

struct TssArgs {
  const void* stack;
  long pitch, frame_stride;
  int T, h, w, tiles_x;
  const double* offset;
  const double* ascent;
  const double* error;
  long plane_pitch;
  double* avlen;
  long avlen_pitch;
  unsigned char* zero_mask;   // may be null
  long mask_pitch;
  unsigned char* events;      // may be null
  long ev_pitch, ev_frame_stride;
};

// scipy.ndimage `reflect` (d c b a | a b c d) of any index, reflected as often as it takes
__device__ inline int tss_reflect(int i, int n) {
  const int p = 2 * n;
  int m = i % p;
  if (m < 0) m += p;
  return m < n ? m : p - 1 - m;
}

// above += v > c; below += v < nc.  IPA_TSS_PLAIN_COUNT=1 (make DEFS=-DIPA_TSS_PLAIN_COUNT=1) builds the
// plain C++ form, for another target or to look at what a later compiler makes of it.  With ROCm 7 the
// compiler, given `n += v > c`, forms the 200 lane masks of a frame first and adds them up as a
// tree: more masks than there are scalar registers, spilled through v_writelane (1.13 ms where the
// form below takes 0.61 ms, 15 uint16 4K frames).  The default writes each comparison as one compare
// into VCC and one add of the carry - wave64 and the VOP2 carry form of gfx9, which is what the
// library is built for.
#ifndef IPA_TSS_PLAIN_COUNT
#define IPA_TSS_PLAIN_COUNT 0
#endif
__device__ inline void count_beyond(unsigned& above, unsigned& below, double v, double c, double nc) {
#if IPA_TSS_PLAIN_COUNT
  above += v > c ? 1u : 0u;
  below += v < nc ? 1u : 0u;
#else
  asm("v_cmp_gt_f64 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, 0, %0, vcc" : "+v"(above) : "v"(v), "v"(c) : "vcc");
  asm("v_cmp_lt_f64 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, 0, %0, vcc" : "+v"(below) : "v"(v), "v"(nc) : "vcc");
#endif
}

template <typename E>
__global__ void __launch_bounds__(kTssThreads)
tss_event_length_kernel(TssArgs a, TssTimes t) {
  __shared__ double lds[2][kTssCells];
  const int tid = threadIdx.x;
  const int by = blockIdx.x / a.tiles_x, bx = blockIdx.x - by * a.tiles_x;
  const int x0 = bx * kTssTileW, y0 = by * kTssTileH;
  const int lx = tid & (kTssTileW - 1), ly = (tid / kTssTileW) * kTssPx;

  // the cells of the halo tile this lane stages: where they come from and whose line they lie on
  long src[kTssSlots];
  double off[kTssSlots], asc[kTssSlots];
  E cur[kTssSlots];
  const E* st = (const E*)a.stack;
#pragma unroll
  for (int i = 0; i < kTssSlots; i++) {
    const int cell = tid + i * kTssThreads;
    src[i] = -1;
    off[i] = asc[i] = 0.0;
    cur[i] = E(0);
    if (cell < kTssCells) {
      const int cy = cell / kTssLdsW, cx = cell - cy * kTssLdsW;
      const int gy = tss_reflect(y0 - kTssHalo + cy, a.h), gx = tss_reflect(x0 - kTssHalo + cx, a.w);
      src[i] = (long)gy * a.pitch + gx;
      const long po = (long)gy * a.plane_pitch + gx;
      off[i] = a.offset[po];
      asc[i] = a.ascent[po];
      cur[i] = st[src[i]];
    }
  }

  // the lane's pixels and their thresholds
  const int x = x0 + lx;
  bool live[kTssPx];
  double c[kTssPx], nc[kTssPx];
#pragma unroll
  for (int j = 0; j < kTssPx; j++) {
    const int y = y0 + ly + j;
    live[j] = x < a.w && y < a.h;
    c[j] = live[j] ? 0.5 * a.error[(long)y * a.plane_pitch + x] : 0.0;
    nc[j] = -c[j];
  }

  // plane counts of the five planes around a frame, `above` in the low half, `below` in the high
  unsigned r0[kTssPx], r1[kTssPx], r2[kTssPx], r3[kTssPx], r4[kTssPx];
  int nvals[kTssPx], nclusters[kTssPx];
  bool last[kTssPx];
#pragma unroll
  for (int j = 0; j < kTssPx; j++) {
    r0[j] = r1[j] = r2[j] = r3[j] = r4[j] = 0;
    nvals[j] = nclusters[j] = 0;
    last[j] = false;
  }

  // frame k is decided by the window r0..r4; then the window moves on by one plane
  auto emit = [&](int k) {
#pragma unroll
    for (int j = 0; j < kTssPx; j++) {
      const unsigned s = r0[j] + r1[j] + r2[j] + r3[j] + r4[j];
      const bool evt = (s & 0xffffu) >= kTssMajority || (s >> 16) >= kTssMajority;
      if (evt) {
        nvals[j]++;
        if (!last[j]) nclusters[j]++;
      }
      last[j] = evt;
      if (a.events && live[j])
        a.events[(long)k * a.ev_frame_stride + (long)(y0 + ly + j) * a.ev_pitch + x] = evt ? 1 : 0;
      r0[j] = r1[j];
      r1[j] = r2[j];
      r2[j] = r3[j];
      r3[j] = r4[j];
    }
  };

  for (int s = 0; s < a.T; s++) {
    double* buf = lds[s & 1];
    const double ts = t.x[s];
#pragma unroll
    for (int i = 0; i < kTssSlots; i++) {
      const int cell = tid + i * kTssThreads;
      if (cell < kTssCells) buf[cell] = (double)cur[i] - (off[i] + ts * asc[i]);
    }
    if (s + 1 < a.T) {
      const E* nx = st + (long)(s + 1) * a.frame_stride;
#pragma unroll
      for (int i = 0; i < kTssSlots; i++)
        if (src[i] >= 0) cur[i] = nx[src[i]];
    }
    // one barrier a frame: the other buffer is written next, and nobody writes this one again
    // before every lane has passed the next barrier
    __syncthreads();
    // above and below in counters of their own, a compare and an add-with-carry each (count_beyond)
    unsigned above[kTssPx], below[kTssPx];
#pragma unroll
    for (int j = 0; j < kTssPx; j++) above[j] = below[j] = 0;
    const double* row = buf + ly * kTssLdsW + lx;
#pragma unroll
    for (int rr = 0; rr < kTssPx + 2 * kTssHalo; rr++) {
#pragma unroll
      for (int cc = 0; cc < 2 * kTssHalo + 1; cc++) {
        const double v = row[rr * kTssLdsW + cc];
#pragma unroll
        for (int j = 0; j < kTssPx; j++)
          if (rr - j >= 0 && rr - j <= 2 * kTssHalo) count_beyond(above[j], below[j], v, c[j], nc[j]);
      }
    }
    unsigned cnt[kTssPx];
#pragma unroll
    for (int j = 0; j < kTssPx; j++) cnt[j] = above[j] | (below[j] << 16);
    if (s == 0) {          // plane 0 is also the reflected plane -1
#pragma unroll
      for (int j = 0; j < kTssPx; j++) r1[j] = r2[j] = cnt[j];
    } else if (s == 1) {   // plane 1 is also the reflected plane -2
#pragma unroll
      for (int j = 0; j < kTssPx; j++) r0[j] = r3[j] = cnt[j];
    } else {
#pragma unroll
      for (int j = 0; j < kTssPx; j++) r4[j] = cnt[j];
      emit(s - 2);
    }
  }
  // r2, r3 hold planes T - 2, T - 1: the reflected plane T is T - 1, plane T + 1 is T - 2
  unsigned before_last[kTssPx];
#pragma unroll
  for (int j = 0; j < kTssPx; j++) {
    before_last[j] = r2[j];
    r4[j] = r3[j];
  }
  emit(a.T - 2);
#pragma unroll
  for (int j = 0; j < kTssPx; j++) r4[j] = before_last[j];
  emit(a.T - 1);

#pragma unroll
  for (int j = 0; j < kTssPx; j++) {
    if (!live[j]) continue;
    const int y = y0 + ly + j;
    a.avlen[(long)y * a.avlen_pitch + x] = nclusters[j] == 0 ? 0.0 : (double)nvals[j] / (double)nclusters[j];
    if (a.zero_mask) a.zero_mask[(long)y * a.mask_pitch + x] = nclusters[j] == 0 ? 1 : 0;
  }
}

// ---- the 2-D tail: three 3 x 3 stages with the edge repeated, staged through LDS.  A stage's value
// at a position beyond the image is its value at the clamped position, so every cell is computed AT
// its clamped position, from that position's own clamped neighbours.
constexpr int kFinW = 32, kFinH = 8;
constexpr int kFin2W = kFinW + 4, kFin2H = kFinH + 4;   // a2: two rings
constexpr int kFin3W = kFinW + 2, kFin3H = kFinH + 2;   // a3: one ring

__device__ inline int clampi(int i, int n) { return i < 0 ? 0 : i >= n ? n - 1 : i; }

__global__ void __launch_bounds__(kTssThreads)
tss_finish_kernel(const double* __restrict__ a1, const unsigned char* __restrict__ m0, int h, int w, long pitch,
                  long mask_pitch, int tiles_x, double* __restrict__ out, long out_pitch) {
  __shared__ double s2[kFin2H * kFin2W];
  __shared__ double s3[kFin3H * kFin3W];
  const int by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
  const int x0 = bx * kFinW, y0 = by * kFinH;
  // a2 = a1 with zeros where the 3 x 3 dilated mask is set
  for (int cell = threadIdx.x; cell < kFin2H * kFin2W; cell += kTssThreads) {
    const int cy = cell / kFin2W, cx = cell - cy * kFin2W;
    const int py = clampi(y0 - 2 + cy, h), px = clampi(x0 - 2 + cx, w);
    bool m1 = false;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
      for (int dx = -1; dx <= 1; dx++)
        m1 = m1 || m0[(long)clampi(py + dy, h) * mask_pitch + clampi(px + dx, w)] != 0;
    s2[cell] = m1 ? 0.0 : a1[(long)py * pitch + px];
  }
  __syncthreads();
  // a3 = 3 x 3 maximum of a2
  for (int cell = threadIdx.x; cell < kFin3H * kFin3W; cell += kTssThreads) {
    const int cy = cell / kFin3W, cx = cell - cy * kFin3W;
    const int py = clampi(y0 - 1 + cy, h), px = clampi(x0 - 1 + cx, w);
    double m = s2[(clampi(py - 1, h) - (y0 - 2)) * kFin2W + clampi(px - 1, w) - (x0 - 2)];
#pragma unroll
    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
      for (int dx = -1; dx <= 1; dx++) {
        const double v = s2[(clampi(py + dy, h) - (y0 - 2)) * kFin2W + clampi(px + dx, w) - (x0 - 2)];
        m = v > m ? v : m;
      }
    s3[cell] = m;
  }
  __syncthreads();
  // a4 = 3 x 3 median of a3, zeros where a3 is zero
  const int px = x0 + (threadIdx.x & (kFinW - 1)), py = y0 + threadIdx.x / kFinW;
  if (px >= w || py >= h) return;
  double win[3][3];
#pragma unroll
  for (int dx = -1; dx <= 1; dx++)
#pragma unroll
    for (int dy = -1; dy <= 1; dy++)
      win[dx + 1][dy + 1] = s3[(clampi(py + dy, h) - (y0 - 1)) * kFin3W + clampi(px + dx, w) - (x0 - 1)];
  const double centre = win[1][1];
  const double med = median9(win);
  out[(long)py * out_pitch + px] = centre == 0.0 ? 0.0 : med;
}

}  // namespace
}  // namespace ipa

using namespace ipa;

extern "C" {

int ipa_tss_event_length_dev(ipa_ctx* ctx, const void* d_stack, int dtype, int T, int h, int w, long pitch,
                             long frame_stride, const double* times, const double* d_offset,
                             const double* d_ascent, const double* d_error, long plane_pitch, double* d_avlen,
                             long avlen_pitch, unsigned char* d_zero_mask, long mask_pitch,
                             unsigned char* d_events, long ev_pitch, long ev_frame_stride) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  if (T > kTssMaxT) IPA_UNSUPPORTED(ctx, "tss_event_length: at most %d frames (got %d)", kTssMaxT, T);
  IPA_REQUIRE(ctx, T >= 2, "tss_event_length: needs at least 2 frames (got %d)", T);
  IPA_REQUIRE(ctx, d_stack && times && d_offset && d_ascent && d_error && d_avlen, "tss_event_length: null pointer");
  IPA_REQUIRE(ctx, h > 0 && w > 0, "tss_event_length: empty image");
  const long tx = ((long)w + kTssTileW - 1) / kTssTileW, ty = ((long)h + kTssTileH - 1) / kTssTileH;
  IPA_REQUIRE(ctx, tx * ty <= 0x7fffffffL, "tss_event_length: image too large");
  IPA_REQUIRE(ctx, pitch >= w && plane_pitch >= w && avlen_pitch >= w && (!d_zero_mask || mask_pitch >= w) &&
                       (!d_events || ev_pitch >= w),
              "tss_event_length: pitch smaller than width");
  IPA_REQUIRE(ctx, frame_stride >= (long)(h - 1) * pitch + w, "tss_event_length: frames overlap");
  IPA_REQUIRE(ctx, !d_events || ev_frame_stride >= (long)(h - 1) * ev_pitch + w,
              "tss_event_length: event frames overlap");
  if (!known_dtype(dtype))
    IPA_UNSUPPORTED(ctx, "tss_event_length: frames are uint8 / uint16 / float32 / float64 (got dtype %d)", dtype);
  // outputs first: no output may touch another output or an input
  const Span spans[] = {span2d(d_avlen, h, w, avlen_pitch, 8),
                        span2d(d_zero_mask, h, w, mask_pitch, 1),
                        span_stack(d_events, T, h, w, ev_pitch, ev_frame_stride, 1),
                        span_stack(d_stack, T, h, w, pitch, frame_stride, ipa_dtype_size(dtype)),
                        span2d(d_offset, h, w, plane_pitch, 8),
                        span2d(d_ascent, h, w, plane_pitch, 8),
                        span2d(d_error, h, w, plane_pitch, 8)};
  IPA_REQUIRE(ctx, !written_overlaps(spans, 3), "tss_event_length: an output overlaps another array");
  TssTimes t;
  for (int k = 0; k < kTssMaxT; k++) t.x[k] = k < T ? times[k] : 0.0;
  TssArgs a;
  a.stack = d_stack;
  a.pitch = pitch;
  a.frame_stride = frame_stride;
  a.T = T;
  a.h = h;
  a.w = w;
  a.tiles_x = (int)tx;
  a.offset = d_offset;
  a.ascent = d_ascent;
  a.error = d_error;
  a.plane_pitch = plane_pitch;
  a.avlen = d_avlen;
  a.avlen_pitch = avlen_pitch;
  a.zero_mask = d_zero_mask;
  a.mask_pitch = mask_pitch;
  a.events = d_events;
  a.ev_pitch = ev_pitch;
  a.ev_frame_stride = ev_frame_stride;
  return by_dtype(dtype, [&](auto e) {
    using E = decltype(e);
    return launch(ctx, tss_event_length_kernel<E>, dim3((unsigned)(tx * ty)), dim3(kTssThreads), 0, a, t);
  });
}

int ipa_tss_finish_dev(ipa_ctx* ctx, const double* d_mean, const unsigned char* d_mask, int h, int w, long pitch,
                       long mask_pitch, double* d_out, long out_pitch) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  IPA_REQUIRE(ctx, d_mean && d_mask && d_out, "tss_finish: null pointer");
  IPA_REQUIRE(ctx, h > 0 && w > 0, "tss_finish: empty image");
  const long tx = ((long)w + kFinW - 1) / kFinW, ty = ((long)h + kFinH - 1) / kFinH;
  IPA_REQUIRE(ctx, tx * ty <= 0x7fffffffL, "tss_finish: image too large");
  IPA_REQUIRE(ctx, pitch >= w && mask_pitch >= w && out_pitch >= w, "tss_finish: pitch smaller than width");
  const Span out = span2d(d_out, h, w, out_pitch, 8);
  IPA_REQUIRE(ctx, !overlap(out, span2d(d_mean, h, w, pitch, 8)) && !overlap(out, span2d(d_mask, h, w, mask_pitch, 1)),
              "tss_finish does not run in place");
  return launch(ctx, tss_finish_kernel, dim3((unsigned)(tx * ty)), dim3(kTssThreads), 0, d_mean, d_mask, h, w, pitch,
                mask_pitch, (int)tx, d_out, out_pitch);
}

}  // extern "C"
