// nlm.hip — non-local-means denoising on gfx950:
//   ipa_nl_means_dev     skimage.restoration.denoise_nl_means(image, patch_size, patch_distance, h,
//                        fast_mode=True, sigma) as camera/CameraCalibration.py:461-474 calls it
//   ipa_nan_to_zero_dev  image[np.isnan(image)] = 0 (camera/CameraCalibration.py:467)
//
// With s = patch_size (even: s + 1), o = s / 2, d = patch_distance, P the image continued by
// numpy's `reflect` (no edge repeat, period 2 (n - 1)):
//   D(p, t) = max((sum_q (P[q] - P[q + t])^2 - 2 sigma^2 (s - 1)^2) / (s^2 h^2), 0)
//             q over the (s - 1) x (s - 1) window at offsets -o + 1 ... +o from p in both axes
//   w(p, t) = D > 5 ? 0 : exp(-D),  w(p, 0) = 2
//   out[p]  = sum_t w P[p + t] / sum_t w,   t in [-d, d]^2
//
// A workgroup of 4 waves owns an output tile of (65 - W) x 4 R pixels, W = s - 1, and holds it
// with a halo of d + o pixels in LDS, filled through the reflect index map.  A wave owns R output
// rows; its 64 lanes are 64 adjacent columns, W - 1 of them only there for their neighbours'
// windows.  For every shift t the wave walks down its R + W - 1 window rows: a lane squares one
// difference per row, the W squares of a window row come from the neighbouring lanes through DPP
// wave shifts, and the last W row sums are kept in registers (the walk is unrolled, so the ring
// index is static).  A pixel-shift pair costs one difference, W - 1 lane shifts and 2 W - 1
// additions, not W^2 differences.  The W row sums are added afresh for every pixel: a running
// sum would save W - 2 additions and carry the rounding of every row above it.  sum w and
// sum w (P[p + t] - P[p]) stay in registers over all (2 d + 1)^2 shifts, and the result is
// P[p] + sum w (P[p + t] - P[p]) / sum w with one division: the weighted mean, exact where every
// surviving neighbour equals the pixel (a constant image, a cut-off only the self pair passes).
#include "common.hpp"
#include "frame_args.hpp"
#include "launch.hpp"

namespace ipa {
namespace {

constexpr int kNlmWaves = 4;
constexpr int kNlmLdsBytes = 65536;   // static + dynamic LDS a workgroup may ask for

template <typename T> struct NlmRows;           // output rows per wave
template <> struct NlmRows<float> { static constexpr int R = 16; };
template <> struct NlmRows<double> { static constexpr int R = 8; };

// DPP wave shifts (GFX9): the value of lane - 1 / lane + 1, 0 at the ends of the wave
__device__ inline int dpp_from_left(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xf, 0xf, true); }
__device__ inline int dpp_from_right(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x130, 0xf, 0xf, true); }
__device__ inline float from_left(float v) { return __int_as_float(dpp_from_left(__float_as_int(v))); }
__device__ inline float from_right(float v) { return __int_as_float(dpp_from_right(__float_as_int(v))); }
__device__ inline double from_left(double v) {
  return __hiloint2double(dpp_from_left(__double2hiint(v)), dpp_from_left(__double2loint(v)));
}
__device__ inline double from_right(double v) {
  return __hiloint2double(dpp_from_right(__double2hiint(v)), dpp_from_right(__double2loint(v)));
}

__device__ inline float exp_neg(float d) { return __expf(-d); }
__device__ inline double exp_neg(double d) { return exp(-d); }

// numpy `reflect`: ... 2 1 | 0 1 2 ... n-1 | n-2 n-3 ...   (n >= 2)
__device__ inline int reflect_idx(int i, int n) {
  const int p = 2 * (n - 1);
  int m = i % p;
  if (m < 0) m += p;
  return m < n ? m : p - m;
}

struct NlmArgs {
  const void* src;
  void* dst;
  long pitch, frame_stride, dst_pitch, dst_frame_stride;
  int h, w, d;
  double inv;   // 1 / (s^2 h^2)
  double sig;   // 2 sigma^2 (s - 1)^2
};

template <typename T, int W>
__global__ void __launch_bounds__(64 * kNlmWaves)
nlm_kernel(NlmArgs a) {
  constexpr int R = NlmRows<T>::R;
  constexpr int O = W / 2;            // s / 2
  constexpr int TX = 65 - W, TY = kNlmWaves * R;
  extern __shared__ __align__(16) unsigned char nlm_lds[];
  T* tile = (T*)nlm_lds;
  const int d = a.d;
  const int lw = 64 + 2 * d, lh = TY + W - 1 + 2 * d;
  const int x0 = blockIdx.x * TX - (O - 1), y0 = blockIdx.y * TY - (O - 1);   // lane 0, window row 0
  const T* src = (const T*)a.src + (long)blockIdx.z * a.frame_stride;

  for (int ly = threadIdx.x >> 6; ly < lh; ly += kNlmWaves) {
    const long row = (long)reflect_idx(y0 - d + ly, a.h) * a.pitch;
    for (int lx = threadIdx.x & 63; lx < lw; lx += 64)
      tile[ly * lw + lx] = src[row + reflect_idx(x0 - d + lx, a.w)];
  }
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int oy = blockIdx.y * TY + wave * R;   // first output row of the wave
  if (oy >= a.h) return;
  const T inv = (T)a.inv, sig = (T)a.sig;
  const T* base = tile + (wave * R + d) * lw + d + lane;   // window row 0 of the wave, this lane

  T sw[R], sv[R];
#pragma unroll
  for (int i = 0; i < R; i++) sw[i] = sv[i] = (T)0;

#pragma unroll 1
  for (int tr = -d; tr <= d; tr++) {
#pragma unroll 1
    for (int tc = -d; tc <= d; tc++) {
      const T* pa = base;
      const T* pb = base + tr * lw + tc;
      const T self = (tr == 0 && tc == 0) ? (T)2 : (T)0;
      T ring[W];
#pragma unroll
      for (int k = 0; k < R + W - 1; k++) {
        const T df = pa[k * lw] - pb[k * lw];
        const T q = df * df;
        T hs = q, l = q, r = q;
#pragma unroll
        for (int j = 1; j <= O; j++) {
          r = from_right(r);
          hs += r;
          if (j < O) {
            l = from_left(l);
            hs += l;
          }
        }
        ring[k % W] = hs;
        if (k >= W - 1) {
          const int i = k - (W - 1);   // output row; its pixel is window row i + O - 1
          T v = ring[0];
#pragma unroll
          for (int j = 1; j < W; j++) v += ring[j];
          T dist = (v - sig) * inv;
          dist = dist > (T)0 ? dist : (T)0;
          T wt = dist > (T)5 ? (T)0 : exp_neg(dist);
          wt = self != (T)0 ? self : wt;
          sw[i] += wt;
          sv[i] += wt * (pb[(i + O - 1) * lw] - pa[(i + O - 1) * lw]);
        }
      }
    }
  }

  const int x = x0 + lane;
  if (lane < O - 1 || lane >= 64 - O || x >= a.w) return;
  T* dst = (T*)a.dst + (long)blockIdx.z * a.dst_frame_stride;
#pragma unroll
  for (int i = 0; i < R; i++)
    if (oy + i < a.h) dst[(long)(oy + i) * a.dst_pitch + x] = base[(i + O - 1) * lw] + sv[i] / sw[i];
}

template <typename T>
__global__ void __launch_bounds__(256)
nan_to_zero_kernel(T* img, int h, int w, long pitch, long frame_stride) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= w || y >= h) return;
  T* p = img + (long)blockIdx.z * frame_stride + (long)y * pitch + x;
  const T v = *p;
  if (v != v) *p = (T)0;
}

template <typename T>
size_t nlm_lds_bytes(int s, int d) {
  return (size_t)(kNlmWaves * NlmRows<T>::R + s - 2 + 2 * d) * (64 + 2 * d) * sizeof(T);
}

// the kernel of the odd patch size s = 3 ... 11 (W = s - 1) over n frames; W listed last first: pick
// instantiates, and the code object lays out, from the back
template <typename T>
int nlm_dispatch(ipa_ctx* ctx, int s, int n, const NlmArgs& a) {
  const size_t lds = nlm_lds_bytes<T>(s, a.d);
  IPA_REQUIRE(ctx, lds <= (size_t)kNlmLdsBytes,
              "nl_means: the tile of patch_size %d, patch_distance %d needs %zu bytes of LDS (limit %d)", s, a.d, lds,
              kNlmLdsBytes);
  constexpr int TY = kNlmWaves * NlmRows<T>::R;
  return pick<10, 8, 6, 4, 2>(s - 1, [&](auto W) {
    return launch(ctx, nlm_kernel<T, W()>, dim3((a.w + 64 - W()) / (65 - W()), (a.h + TY - 1) / TY, n),
                  dim3(64 * kNlmWaves), lds, a);
  });
}

}  // namespace
}  // namespace ipa

using namespace ipa;

extern "C" {

int ipa_nl_means_dev(ipa_ctx* ctx, const void* d_src, int dtype, int n, int h, int w, long pitch,
                     long frame_stride, int patch_size, int patch_distance, double h_cut, double sigma,
                     void* d_dst, long dst_pitch, long dst_frame_stride) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  IPA_REQUIRE(ctx, d_src && d_dst, "nl_means: null pointer");
  IPA_REQUIRE(ctx, n >= 1 && n <= 65535 && h >= 2 && w >= 2,
              "nl_means needs 1 ... 65535 frames of at least 2 x 2 pixels");
  IPA_REQUIRE(ctx, pitch >= w && dst_pitch >= w, "nl_means: pitch smaller than width");
  IPA_REQUIRE(ctx, n == 1 || (frame_stride >= (long)(h - 1) * pitch + w &&
                              dst_frame_stride >= (long)(h - 1) * dst_pitch + w),
              "nl_means: frames overlap");
  if (dtype != IPA_F32 && dtype != IPA_F64)
    IPA_UNSUPPORTED(ctx, "nl_means: frames are float32 / float64 (got dtype %d)", dtype);
  IPA_REQUIRE(ctx, patch_size >= 2 && patch_size <= 11, "nl_means: patch_size %d is not in 2 ... 11", patch_size);
  IPA_REQUIRE(ctx, patch_distance >= 0, "nl_means: patch_distance %d is negative", patch_distance);
  IPA_REQUIRE(ctx, h_cut > 0 && sigma >= 0, "nl_means: h must be positive and sigma not negative");
  const size_t es = ipa_dtype_size(dtype);
  IPA_REQUIRE(ctx, !overlap(span_stack(d_src, n, h, w, pitch, frame_stride, es),
                            span_stack(d_dst, n, h, w, dst_pitch, dst_frame_stride, es)),
              "nl_means does not run in place");
  const int s = patch_size | 1;   // an even size is the next odd one
  NlmArgs a;
  a.src = d_src;
  a.dst = d_dst;
  a.pitch = pitch;
  a.frame_stride = frame_stride;
  a.dst_pitch = dst_pitch;
  a.dst_frame_stride = dst_frame_stride;
  a.h = h;
  a.w = w;
  a.d = patch_distance;
  a.inv = 1.0 / ((double)s * s * h_cut * h_cut);
  a.sig = 2.0 * sigma * sigma * (double)(s - 1) * (s - 1);
  return by_float(dtype, [&](auto t) { return nlm_dispatch<decltype(t)>(ctx, s, n, a); });
}

int ipa_nan_to_zero_dev(ipa_ctx* ctx, void* d_img, int dtype, int n, int h, int w, long pitch,
                        long frame_stride) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  IPA_REQUIRE(ctx, d_img, "nan_to_zero: null pointer");
  IPA_REQUIRE(ctx, n >= 1 && n <= 65535 && h > 0 && w > 0, "nan_to_zero needs 1 ... 65535 non-empty frames");
  IPA_REQUIRE(ctx, pitch >= w, "nan_to_zero: pitch smaller than width");
  if (dtype != IPA_F32 && dtype != IPA_F64)
    IPA_UNSUPPORTED(ctx, "nan_to_zero: frames are float32 / float64 (got dtype %d)", dtype);
  dim3 grid((w + 63) / 64, (h + 3) / 4, n), block(64, 4);
  return by_float(dtype, [&](auto t) {
    return launch(ctx, nan_to_zero_kernel<decltype(t)>, grid, block, 0, d_img, h, w, pitch,
                  frame_stride);
  });
}

}  // extern "C"
