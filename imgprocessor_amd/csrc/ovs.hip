// ovs.hip — object / vignetting separation on gfx950: the refinement loop of
// camera/flatField/vignettingFromRandomSteps.py ("Method D": one object imaged at random positions).
//   ipa_ovs_object_dev           :241-249  the object from the current flat field
//   ipa_ovs_flatfield_dev        :253-265  the new flat field from the object
//   ipa_masked_running_mean_dev  :146-151  one MaskedMovingAverage.update(data, mask)
//
// Both steps are N perspective warps (cv2.warpPerspective: bilinear, coordinates rounded to 1/32 px,
// constant border 0), a division and a masked running mean per pixel.  A lane owns one output pixel
// and walks the N fitted images in order; no warped frame and no (N, h, w) intermediate exists.
//
// The coordinates are HomographyCoord::get and the weights axis_split<kLinear> of sampler.hpp, what
// ipa_warp_perspective_dev runs on a float64 image with IPA_INTER_LINEAR | IPA_INTER_Q5.  The object
// step samples the flat field through sample<double, kLinear, double> itself.  The flat-field step
// samples an image that exists nowhere - tap (r, c) of fit k is NaN where masked, fit / object
// otherwise - so sample_taps() below restates sample() over a tap functor, operation for operation:
// sample()'s interior and border branches are the same arithmetic (wx[0] * v0, fma(wx[1], v1, .),
// wy[0] * r0, fma(wy[1], r1, .)) with 0 for a tap outside the frame, and a footprint wholly outside
// is 0 without a tap being formed - the cheap way out for the many flat-field pixels outside a fit.
//
// Everything is float64, every division IEEE, nothing fused but the two explicit fma of the sampler
// (Makefile + pragma).  The N matrices go through the context's table buffer (ipa_tab_upload) and
// are read at wave-uniform addresses.  A workgroup is a 64 x 4 tile: neighbouring lanes gather
// neighbouring source pixels under the near-identity homographies of a fit.
#include "common.hpp"
#include "frame_args.hpp"
#include "launch.hpp"
#include "sampler.hpp"

#include <float.h>

#pragma clang fp contract(off)

namespace ipa {
namespace {

constexpr int kOvsMaxN = 64;
constexpr int kOvsThreads = 256;

// MaskedMovingAverage.update for one accepted value
__device__ __forceinline__ void running_mean(double& avg, int& n, double x) {
  n += 1;
  avg = n == 1 ? x : avg + (x - avg) / (double)n;
}

__device__ __forceinline__ void coord_of(const double* __restrict__ mats, int k, int x, int y, double& sx,
                                         double& sy) {
  HomographyCoord c;
#pragma unroll
  for (int i = 0; i < 9; i++) c.m[i] = mats[k * 9 + i];
  c.get(x, y, sx, sy);
}

// sample<double, kLinear, double>(s, sx, sy, 0.0) with IPA_BORDER_CONSTANT over tap(row, column)
// instead of a load; s gives the frame's size and the coordinate rule
template <typename Tap>
__device__ __forceinline__ double sample_taps(const SrcView& s, double sx, double sy, const Tap& tap) {
  if (!(sx > (double)-kCoordLimit && sx < (double)kCoordLimit && sy > (double)-kCoordLimit &&
        sy < (double)kCoordLimit))
    return 0.0;
  int ix0, iy0;
  double wx[2], wy[2];
  axis_split<kLinear, double, double>(s, sx, ix0, wx);
  axis_split<kLinear, double, double>(s, sy, iy0, wy);
  if (ix0 >= s.w || ix0 + 2 <= 0 || iy0 >= s.h || iy0 + 2 <= 0) return 0.0;  // whole footprint outside
  double out = 0.0;
#pragma unroll
  for (int r = 0; r < 2; r++) {
    const int yy = resolve_idx(iy0 + r, s.h, IPA_BORDER_CONSTANT);
    double rs = 0.0;
#pragma unroll
    for (int c = 0; c < 2; c++) {
      const int xx = resolve_idx(ix0 + c, s.w, IPA_BORDER_CONSTANT);
      const double v = (yy < 0 || xx < 0) ? 0.0 : tap(yy, xx);
      rs = c == 0 ? wx[0] * v : ipa_fma(wx[c], v, rs);
    }
    out = r == 0 ? wy[0] * rs : ipa_fma(wy[r], rs, out);
  }
  return out;
}

__device__ __forceinline__ SrcView view_of(const void* base, unsigned bytes, int h, int w, int pitch) {
  SrcView s;
  s.rsrc = make_rsrc(base, bytes);
  s.h = h;
  s.w = w;
  s.pitch = pitch;
  s.border = IPA_BORDER_CONSTANT;
  s.q5 = 1;
  s.cubic_a = 0.f;
  s.lanczos = nullptr;
  return s;
}

// ---- (a) object(y, x) = running mean over k of fit_k(y, x) / ff(M_k (x, y, 1)), where that is != 0
template <typename E>
__global__ void __launch_bounds__(kOvsThreads)
ovs_object_kernel(const double* __restrict__ ff, int fh, int fw, int ff_pitch, unsigned ff_bytes,
                  const E* __restrict__ fits, long fit_pitch, long fit_stride, const double* __restrict__ mats,
                  int n, int oh, int ow, int tiles_x, double* __restrict__ obj, long obj_pitch,
                  int* __restrict__ count, long count_pitch) {
  int x, y;
  if (!tile_px(tiles_x, oh, ow, x, y)) return;
  const SrcView s = view_of(ff, ff_bytes, fh, fw, ff_pitch);
  const E* px = fits + (long)y * fit_pitch + x;
  double avg = 0.0;
  int cnt = 0;
  for (int k = 0; k < n; k++) {
    const double f = (double)px[(long)k * fit_stride];
    double sx, sy;
    coord_of(mats, k, x, y, sx, sy);
    const double wgt = sample<double, kLinear, double>(s, sx, sy, 0.0);
    if (wgt != 0.0) running_mean(avg, cnt, f / wgt);   // NaN != 0: accepted, as in numpy
  }
  obj[(long)y * obj_pitch + x] = avg;
  count[(long)y * count_pitch + x] = cnt;
}

// ---- (b) ff(y, x) = running mean over k of nan_to_num(warp(fit_k / object, masked -> NaN)), where != 0
template <typename E>
__global__ void __launch_bounds__(kOvsThreads)
ovs_flatfield_kernel(const double* __restrict__ obj, long obj_pitch, const E* __restrict__ fits, long fit_pitch,
                     long fit_stride, const unsigned char* __restrict__ masks, long mask_pitch, long mask_stride,
                     const double* __restrict__ mats, int n, int oh, int ow, int fh, int fw, int tiles_x,
                     double* __restrict__ ff, long ff_pitch, int* __restrict__ count, long count_pitch, int clip01,
                     double* __restrict__ sub, int sub_step, long sub_pitch) {
  int x, y;
  if (!tile_px(tiles_x, fh, fw, x, y)) return;
  const SrcView s = view_of(obj, 0u, oh, ow, 0);   // size and coordinate rule only: the taps are formed below
  double avg = 0.0;
  int cnt = 0;
  for (int k = 0; k < n; k++) {
    double sx, sy;
    coord_of(mats, k, x, y, sx, sy);
    const E* fit = fits + (long)k * fit_stride;
    const unsigned char* mask = masks + (long)k * mask_stride;
    double v = sample_taps(s, sx, sy, [&](int r, int c) {
      if (mask[(long)r * mask_pitch + c]) return (double)NAN;
      return (double)fit[(long)r * fit_pitch + c] / obj[(long)r * obj_pitch + c];
    });
    // np.nan_to_num
    if (v != v) v = 0.0;
    else if (v == (double)INFINITY) v = DBL_MAX;
    else if (v == -(double)INFINITY) v = -DBL_MAX;
    if (v != 0.0) running_mean(avg, cnt, v);
  }
  if (sub && x % sub_step == 0 && y % sub_step == 0) sub[(long)(y / sub_step) * sub_pitch + x / sub_step] = avg;
  if (clip01) avg = avg < 0.0 ? 0.0 : (avg > 1.0 ? 1.0 : avg);   // np.clip(., 0, 1): NaN stays
  ff[(long)y * ff_pitch + x] = avg;
  count[(long)y * count_pitch + x] = cnt;
}

// ---- (c) one MaskedMovingAverage.update(data, mask) in place
template <typename E>
__global__ void __launch_bounds__(kOvsThreads)
masked_running_mean_kernel(double* __restrict__ avg, long avg_pitch, int* __restrict__ cnt, long cnt_pitch,
                           const E* __restrict__ data, long data_pitch, const unsigned char* __restrict__ mask,
                           long mask_pitch, int h, int w, int tiles_x) {
  int x, y;
  if (!tile_px(tiles_x, h, w, x, y)) return;
  if (mask && !mask[(long)y * mask_pitch + x]) return;
  double a = avg[(long)y * avg_pitch + x];
  int n = cnt[(long)y * cnt_pitch + x];
  running_mean(a, n, (double)data[(long)y * data_pitch + x]);
  avg[(long)y * avg_pitch + x] = a;
  cnt[(long)y * cnt_pitch + x] = n;
}

// what the two steps check alike: frame count, the stack of fits, the matrices -> the device table
int ovs_common(ipa_ctx* ctx, const char* what, const void* d_fits, int dtype, int n, int oh, int ow, long fit_pitch,
               long fit_frame_stride, const double* mats, Span* fits) {
  if (n > kOvsMaxN) IPA_UNSUPPORTED(ctx, "%s: at most %d fitted images (got %d)", what, kOvsMaxN, n);
  IPA_REQUIRE(ctx, n >= 1, "%s: needs at least one fitted image (got %d)", what, n);
  IPA_REQUIRE(ctx, d_fits && mats, "%s: null pointer", what);
  IPA_REQUIRE(ctx, oh > 0 && ow > 0, "%s: empty image", what);
  IPA_REQUIRE(ctx, fit_pitch >= ow, "%s: pitch smaller than width", what);
  IPA_REQUIRE(ctx, fit_frame_stride >= (long)(oh - 1) * fit_pitch + ow, "%s: frames overlap", what);
  if (!known_dtype(dtype))
    IPA_UNSUPPORTED(ctx, "%s: fitted images are uint8 / uint16 / float32 / float64 (got dtype %d)", what, dtype);
  *fits = span_stack(d_fits, n, oh, ow, fit_pitch, fit_frame_stride, ipa_dtype_size(dtype));
  return IPA_OK;
}

}  // namespace
}  // namespace ipa

using namespace ipa;

extern "C" {

int ipa_ovs_object_dev(ipa_ctx* ctx, const double* d_ff, int fh, int fw, long ff_pitch, const void* d_fits, int dtype,
                       int n, int oh, int ow, long fit_pitch, long fit_frame_stride, const double* mats,
                       double* d_obj, long obj_pitch, int* d_count, long count_pitch) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  Span fits;
  int rc = ovs_common(ctx, "ovs_object", d_fits, dtype, n, oh, ow, fit_pitch, fit_frame_stride, mats, &fits);
  if (rc != IPA_OK) return rc;
  IPA_REQUIRE(ctx, d_ff && d_obj && d_count, "ovs_object: null pointer");
  IPA_REQUIRE(ctx, fh > 0 && fw > 0, "ovs_object: empty flat field");
  IPA_REQUIRE(ctx, ff_pitch >= fw && obj_pitch >= ow && count_pitch >= ow, "ovs_object: pitch smaller than width");
  // the sampler addresses the flat field with 32-bit byte offsets
  IPA_REQUIRE(ctx, (long)(fh - 1) * ff_pitch + fw < (1L << 28), "ovs_object: flat field too large");
  const Span ff = span2d(d_ff, fh, fw, ff_pitch, 8);
  const Span spans[] = {span2d(d_obj, oh, ow, obj_pitch, 8), span2d(d_count, oh, ow, count_pitch, 4), ff, fits};
  IPA_REQUIRE(ctx, !written_overlaps(spans, 2), "ovs_object: an output overlaps another array");
  int tiles_x;
  unsigned grid;
  rc = frame_args(ctx, "ovs_object", oh, ow, &tiles_x, &grid);
  if (rc != IPA_OK) return rc;
  void* d_mats;
  rc = ipa_tab_upload(ctx, mats, (size_t)n * 9 * sizeof(double), &d_mats);
  if (rc != IPA_OK) return rc;
  return by_dtype(dtype, [&](auto e) {
    using E = decltype(e);
    return launch(ctx, ovs_object_kernel<E>, dim3(grid), dim3(kOvsThreads), 0, d_ff, fh, fw, (int)ff_pitch,
                  (unsigned)ff.bytes, d_fits, fit_pitch, fit_frame_stride, d_mats, n, oh, ow, tiles_x, d_obj, obj_pitch,
                  d_count, count_pitch);
  });
}

int ipa_ovs_flatfield_dev(ipa_ctx* ctx, const double* d_obj, long obj_pitch, const void* d_fits, int dtype, int n,
                          int oh, int ow, long fit_pitch, long fit_frame_stride, const unsigned char* d_masks,
                          long mask_pitch, long mask_frame_stride, const double* mats, double* d_ff, int fh, int fw,
                          long ff_pitch, int* d_count, long count_pitch, int clip01, double* d_sub, int sub_step,
                          long sub_pitch) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  Span fits;
  int rc = ovs_common(ctx, "ovs_flatfield", d_fits, dtype, n, oh, ow, fit_pitch, fit_frame_stride, mats, &fits);
  if (rc != IPA_OK) return rc;
  IPA_REQUIRE(ctx, d_obj && d_masks && d_ff && d_count, "ovs_flatfield: null pointer");
  IPA_REQUIRE(ctx, fh > 0 && fw > 0, "ovs_flatfield: empty flat field");
  IPA_REQUIRE(ctx, obj_pitch >= ow && mask_pitch >= ow && ff_pitch >= fw && count_pitch >= fw,
              "ovs_flatfield: pitch smaller than width");
  IPA_REQUIRE(ctx, mask_frame_stride >= (long)(oh - 1) * mask_pitch + ow, "ovs_flatfield: mask frames overlap");
  const int sh = d_sub && sub_step > 0 ? (fh + sub_step - 1) / sub_step : 0;
  const int sw = d_sub && sub_step > 0 ? (fw + sub_step - 1) / sub_step : 0;
  IPA_REQUIRE(ctx, !d_sub || (sub_step >= 1 && sub_pitch >= sw), "ovs_flatfield: bad every-n-th grid");
  const Span spans[] = {span2d(d_ff, fh, fw, ff_pitch, 8),
                        span2d(d_count, fh, fw, count_pitch, 4),
                        span2d(d_sub, sh, sw, sub_pitch, 8),
                        span2d(d_obj, oh, ow, obj_pitch, 8),
                        fits,
                        span_stack(d_masks, n, oh, ow, mask_pitch, mask_frame_stride, 1)};
  IPA_REQUIRE(ctx, !written_overlaps(spans, 3), "ovs_flatfield: an output overlaps another array");
  int tiles_x;
  unsigned grid;
  rc = frame_args(ctx, "ovs_flatfield", fh, fw, &tiles_x, &grid);
  if (rc != IPA_OK) return rc;
  void* d_mats;
  rc = ipa_tab_upload(ctx, mats, (size_t)n * 9 * sizeof(double), &d_mats);
  if (rc != IPA_OK) return rc;
  return by_dtype(dtype, [&](auto e) {
    using E = decltype(e);
    return launch(ctx, ovs_flatfield_kernel<E>, dim3(grid), dim3(kOvsThreads), 0, d_obj, obj_pitch, d_fits, fit_pitch,
                  fit_frame_stride, d_masks, mask_pitch, mask_frame_stride, d_mats, n, oh, ow, fh, fw, tiles_x, d_ff,
                  ff_pitch, d_count, count_pitch, clip01, d_sub, d_sub ? sub_step : 1, sub_pitch);
  });
}

int ipa_masked_running_mean_dev(ipa_ctx* ctx, double* d_avg, long avg_pitch, int* d_n, long n_pitch, const void* d_data,
                                int dtype, long data_pitch, const unsigned char* d_mask, long mask_pitch, int h,
                                int w) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  IPA_REQUIRE(ctx, d_avg && d_n && d_data, "masked_running_mean: null pointer");
  int tiles_x;
  unsigned grid;
  const int rc = frame_args(ctx, "masked_running_mean", h, w, &tiles_x, &grid);
  if (rc != IPA_OK) return rc;
  IPA_REQUIRE(ctx, avg_pitch >= w && n_pitch >= w && data_pitch >= w && (!d_mask || mask_pitch >= w),
              "masked_running_mean: pitch smaller than width");
  if (!known_dtype(dtype))
    IPA_UNSUPPORTED(ctx, "masked_running_mean: data is uint8 / uint16 / float32 / float64 (got dtype %d)", dtype);
  const Span spans[] = {span2d(d_avg, h, w, avg_pitch, 8), span2d(d_n, h, w, n_pitch, 4),
                        span2d(d_data, h, w, data_pitch, ipa_dtype_size(dtype)), span2d(d_mask, h, w, mask_pitch, 1)};
  IPA_REQUIRE(ctx, !written_overlaps(spans, 2), "masked_running_mean: the state overlaps another array");
  return by_dtype(dtype, [&](auto e) {
    using E = decltype(e);
    return launch(ctx, masked_running_mean_kernel<E>, dim3(grid), dim3(kOvsThreads), 0, d_avg, avg_pitch, d_n, n_pitch,
                  d_data, data_pitch, d_mask, mask_pitch, h, w, tiles_x);
  });
}

}  // extern "C"
