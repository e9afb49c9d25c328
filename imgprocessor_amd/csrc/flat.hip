// flat.hip — flat field calibration on gfx950: the frame passes of camera/flatField/
// flatFieldFromCloseDistance.py ("Method A" of Bedrich et al. 2017) and camera/flatField/sensitivity.py
// between the pieces ste.hip, nlf.hip, dark.hip and resize.hip already hold.
//   ipa_stack_mean_dev        transform/imgAverage.py:14-21
//   ipa_luma_dev              transformations.py:126-135 (toGray)
//   ipa_strided_extremum_dev  flatFieldFromCloseDistance.py:36, :91 (median_filter(img[::10, ::10], 3).max())
//                             and :62 (the minimum under the sort key)
//   ipa_flat_scale_dev        flatFieldFromCloseDistance.py:34-37, :96 (img -= bg; img /= mx)
//   ipa_nlf_lower_mask_dev    flatFieldFromCloseDistance.py:80-81 (i > noSTE - nlf(noSTE) * nstd)
//   ipa_sens_shrink_dev       sensitivity.py:21-23 (median_filter(i - bg, 3), INTER_AREA half of fastMean)
//   ipa_sens_accumulate_dev   sensitivity.py:23-29 (INTER_LINEAR half of fastMean, i / smooth, the mean)
//
// Everything is float64, every operation correctly rounded and unfused (Makefile + pragma), so the
// results equal numpy's bits; the two resizes follow resize.hip operation by operation.  The
// streaming kernels run one pixel per lane on 64 x 4 tiles, the stack mean 4 (uint8, uint16) or 2
// (float32) adjacent pixels per lane where rows, frames and the result are aligned for it.  The
// extremum goes through per-workgroup partials and a last workgroup - no float atomics.  The
// fused shrink keeps the medians of one row of destination blocks in LDS and writes only the small
// image: the float64 median frame never reaches memory.
#include "common.hpp"
#include "frame_args.hpp"
#include "interp_paths.hpp"
#include "launch.hpp"
#include "nlf_fn.hpp"
#include "reduce.hpp"

#pragma clang fp contract(off)

namespace ipa {
namespace {

constexpr int kFlatThreads = 256;    // a 64 x 4 tile
constexpr int kShrinkLds = 49152;    // medians of one workgroup of sens_shrink_kernel
constexpr int kShrinkMaxDst = 32;    // destination pixels per workgroup
constexpr int kExtMaxGrid = 4096;    // partial extrema

template <typename T> constexpr int kMeanPx = sizeof(T) <= 2 ? 4 : sizeof(T) == 4 ? 2 : 1;

// out = (f0 + f1 + ... in frame order) / n: numpy's `out = float(f0); out += f; out /= n`
template <typename T, int PX>
__global__ void __launch_bounds__(kFlatThreads)
stack_mean_kernel(const T* __restrict__ stack, long pitch, long frame_stride, int n, int h, int w, int tiles_x,
                  double* __restrict__ out, long out_pitch) {
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x0 = (tx * 64 + (threadIdx.x & 63)) * PX, y = ty * 4 + (threadIdx.x >> 6);
  if (x0 >= w || y >= h) return;
  const int npx = min(PX, w - x0);   // < PX in the last lane of a row whose width is no multiple
  const T* px = stack + (long)y * pitch + x0;
  PxVec<double, PX> acc;
  auto load = [&](int k) {
    const T* p = px + (long)k * frame_stride;
    PxVec<T, PX> r;
    if (PX == 1 || npx == PX) {
      r = *(const PxVec<T, PX>*)p;
    } else {
#pragma unroll
      for (int j = 0; j < PX; j++) r.v[j] = j < npx ? p[j] : T(0);
    }
    return r;
  };
  {
    const PxVec<T, PX> r = load(0);
#pragma unroll
    for (int j = 0; j < PX; j++) acc.v[j] = (double)r.v[j];
  }
#pragma unroll 4
  for (int k = 1; k < n; k++) {
    const PxVec<T, PX> r = load(k);
#pragma unroll
    for (int j = 0; j < PX; j++) acc.v[j] += (double)r.v[j];
  }
  const double dn = (double)n;
#pragma unroll
  for (int j = 0; j < PX; j++) acc.v[j] = acc.v[j] / dn;
  double* o = out + (long)y * out_pitch + x0;
  if (PX == 1 || npx == PX) {
    *(PxVec<double, PX>*)o = acc;
  } else {
#pragma unroll
    for (int j = 0; j < PX; j++)
      if (j < npx) o[j] = acc.v[j];
  }
}

__global__ void __launch_bounds__(kFlatThreads)
luma_kernel(const double* __restrict__ img, int h, int w, long pitch, int tiles_x, double wr, double wg, double wb,
            double wsum, double* __restrict__ out, long out_pitch) {
  int x, y;
  if (!tile_px(tiles_x, h, w, x, y)) return;
  const double* p = img + (long)y * pitch + 3L * x;
  out[(long)y * out_pitch + x] = ((p[0] * wr + p[1] * wg) + p[2] * wb) / wsum;
}

// an extremum and how two of them merge: MODE 0 maximum, 1 minimum (numpy's: a NaN wins)
template <int MODE>
struct Ext {
  double v;
};
template <int MODE>
__device__ inline Ext<MODE> merge(Ext<MODE> a, Ext<MODE> b) {
  return {MODE == 0 ? np_max(a.v, b.v) : np_min(a.v, b.v)};
}

// The sampled grid a[::sy, ::sx] has gh x gw points.  MODE 0: a lane takes the 3 x 3 median of a
// grid point, the edge sample repeated (scipy's 'reflect'); MODE 1: the sample itself.  Workgroup b
// writes the extremum of its lanes' points b, b + gridDim, ... to part[b].
template <typename T, int MODE>
__global__ void __launch_bounds__(kFlatThreads)
strided_extremum_kernel(const T* __restrict__ img, long pitch, int gh, int gw, int sy, int sx,
                        double* __restrict__ part) {
  __shared__ Ext<MODE> lds[kFlatThreads];
  const long n = (long)gh * gw;
  Ext<MODE> m = {MODE == 0 ? -__builtin_inf() : __builtin_inf()};
  for (long i = (long)blockIdx.x * kFlatThreads + threadIdx.x; i < n; i += (long)gridDim.x * kFlatThreads) {
    const int gy = (int)(i / gw), gx = (int)(i - (long)gy * gw);
    double v;
    if (MODE == 0) {
      double c[3][3];   // [column][row]
#pragma unroll
      for (int a = 0; a < 3; a++) {
        const int xx = min(max(gx + a - 1, 0), gw - 1);
#pragma unroll
        for (int b = 0; b < 3; b++) {
          const int yy = min(max(gy + b - 1, 0), gh - 1);
          c[a][b] = (double)img[(long)yy * sy * pitch + (long)xx * sx];
        }
      }
      v = median9(c);
    } else {
      v = (double)img[(long)gy * sy * pitch + (long)gx * sx];
    }
    m = merge(m, Ext<MODE>{v});
  }
  m = block_merge<kFlatThreads>(m, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = m.v;
}

// one workgroup: the partials in workgroup order -> res[0]
template <int MODE>
__global__ void __launch_bounds__(kFlatThreads)
extremum_final_kernel(const double* __restrict__ part, int n_part, double* __restrict__ res) {
  __shared__ Ext<MODE> lds[kFlatThreads];
  const Ext<MODE> none = {MODE == 0 ? -__builtin_inf() : __builtin_inf()};
  const Ext<MODE> m = merge_partials<kFlatThreads>((const Ext<MODE>*)part, n_part, none, lds);   // one double each
  if (threadIdx.x == 0) res[0] = m.v;
}

__global__ void __launch_bounds__(kFlatThreads)
flat_scale_kernel(const double* img, int h, int w, long pitch, int tiles_x, const double* __restrict__ bg,
                  long bg_pitch, double bg_value, int subtract, double div, int divide, double* out,
                  long out_pitch) {
  int x, y;
  if (!tile_px(tiles_x, h, w, x, y)) return;
  double v = img[(long)y * pitch + x];
  if (subtract) v = v - (bg ? bg[(long)y * bg_pitch + x] : bg_value);
  if (divide) v = v / div;
  out[(long)y * out_pitch + x] = v;
}

template <typename T>
__global__ void __launch_bounds__(kFlatThreads)
nlf_lower_mask_kernel(const T* __restrict__ img, int h, int w, long pitch, int tiles_x,
                      const double* __restrict__ avg, long avg_pitch, NlfParams f, double nstd,
                      unsigned char* __restrict__ mask, long mask_pitch) {
  int x, y;
  if (!tile_px(tiles_x, h, w, x, y)) return;
  const double a = avg[(long)y * avg_pitch + x];
  const double thr = a - nlf_eval(f, a) * nstd;
  mask[(long)y * mask_pitch + x] = (double)img[(long)y * pitch + x] > thr ? 1 : 0;
}

// a frame as the reference sees it after `i = float(frame); i -= bg`
struct SensSrc {
  const void* img;
  const double* bg;   // NULL: bg_value
  long pitch, bg_pitch;
  double bg_value;
};
template <typename T>
__device__ inline double sens_px(const SensSrc& s, int y, int x) {
  const double v = (double)((const T*)s.img)[(long)y * s.pitch + x];
  return v - (s.bg ? s.bg[(long)y * s.bg_pitch + x] : s.bg_value);
}

// median9 of nlf_fn.hpp on the frame's own values: subtracting one number is monotone, so with a
// scalar background the median of `frame - bg` is the median of the frame, minus bg, to the bit -
// and the 19 exchanges run on integers or float32 instead of float64.  numpy's NaN rule as there.
template <typename V> __device__ inline V raw_min(V a, V b) { return (a < b || a != a) ? a : b; }
template <typename V> __device__ inline V raw_max(V a, V b) { return (a > b || a != a) ? a : b; }
template <typename V> __device__ inline V raw_med3(V a, V b, V c) {
  return raw_max(raw_min(a, b), raw_min(raw_max(a, b), c));
}
template <typename V>
__device__ inline V raw_median9(V (&c)[3][3]) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
    V lo = raw_min(c[i][0], c[i][1]), hi = raw_max(c[i][0], c[i][1]);
    c[i][0] = lo;
    c[i][1] = raw_min(hi, c[i][2]);
    c[i][2] = raw_max(hi, c[i][2]);
    lo = raw_min(c[i][0], c[i][1]);
    c[i][1] = raw_max(c[i][0], c[i][1]);
    c[i][0] = lo;
  }
  const V lo = raw_max(raw_max(c[0][0], c[1][0]), c[2][0]);
  const V mid = raw_med3(c[0][1], c[1][1], c[2][1]);
  const V hi = raw_min(raw_min(c[0][2], c[1][2]), c[2][2]);
  return raw_med3(lo, mid, hi);
}

// h = isy * dh, w = isx * dw.  A workgroup owns `dpb` adjacent destination pixels of one row of the
// small image: the isy x (dpb * isx) source pixels under them.  First every lane takes the 3 x 3
// median (the edge pixel repeated) of some of those pixels into LDS - each source pixel's median
// is computed once -, then lane d adds up block d in area_fast_kernel's order.
template <typename T>
__global__ void __launch_bounds__(kFlatThreads)
sens_shrink_kernel(SensSrc s, int h, int w, int isx, int isy, int dpb, int dw, double* __restrict__ small,
                   long small_pitch) {
  extern __shared__ double med[];
  const int dy = blockIdx.y, d0 = blockIdx.x * dpb;
  const int nd = min(dpb, dw - d0);
  const int tw = nd * isx, x0 = d0 * isx, y0 = dy * isy;
  for (int i = threadIdx.x; i < isy * tw; i += kFlatThreads) {
    const int r = i / tw, cx = i - r * tw;
    const int x = x0 + cx, y = y0 + r;
    if (s.bg) {
      double c[3][3];   // [column][row]
#pragma unroll
      for (int a = 0; a < 3; a++) {
        const int xx = min(max(x + a - 1, 0), w - 1);
#pragma unroll
        for (int b = 0; b < 3; b++) c[a][b] = sens_px<T>(s, min(max(y + b - 1, 0), h - 1), xx);
      }
      med[i] = median9(c);
    } else {
      T c[3][3];
#pragma unroll
      for (int a = 0; a < 3; a++) {
        const int xx = min(max(x + a - 1, 0), w - 1);
#pragma unroll
        for (int b = 0; b < 3; b++)
          c[a][b] = ((const T*)s.img)[(long)min(max(y + b - 1, 0), h - 1) * s.pitch + xx];
      }
      med[i] = (double)raw_median9(c) - s.bg_value;
    }
  }
  __syncthreads();
  const int d = threadIdx.x;
  if (d >= nd) return;
  const float fscale = 1.f / (float)(isx * isy);
  const int area = isx * isy;
  auto px = [&](int e) { return med[(e / isx) * tw + d * isx + e % isx]; };
  double sum = 0;
  int k = 0;
  for (; k <= area - 4; k += 4) {
    const double a = px(k), b = px(k + 1), c = px(k + 2), e = px(k + 3);
    sum += a + b + c + e;
  }
  for (; k < area; k++) sum += px(k);
  small[(long)dy * small_pitch + d0 + d] = (double)(sum * fscale);
}

struct AccArgs {
  SensSrc src;
  int h, w, tiles_x;
  const double* small;
  long small_pitch;
  int sh;   // rows of `small`
  ipa_resize_tabs tab;
  double* acc;
  long acc_pitch;
  int first, n_last;
};

// up(small) at (x, y) as hresize_kernel<double, 2> and vresize_kernel<double, 2> compute it through
// their intermediate: the horizontal blend of the two source rows, each rounded, then the vertical
template <typename T>
__global__ void __launch_bounds__(kFlatThreads)
sens_accumulate_kernel(AccArgs a) {
  int x, y;
  if (!tile_px(a.tiles_x, a.h, a.w, x, y)) return;
  const int sx = a.tab.xofs[x], sy0 = a.tab.yofs[y];
  const float a0 = a.tab.alpha[2L * x], a1 = a.tab.alpha[2L * x + 1];
  const float b0 = a.tab.beta[2L * y], b1 = a.tab.beta[2L * y + 1];
  double up = 0;
#pragma unroll
  for (int k = 0; k < 2; k++) {
    int sy = sy0 + k;
    sy = sy >= 0 ? (sy < a.sh ? sy : a.sh - 1) : 0;
    const double* S = a.small + (long)sy * a.small_pitch;
    double v;
    if (x >= a.tab.xmax) v = S[sx] * 1.0;
    else v = S[sx] * (double)a0 + S[sx + 1] * (double)a1;
    const double t = v * (double)(k == 0 ? b0 : b1);
    up = k == 0 ? t : up + t;
  }
  const double q = sens_px<T>(a.src, y, x) / up;
  double* o = a.acc + (long)y * a.acc_pitch + x;
  double r = a.first ? q : *o + q;
  if (a.n_last > 0) r = r / (double)a.n_last;
  *o = r;
}

// the frame, its dtype and its background of the two sensitivity calls
int sens_args(ipa_ctx* ctx, const char* what, const void* d_img, int dtype, int h, int w, long pitch,
              const double* d_bg, long bg_pitch, int dh, int dw) {
  IPA_REQUIRE(ctx, d_img, "%s: null image", what);
  IPA_REQUIRE(ctx, h > 0 && w > 0 && h <= 65535, "%s: empty image or more than 65535 rows", what);
  IPA_REQUIRE(ctx, pitch >= w && (!d_bg || bg_pitch >= w), "%s: pitch smaller than width", what);
  IPA_REQUIRE(ctx, dh > 0 && dw > 0, "%s: the small image is empty (%d x %d)", what, dh, dw);
  if (!known_dtype(dtype))
    IPA_UNSUPPORTED(ctx, "%s: frames are uint8 / uint16 / float32 / float64 (got dtype %d)", what, dtype);
  if (dh > h || dw > w) IPA_UNSUPPORTED(ctx, "%s: the small image is larger than the frame", what);
  return IPA_OK;
}

}  // namespace
}  // namespace ipa

using namespace ipa;

extern "C" {

int ipa_stack_mean_dev(ipa_ctx* ctx, const void* d_stack, int dtype, int n, int h, int w, long pitch,
                       long frame_stride, double* d_out, long out_pitch) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  IPA_REQUIRE(ctx, d_stack && d_out, "stack_mean: null pointer");
  IPA_REQUIRE(ctx, n >= 1, "stack_mean: no frames");
  int tiles_x;
  unsigned grid;
  int rc = frame_args(ctx, "stack_mean", h, w, &tiles_x, &grid);
  if (rc) return rc;
  IPA_REQUIRE(ctx, pitch >= w && out_pitch >= w, "stack_mean: pitch smaller than width");
  IPA_REQUIRE(ctx, n == 1 || frame_stride >= (long)(h - 1) * pitch + w, "stack_mean: frames overlap");
  if (!known_dtype(dtype))
    IPA_UNSUPPORTED(ctx, "stack_mean: frames are uint8 / uint16 / float32 / float64 (got dtype %d)", dtype);
  const size_t es = ipa_dtype_size(dtype);
  const Span st = span_stack(d_stack, n, h, w, pitch, frame_stride, es);
  IPA_REQUIRE(ctx, !overlap(st, span2d(d_out, h, w, out_pitch, 8)), "stack_mean does not run in place");
  return by_dtype(dtype, [&](auto e) {
    using E = decltype(e);
    constexpr int P = kMeanPx<E>;
    if constexpr (P > 1) {
      const size_t in = sizeof(E) * P, out = 8 * (size_t)P;
      if ((uintptr_t)d_stack % in == 0 && (pitch * sizeof(E)) % in == 0 && (frame_stride * sizeof(E)) % in == 0 &&
          (uintptr_t)d_out % out == 0 && out_pitch % P == 0) {
        const int tx = (w + 64 * P - 1) / (64 * P);
        return launch(ctx, stack_mean_kernel<E, P>, dim3((unsigned)tx * ((h + 3) / 4)), dim3(kFlatThreads), 0,
                      d_stack, pitch, frame_stride, n, h, w, tx, d_out, out_pitch);
      }
    }
    return launch(ctx, stack_mean_kernel<E, 1>, dim3(grid), dim3(kFlatThreads), 0, d_stack, pitch, frame_stride, n,
                  h, w, tiles_x, d_out, out_pitch);
  });
}

int ipa_luma_dev(ipa_ctx* ctx, const double* d_img, int h, int w, long pitch, const double* wgt, double wsum,
                 double* d_out, long out_pitch) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  IPA_REQUIRE(ctx, d_img && d_out && wgt, "luma: null pointer");
  int tiles_x;
  unsigned grid;
  int rc = frame_args(ctx, "luma", h, w, &tiles_x, &grid);
  if (rc) return rc;
  IPA_REQUIRE(ctx, pitch >= 3L * w && out_pitch >= w, "luma: pitch smaller than the row");
  IPA_REQUIRE(ctx, !overlap(span2d(d_img, h, 3L * w, pitch, 8), span2d(d_out, h, w, out_pitch, 8)),
              "luma does not run in place");
  return launch(ctx, luma_kernel, dim3(grid), dim3(kFlatThreads), 0, d_img, h, w, pitch, tiles_x, wgt[0], wgt[1],
                wgt[2], wsum, d_out, out_pitch);
}

int ipa_strided_extremum_dev(ipa_ctx* ctx, const void* d_img, int dtype, int h, int w, long pitch, int step_y,
                             int step_x, int mode, double* result) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  IPA_REQUIRE(ctx, d_img && result, "strided_extremum: null pointer");
  IPA_REQUIRE(ctx, h > 0 && w > 0 && pitch >= w, "strided_extremum: empty image or pitch smaller than width");
  IPA_REQUIRE(ctx, step_y >= 1 && step_x >= 1, "strided_extremum: steps must be at least 1 (got %d, %d)", step_y,
              step_x);
  IPA_REQUIRE(ctx, mode == IPA_EXTREMUM_MEDIAN_MAX || mode == IPA_EXTREMUM_MIN, "strided_extremum: unknown mode %d",
              mode);
  if (!known_dtype(dtype) || (mode == IPA_EXTREMUM_MEDIAN_MAX && dtype != IPA_F64))
    IPA_UNSUPPORTED(ctx, "strided_extremum: the median's maximum takes float64 frames, the minimum uint8 / uint16 / "
                         "float32 / float64 (got dtype %d)", dtype);
  const int gh = (h + step_y - 1) / step_y, gw = (w + step_x - 1) / step_x;
  const long blocks = ((long)gh * gw + kFlatThreads - 1) / kFlatThreads;
  const int grid = (int)(blocks < kExtMaxGrid ? blocks : kExtMaxGrid);
  double *part, *res;
  int rc = stage_ws(ctx, slot(&part, grid), slot(&res, 1));
  if (rc) return rc;
  if (mode == IPA_EXTREMUM_MEDIAN_MAX) {
    rc = launch(ctx, strided_extremum_kernel<double, 0>, dim3(grid), dim3(kFlatThreads), 0, d_img, pitch, gh, gw,
                step_y, step_x, part);
    if (!rc) rc = launch(ctx, extremum_final_kernel<0>, dim3(1), dim3(kFlatThreads), 0, part, grid, res);
  } else {
    rc = by_dtype(dtype, [&](auto e) {
      return launch(ctx, strided_extremum_kernel<decltype(e), 1>, dim3(grid), dim3(kFlatThreads), 0, d_img, pitch,
                    gh, gw, step_y, step_x, part);
    });
    if (!rc) rc = launch(ctx, extremum_final_kernel<1>, dim3(1), dim3(kFlatThreads), 0, part, grid, res);
  }
  if (rc) return rc;
  return ipa_stage_out(ctx, {{result, res, sizeof(double)}});
}

int ipa_flat_scale_dev(ipa_ctx* ctx, const double* d_img, int h, int w, long pitch, const double* d_bg,
                       long bg_pitch, double bg_value, int subtract, double div, int divide, double* d_out,
                       long out_pitch) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  IPA_REQUIRE(ctx, d_img && d_out, "flat_scale: null pointer");
  int tiles_x;
  unsigned grid;
  int rc = frame_args(ctx, "flat_scale", h, w, &tiles_x, &grid);
  if (rc) return rc;
  IPA_REQUIRE(ctx, pitch >= w && out_pitch >= w && (!d_bg || bg_pitch >= w), "flat_scale: pitch smaller than width");
  // in place is fine - a lane reads its pixel before it writes it -, a partial overlap is not
  const Span out = span2d(d_out, h, w, out_pitch, 8);
  const bool same = d_img == d_out && pitch == out_pitch;
  IPA_REQUIRE(ctx, same || !overlap(span2d(d_img, h, w, pitch, 8), out),
              "flat_scale: image and result overlap without being the same array");
  IPA_REQUIRE(ctx, !overlap(span2d(d_bg, h, w, bg_pitch, 8), out), "flat_scale: the result overlaps the background");
  return launch(ctx, flat_scale_kernel, dim3(grid), dim3(kFlatThreads), 0, d_img, h, w, pitch, tiles_x, d_bg, bg_pitch,
                bg_value, subtract, div, divide, d_out, out_pitch);
}

int ipa_nlf_lower_mask_dev(ipa_ctx* ctx, const void* d_img, int dtype, int h, int w, long pitch,
                           const double* d_avg, long avg_pitch, int kind, const double* params, double nstd,
                           unsigned char* d_mask, long mask_pitch) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  IPA_REQUIRE(ctx, d_img && d_avg && d_mask && params, "nlf_lower_mask: null pointer");
  int tiles_x;
  unsigned grid;
  int rc = frame_args(ctx, "nlf_lower_mask", h, w, &tiles_x, &grid);
  if (rc) return rc;
  IPA_REQUIRE(ctx, pitch >= w && avg_pitch >= w && mask_pitch >= w, "nlf_lower_mask: pitch smaller than width");
  const int n_params = nlf_param_count(kind);
  IPA_REQUIRE(ctx, n_params, "nlf_lower_mask: unknown kind %d", kind);
  if (!known_dtype(dtype))
    IPA_UNSUPPORTED(ctx, "nlf_lower_mask: frames are uint8 / uint16 / float32 / float64 (got dtype %d)", dtype);
  const Span m = span2d(d_mask, h, w, mask_pitch, 1);
  IPA_REQUIRE(ctx, !overlap(m, span2d(d_img, h, w, pitch, ipa_dtype_size(dtype))) &&
                       !overlap(m, span2d(d_avg, h, w, avg_pitch, 8)),
              "nlf_lower_mask does not run in place");
  NlfParams f;
  f.kind = kind;
  for (int i = 0; i < 5; i++) f.p[i] = i < n_params ? params[i] : 0.0;
  return by_dtype(dtype, [&](auto e) {
    return launch(ctx, nlf_lower_mask_kernel<decltype(e)>, dim3(grid), dim3(kFlatThreads), 0, d_img, h, w, pitch,
                  tiles_x, d_avg, avg_pitch, f, nstd, d_mask, mask_pitch);
  });
}

int ipa_sens_shrink_dev(ipa_ctx* ctx, const void* d_img, int dtype, int h, int w, long pitch,
                        const double* d_bg, long bg_pitch, double bg_value, int dh, int dw, double* d_small,
                        long small_pitch) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  int rc = sens_args(ctx, "sens_shrink", d_img, dtype, h, w, pitch, d_bg, bg_pitch, dh, dw);
  if (rc) return rc;
  IPA_REQUIRE(ctx, d_small && small_pitch >= dw, "sens_shrink: null small image or pitch smaller than its width");
  const Span sm = span2d(d_small, dh, dw, small_pitch, 8);
  IPA_REQUIRE(ctx, !overlap(sm, span2d(d_img, h, w, pitch, ipa_dtype_size(dtype))) &&
                       !overlap(sm, span2d(d_bg, h, w, bg_pitch, 8)),
              "sens_shrink does not run in place");
  int isx = 0, isy = 0;
  const int area = resize_area_path(resize_scale(w, dw), resize_scale(h, dh), &isx, &isy);
  const long block = (long)isx * isy;
  if (area == 1 && (long)isx * dw == w && (long)isy * dh == h && block * 8 <= kShrinkLds) {
    const long fit = kShrinkLds / (block * 8);
    const int dpb = (int)(fit < kShrinkMaxDst ? fit : kShrinkMaxDst);
    const SensSrc src = {d_img, d_bg, pitch, bg_pitch, bg_value};
    const dim3 grid((unsigned)((dw + dpb - 1) / dpb), (unsigned)dh);
    return by_dtype(dtype, [&](auto e) {
      return launch(ctx, sens_shrink_kernel<decltype(e)>, grid, dim3(kFlatThreads), (size_t)block * dpb * 8, src, h,
                    w, isx, isy, dpb, dw, d_small, small_pitch);
    });
  }
  // the median frame through the workspace, then resize.hip's INTER_AREA
  rc = ipa_ws_reserve(ctx, (size_t)h * w * 8);
  if (rc) return rc;
  double* med = (double*)ctx->ws;
  rc = ipa_nlf_signal_dev(ctx, d_img, dtype, nullptr, h, w, pitch, 0, d_bg, bg_pitch, bg_value, med, w);
  if (rc) return rc;
  return ipa_resize_dev(ctx, med, IPA_F64, h, w, w, d_small, dh, dw, small_pitch, IPA_RESIZE_AREA);
}

int ipa_sens_accumulate_dev(ipa_ctx* ctx, const void* d_img, int dtype, int h, int w, long pitch,
                            const double* d_bg, long bg_pitch, double bg_value, const double* d_small, int dh,
                            int dw, long small_pitch, double* d_acc, long acc_pitch, int first, int n_last) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  int rc = sens_args(ctx, "sens_accumulate", d_img, dtype, h, w, pitch, d_bg, bg_pitch, dh, dw);
  if (rc) return rc;
  IPA_REQUIRE(ctx, d_small && small_pitch >= dw && d_acc && acc_pitch >= w,
              "sens_accumulate: null pointer or pitch smaller than width");
  IPA_REQUIRE(ctx, n_last >= 0, "sens_accumulate: negative frame count");
  const Span acc = span2d(d_acc, h, w, acc_pitch, 8);
  IPA_REQUIRE(ctx, !overlap(acc, span2d(d_img, h, w, pitch, ipa_dtype_size(dtype))) &&
                       !overlap(acc, span2d(d_bg, h, w, bg_pitch, 8)) &&
                       !overlap(acc, span2d(d_small, dh, dw, small_pitch, 8)),
              "sens_accumulate: the accumulator overlaps an input");
  AccArgs a;
  unsigned grid;
  rc = frame_args(ctx, "sens_accumulate", h, w, &a.tiles_x, &grid);
  if (rc) return rc;
  // small -> frame: dw x dh is the SOURCE of this resize
  rc = ipa_resize_tables(ctx, dh, dw, h, w, IPA_RESIZE_LINEAR, 2, &a.tab);
  if (rc) return rc;
  a.src = {d_img, d_bg, pitch, bg_pitch, bg_value};
  a.h = h;
  a.w = w;
  a.small = d_small;
  a.small_pitch = small_pitch;
  a.sh = dh;
  a.acc = d_acc;
  a.acc_pitch = acc_pitch;
  a.first = first;
  a.n_last = n_last;
  return by_dtype(dtype, [&](auto e) {
    return launch(ctx, sens_accumulate_kernel<decltype(e)>, dim3(grid), dim3(kFlatThreads), 0, a);
  });
}

}  // extern "C"
