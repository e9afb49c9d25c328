// poly.hip — 2-D polynomial fits of masked frames on gfx950: what interpolate/polyfit2d.py
// (polyfit2dGrid) and camera/flatField/postprocessing/polynomial.py ("POLY repair") do per pixel.
//   ipa_poly2d_moments_dev  polyfit2d.py:13-18, 46-49  the sums of the least-squares fit over the valid pixels
//   ipa_poly2d_eval_dev     polyfit2d.py:22-28, 57-64  the fitted polynomial into the masked pixels / every
//                                                      pixel / an outgrid; polynomial.py:37 the residuum
//   ipa_high_grad_dev       polynomial.py:10-14        _highGrad: |laplace| > 0.01, dilated
//   ipa_clip01_dev          polynomial.py:49           np.clip(out, 0, 1, out=out)
//
// The reference fits raw pixel monomials x**i * y**j through np.linalg.lstsq on an (n_valid, (o+1)^2)
// design matrix.  This file fits products of Chebyshev polynomials T_j(v) T_i(u) on coordinates
// normalised to [-1, 1] - the same polynomial space, a basis that stays well conditioned -
//   u = (2 x - (w - 1)) / (w - 1),  v = (2 y - (h - 1)) / (h - 1),  0 for a dimension of size 1,
//   T_0 = 1, T_1 = u, T_k = (2 u) T_{k-1} - T_{k-2},
// and never forms the design matrix: because T_i T_k = (T_{i+k} + T_{|i-k|}) / 2 the Gram matrix follows
// on the host from M[b][a] = sum T_b(v) T_a(u), a, b <= 2 o; the right-hand side is R[j][i] =
// sum z T_j(v) T_i(u), i, j <= o.  Masked pixels are selected out, never multiplied by zero: a NaN
// under the mask is not read into a sum.
//
// moments.  A wave walks one row, its lanes stride along x with the 2 o + 1 column sums of T_a(u), the
// o + 1 of z T_i(u) and the count in registers; a butterfly over the wave adds them in a fixed order.
// After a barrier thread e of the workgroup owns entry e of {M, R, count} and folds the four rows of
// the workgroup into it through T_b(v), wave 0 first.  A workgroup takes rows 4 (g + k grid) .. + 3 for
// k = 0, 1, ..; its entries go to one slab, and a second launch adds the slabs in a fixed order.  No
// float atomics anywhere: the result of a call depends on its arguments and the grid alone.
//
// eval.  Everything in double, nothing fused (Makefile + pragma), one rounding into the frame's type:
//   Tu[0..o] of u and Tv[0..o] of v by the recurrence above (t2 = 2.0 * u; T_k = t2 * T_{k-1} - T_{k-2});
//   s_j = c[j][0];  for i = 1 .. o:  s_j = s_j + c[j][i] * Tu[i];
//   val = s_0;      for j = 1 .. o:  val = val + s_j * Tv[j];
// c[j][i] is the coefficient of T_j(v) T_i(u).  tests/poly_ref.py restates exactly this and equals it
// bit for bit.  The residuum is sum |(double)new - (double)old| over the replaced pixels with new
// already rounded to the frame's type: a tree over the 256 threads of a 64 x 4 tile, one partial per
// tile, the partials added by one workgroup (thread t takes t, t + 256, .., then the same tree).
//
// high gradients.  scipy.ndimage.laplace(mode='reflect') as correlate1d evaluates a symmetric kernel:
// per axis c * (-2) + (l + r) in double, rounded to the frame's type, axis 0 plus axis 1 in the frame's
// type; |.| > (frame type)0.01.  The maximum_filter of that boolean is a separable dilation; its
// reflecting border repeats pixels the clipped window holds already, so the window is clipped.
#include "common.hpp"
#include "frame_args.hpp"
#include "launch.hpp"
#include "reduce.hpp"

#pragma clang fp contract(off)

namespace ipa {
namespace {

constexpr int kPolyMaxOrder = 5;
constexpr int kPolyThreads = 256;
constexpr int kPolyWaves = kPolyThreads / 64;
constexpr int kPolyMaxGrid = 2048;
constexpr int kPolyAhead = 8;         // pixels a lane has in flight along its row
constexpr int kHighGradMaxSize = 31;

__host__ __device__ constexpr int poly_entries(int o) { return (2 * o + 1) * (2 * o + 1) + (o + 1) * (o + 1) + 1; }

// pixel position -> [-1, 1]; positions outside the frame extrapolate
__device__ __forceinline__ double poly_coord(double p, int n) {
  return n > 1 ? (2.0 * p - (double)(n - 1)) / (double)(n - 1) : 0.0;
}

// t[0 .. N] = T_0 .. T_N of u
template <int N>
__device__ __forceinline__ void cheb(double u, double (&t)[N + 1]) {
  t[0] = 1.0;
  if (N >= 1) t[1] = u;
  const double t2 = 2.0 * u;
#pragma unroll
  for (int k = 2; k <= N; k++) t[k] = t2 * t[k - 1] - t[k - 2];
}

__device__ inline double cheb_at(double u, int k) {
  double a = 1.0, b = u;
  if (k == 0) return a;
  const double t2 = 2.0 * u;
  for (int i = 2; i <= k; i++) {
    const double c = t2 * b - a;
    a = b;
    b = c;
  }
  return b;
}

// ---------------------------------------------------------------- moments
template <int O>
struct RowSums {
  double a[2 * O + 1];   // sum T_a(u)
  double b[O + 1];       // sum z T_i(u)
  double n;              // valid pixels (exact: an integer below 2^53)
  __device__ __forceinline__ void add(int x, int w, double z) {
    double t[2 * O + 1];
    cheb<2 * O>(poly_coord((double)x, w), t);
#pragma unroll
    for (int k = 0; k <= 2 * O; k++) a[k] += t[k];
#pragma unroll
    for (int k = 0; k <= O; k++) b[k] += z * t[k];
    n += 1.0;
  }
};

// slab[blockIdx.x][e]: e < NM^2 -> M[e / NM][e % NM], then R[.][.], then the count
template <typename E, int O>
__global__ void __launch_bounds__(kPolyThreads)
poly_moments_kernel(const E* __restrict__ img, long pitch, const unsigned char* __restrict__ mask, long mask_pitch,
                    int h, int w, int iters, double* __restrict__ slab) {
  constexpr int NM = 2 * O + 1, NR = O + 1, NROW = NM + NR + 1, NE = poly_entries(O);
  static_assert(NE <= kPolyThreads, "one thread per entry");
  __shared__ double rows[kPolyWaves][NROW];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  // the entry of this thread: its row sum and the order of its T(v)
  int col = 0, vb = -1;
  if (t < NM * NM) {
    vb = t / NM;
    col = t - vb * NM;
  } else if (t < NM * NM + NR * NR) {
    vb = (t - NM * NM) / NR;
    col = NM + (t - NM * NM) - vb * NR;
  } else if (t == NE - 1) {
    vb = 0;
    col = NM + NR;
  }
  double acc = 0.0;
  for (int it = 0; it < iters; it++) {
    const long row0 = ((long)it * gridDim.x + blockIdx.x) * kPolyWaves;
    const long row = row0 + wave;
    RowSums<O> s;
#pragma unroll
    for (int k = 0; k < NM; k++) s.a[k] = 0.0;
#pragma unroll
    for (int k = 0; k < NR; k++) s.b[k] = 0.0;
    s.n = 0.0;
    if (row < h) {
      const E* __restrict__ p = img + row * pitch;
      const unsigned char* __restrict__ m = mask ? mask + row * mask_pitch : nullptr;
      int x = lane;
      for (; x + (kPolyAhead - 1) * 64 < w; x += kPolyAhead * 64) {
        E z[kPolyAhead];
        unsigned char mk[kPolyAhead];
#pragma unroll
        for (int k = 0; k < kPolyAhead; k++) {
          z[k] = p[x + k * 64];
          mk[k] = m ? m[x + k * 64] : (unsigned char)0;
        }
#pragma unroll
        for (int k = 0; k < kPolyAhead; k++)
          if (!mk[k]) s.add(x + k * 64, w, (double)z[k]);
      }
      for (; x < w; x += 64)
        if (!m || !m[x]) s.add(x, w, (double)p[x]);
    }
    // butterfly: every lane ends with the same bits, partners add the same two values
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
#pragma unroll
      for (int k = 0; k < NM; k++) s.a[k] += __shfl_xor(s.a[k], d);
#pragma unroll
      for (int k = 0; k < NR; k++) s.b[k] += __shfl_xor(s.b[k], d);
      s.n += __shfl_xor(s.n, d);
    }
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < NM; k++) rows[wave][k] = s.a[k];
#pragma unroll
      for (int k = 0; k < NR; k++) rows[wave][NM + k] = s.b[k];
      rows[wave][NM + NR] = s.n;
    }
    __syncthreads();
    if (vb >= 0) {
      for (int wv = 0; wv < kPolyWaves; wv++) {
        if (row0 + wv >= h) break;
        acc += cheb_at(poly_coord((double)(row0 + wv), h), vb) * rows[wv][col];
      }
    }
    __syncthreads();
  }
  if (t < NE) slab[(long)blockIdx.x * NE + t] = acc;
}

// one workgroup per entry adds the slabs: thread t takes slabs t, t + 256, .., then the tree
__global__ void __launch_bounds__(kPolyThreads)
poly_sum_columns(const double* __restrict__ part, int n_part, int ne, double* __restrict__ out) {
  __shared__ double lds[kPolyThreads];
  const double s = merge_partials<kPolyThreads>(part + blockIdx.x, n_part, 0.0, lds, ne);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// ---------------------------------------------------------------- evaluation
struct PolyCoef {
  double c[(kPolyMaxOrder + 1) * (kPolyMaxOrder + 1)];
};

template <int O>
__device__ __forceinline__ double poly_value(const PolyCoef& pc, double u, double v) {
  double tu[O + 1], tv[O + 1];
  cheb<O>(u, tu);
  cheb<O>(v, tv);
  double val = 0.0;
#pragma unroll
  for (int j = 0; j <= O; j++) {
    double s = pc.c[j * (O + 1)];
#pragma unroll
    for (int i = 1; i <= O; i++) s = s + pc.c[j * (O + 1) + i] * tu[i];
    val = j == 0 ? s : val + s * tv[j];
  }
  return val;
}

struct EvalArgs {
  const void* in;               // FILL: the frame; ALL: the frame the residuum is taken against or NULL
  long in_pitch;
  const unsigned char* mask;    // FILL: non-zero = replace; NULL: every pixel
  long mask_pitch;
  const double *gy, *gx;        // GRID: pixel positions
  long grid_pitch;
  int fh, fw;                   // the frame of the coordinate map
  int oh, ow;                   // the pixels written
  int tiles_x;
  void* out;
  long out_pitch;
  double* part;                 // one residuum partial per tile or NULL
};

template <typename E, int O, int MODE>
__global__ void __launch_bounds__(kPolyThreads)
poly_eval_kernel(PolyCoef pc, EvalArgs a) {
  __shared__ double lds[kPolyThreads];
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int x = tx * 64 + (threadIdx.x & 63), y = ty * 4 + (threadIdx.x >> 6);
  const E* in = (const E*)a.in;
  E* out = (E*)a.out;
  double dev = 0.0;
  if (x < a.ow && y < a.oh) {
    bool replace = true;
    if (MODE == IPA_POLY_FILL && a.mask) replace = a.mask[(long)y * a.mask_pitch + x] != 0;
    if (replace) {
      double px = (double)x, py = (double)y;
      if (MODE == IPA_POLY_GRID) {
        px = a.gx[(long)y * a.grid_pitch + x];
        py = a.gy[(long)y * a.grid_pitch + x];
      }
      const E nv = (E)poly_value<O>(pc, poly_coord(px, a.fw), poly_coord(py, a.fh));
      if (MODE != IPA_POLY_GRID && in && a.part) dev = fabs((double)nv - (double)in[(long)y * a.in_pitch + x]);
      out[(long)y * a.out_pitch + x] = nv;
    } else if (out != in) {
      out[(long)y * a.out_pitch + x] = in[(long)y * a.in_pitch + x];
    }
  }
  if (MODE != IPA_POLY_GRID && a.part) {   // uniform over the launch
    dev = block_merge<kPolyThreads>(dev, lds);
    if (threadIdx.x == 0) a.part[blockIdx.x] = dev;
  }
}

// ---------------------------------------------------------------- high gradients
template <typename E>
__global__ void __launch_bounds__(kPolyThreads)
laplace_mask_kernel(const E* __restrict__ img, long pitch, int h, int w, int tiles_x, double threshold,
                    unsigned char* __restrict__ out, long out_pitch) {
  int x, y;
  if (!tile_px(tiles_x, h, w, x, y)) return;
  const long yc = (long)y * pitch, yu = (long)max(y - 1, 0) * pitch, yd = (long)min(y + 1, h - 1) * pitch;
  const int xl = max(x - 1, 0), xr = min(x + 1, w - 1);
  const double c = (double)img[yc + x];
  const E a0 = (E)(c * -2.0 + ((double)img[yu + x] + (double)img[yd + x]));
  const E a1 = (E)(c * -2.0 + ((double)img[yc + xl] + (double)img[yc + xr]));
  const E lap = a0 + a1;
  const E mag = lap < (E)0 ? -lap : lap;
  out[(long)y * out_pitch + x] = mag > (E)threshold ? 1 : 0;
}

// the OR over the window [-lo, +hi] along x (VERT 0) or y (VERT 1), clipped to the frame; VERT also counts
template <int VERT>
__global__ void __launch_bounds__(kPolyThreads)
dilate_kernel(const unsigned char* __restrict__ in, long in_pitch, int h, int w, int tiles_x, int lo, int hi,
              unsigned char* __restrict__ out, long out_pitch, unsigned long long* __restrict__ count) {
  __shared__ unsigned wave_n[kPolyWaves];
  int x, y;
  const bool inside = tile_px(tiles_x, h, w, x, y);
  unsigned char v = 0;
  if (inside) {
    if (VERT) {
      for (int yy = max(y - lo, 0); yy <= min(y + hi, h - 1); yy++) v |= in[(long)yy * in_pitch + x];
    } else {
      for (int xx = max(x - lo, 0); xx <= min(x + hi, w - 1); xx++) v |= in[(long)y * in_pitch + xx];
    }
    v = v ? 1 : 0;
    out[(long)y * out_pitch + x] = v;
  }
  if (VERT) {
    const unsigned n = (unsigned)__popcll(__ballot(v != 0));
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned s = 0;
      for (int k = 0; k < kPolyWaves; k++) s += wave_n[k];
      if (s) atomicAdd(count, (unsigned long long)s);   // integers: any order gives the same count
    }
  }
}

template <typename E>
__global__ void __launch_bounds__(kPolyThreads)
clip01_kernel(E* __restrict__ img, long pitch, int h, int w, int tiles_x) {
  int x, y;
  if (!tile_px(tiles_x, h, w, x, y)) return;
  const E v = img[(long)y * pitch + x];
  img[(long)y * pitch + x] = v < (E)0 ? (E)0 : (v > (E)1 ? (E)1 : v);   // NaN stays
}

bool float_dtype(int dtype) { return dtype == IPA_F32 || dtype == IPA_F64; }

template <typename E, int MODE>
int eval_launch(ipa_ctx* ctx, int order, unsigned grid, const PolyCoef& pc, const EvalArgs& a) {
  const int rc = pick<0, 1, 2, 3, 4, 5>(order, [&](auto o) {
    return launch(ctx, poly_eval_kernel<E, decltype(o)::value, MODE>, dim3(grid), dim3(kPolyThreads), 0, pc, a);
  });
  return rc == kNotCovered ? IPA_ERR_BAD_ARG : rc;
}

}  // namespace
}  // namespace ipa

using namespace ipa;

extern "C" {

int ipa_poly2d_moments_dev(ipa_ctx* ctx, const void* d_img, int dtype, int h, int w, long pitch,
                           const unsigned char* d_mask, long mask_pitch, int order, double* moments) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  if (order > kPolyMaxOrder) IPA_UNSUPPORTED(ctx, "poly2d_moments: orders 0 .. %d (got %d)", kPolyMaxOrder, order);
  if (!float_dtype(dtype)) IPA_UNSUPPORTED(ctx, "poly2d_moments: frames are float32 / float64 (got dtype %d)", dtype);
  IPA_REQUIRE(ctx, order >= 0, "poly2d_moments: negative order %d", order);
  IPA_REQUIRE(ctx, d_img && moments, "poly2d_moments: null pointer");
  IPA_REQUIRE(ctx, h > 0 && w > 0, "poly2d_moments: empty image");
  IPA_REQUIRE(ctx, pitch >= w && (!d_mask || mask_pitch >= w), "poly2d_moments: pitch smaller than width");
  const int ne = poly_entries(order);
  const long quads = ((long)h + kPolyWaves - 1) / kPolyWaves;
  long cap = (long)(ctx->cu_count > 0 ? ctx->cu_count : 256) * 8;
  cap = cap < kPolyMaxGrid ? cap : kPolyMaxGrid;
  const int grid = (int)(quads < cap ? quads : cap);
  const int iters = (int)((quads + grid - 1) / grid);
  double *slab, *res;
  int rc = stage_ws(ctx, slot(&slab, (size_t)grid * ne), slot(&res, ne));
  if (rc) return rc;
  rc = by_float(dtype, [&](auto e) {
    using E = decltype(e);
    return pick<0, 1, 2, 3, 4, 5>(order, [&](auto o) {
      return launch(ctx, poly_moments_kernel<E, decltype(o)::value>, dim3(grid), dim3(kPolyThreads), 0, d_img, pitch,
                    d_mask, mask_pitch, h, w, iters, slab);
    });
  });
  if (rc) return rc == kNotCovered ? IPA_ERR_BAD_ARG : rc;
  rc = launch(ctx, poly_sum_columns, dim3(ne), dim3(kPolyThreads), 0, slab, grid, ne, res);
  if (rc) return rc;
  return ipa_stage_out(ctx, {{moments, res, (size_t)ne * sizeof(double)}});
}

int ipa_poly2d_eval_dev(ipa_ctx* ctx, const double* coef, int order, int mode, const void* d_in, int dtype, int h,
                        int w, long in_pitch, const unsigned char* d_mask, long mask_pitch, const double* d_gy,
                        const double* d_gx, int gh, int gw, long grid_pitch, void* d_out, long out_pitch,
                        double* residuum) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  if (order > kPolyMaxOrder) IPA_UNSUPPORTED(ctx, "poly2d_eval: orders 0 .. %d (got %d)", kPolyMaxOrder, order);
  if (!float_dtype(dtype)) IPA_UNSUPPORTED(ctx, "poly2d_eval: frames are float32 / float64 (got dtype %d)", dtype);
  IPA_REQUIRE(ctx, order >= 0, "poly2d_eval: negative order %d", order);
  IPA_REQUIRE(ctx, mode == IPA_POLY_FILL || mode == IPA_POLY_ALL || mode == IPA_POLY_GRID,
              "poly2d_eval: unknown mode %d", mode);
  IPA_REQUIRE(ctx, coef && d_out, "poly2d_eval: null pointer");
  IPA_REQUIRE(ctx, h > 0 && w > 0, "poly2d_eval: empty image");
  const size_t es = ipa_dtype_size(dtype);
  const int oh = mode == IPA_POLY_GRID ? gh : h, ow = mode == IPA_POLY_GRID ? gw : w;
  IPA_REQUIRE(ctx, oh > 0 && ow > 0, "poly2d_eval: empty outgrid");
  IPA_REQUIRE(ctx, out_pitch >= ow, "poly2d_eval: pitch smaller than width");
  const Span out = span2d(d_out, oh, ow, out_pitch, es);
  if (mode == IPA_POLY_GRID) {
    IPA_REQUIRE(ctx, d_gy && d_gx && grid_pitch >= gw, "poly2d_eval: null outgrid or pitch smaller than width");
    IPA_REQUIRE(ctx, !overlap(out, span2d(d_gy, gh, gw, grid_pitch, 8)) &&
                         !overlap(out, span2d(d_gx, gh, gw, grid_pitch, 8)),
                "poly2d_eval: the result overlaps the outgrid");
    IPA_REQUIRE(ctx, !residuum, "poly2d_eval: an outgrid has no residuum");
    d_in = nullptr;
    d_mask = nullptr;
  } else {
    IPA_REQUIRE(ctx, mode == IPA_POLY_ALL || d_in, "poly2d_eval: a fill needs the frame");
    IPA_REQUIRE(ctx, !residuum || d_in, "poly2d_eval: the residuum needs the frame");
    IPA_REQUIRE(ctx, !d_in || in_pitch >= w, "poly2d_eval: pitch smaller than width");
    if (mode == IPA_POLY_ALL) d_mask = nullptr;
    IPA_REQUIRE(ctx, !d_mask || mask_pitch >= w, "poly2d_eval: pitch smaller than width");
    // in place means the very same frame: every pixel is read before it is written by its own lane
    IPA_REQUIRE(ctx, (d_in == d_out && in_pitch == out_pitch) || !overlap(out, span2d(d_in, h, w, in_pitch, es)),
                "poly2d_eval: the result overlaps the frame without being it");
    IPA_REQUIRE(ctx, !overlap(out, span2d(d_mask, h, w, mask_pitch, 1)), "poly2d_eval: the result overlaps the mask");
  }
  int tiles_x;
  unsigned grid;
  int rc = frame_args(ctx, "poly2d_eval", oh, ow, &tiles_x, &grid);
  if (rc) return rc;
  double *part = nullptr, *res = nullptr;
  if (residuum) {
    rc = stage_ws(ctx, slot(&part, grid), slot(&res, 1));
    if (rc) return rc;
  }
  PolyCoef pc;
  const int nc = (order + 1) * (order + 1);
  for (int k = 0; k < (int)(sizeof(pc.c) / sizeof(pc.c[0])); k++) pc.c[k] = k < nc ? coef[k] : 0.0;
  const EvalArgs a = {d_in, in_pitch, d_mask, mask_pitch, d_gy, d_gx, grid_pitch, h, w, oh, ow, tiles_x,
                      d_out, out_pitch, part};
  rc = by_float(dtype, [&](auto e) {
    using E = decltype(e);
    if (mode == IPA_POLY_FILL) return eval_launch<E, IPA_POLY_FILL>(ctx, order, grid, pc, a);
    if (mode == IPA_POLY_ALL) return eval_launch<E, IPA_POLY_ALL>(ctx, order, grid, pc, a);
    return eval_launch<E, IPA_POLY_GRID>(ctx, order, grid, pc, a);
  });
  if (rc || !residuum) return rc;
  rc = launch(ctx, poly_sum_columns, dim3(1), dim3(kPolyThreads), 0, part, (int)grid, 1, res);
  if (rc) return rc;
  return ipa_stage_out(ctx, {{residuum, res, sizeof(double)}});
}

int ipa_high_grad_dev(ipa_ctx* ctx, const void* d_img, int dtype, int h, int w, long pitch, double threshold, int size,
                      unsigned char* d_mask, long mask_pitch, double* count) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  if (!float_dtype(dtype)) IPA_UNSUPPORTED(ctx, "high_grad: frames are float32 / float64 (got dtype %d)", dtype);
  if (size > kHighGradMaxSize) IPA_UNSUPPORTED(ctx, "high_grad: windows up to %d (got %d)", kHighGradMaxSize, size);
  IPA_REQUIRE(ctx, size >= 1, "high_grad: window %d", size);
  IPA_REQUIRE(ctx, d_img && d_mask && count, "high_grad: null pointer");
  int tiles_x;
  unsigned grid;
  int rc = frame_args(ctx, "high_grad", h, w, &tiles_x, &grid);
  if (rc) return rc;
  IPA_REQUIRE(ctx, pitch >= w && mask_pitch >= w, "high_grad: pitch smaller than width");
  IPA_REQUIRE(ctx, !overlap(span2d(d_mask, h, w, mask_pitch, 1), span2d(d_img, h, w, pitch, ipa_dtype_size(dtype))),
              "high_grad: the mask overlaps the frame");
  // workspace: the thresholded Laplacian | its dilation along x | the count
  unsigned char *t0, *t1;
  unsigned long long* d_count;
  rc = stage_ws(ctx, slot(&t0, (size_t)h * w), slot(&t1, (size_t)h * w), slot(&d_count, 1));
  if (rc) return rc;
  IPA_HIP(ctx, hipMemsetAsync(d_count, 0, sizeof(unsigned long long), ctx->stream));
  rc = by_float(dtype, [&](auto e) {
    return launch(ctx, laplace_mask_kernel<decltype(e)>, dim3(grid), dim3(kPolyThreads), 0, d_img, pitch, h, w, tiles_x,
                  threshold, t0, w);
  });
  if (rc) return rc;
  // scipy centres a window of `size` on size // 2: offsets -(size // 2) .. size - size // 2 - 1
  const int lo = size / 2, hi = size - size / 2 - 1;
  rc = launch(ctx, dilate_kernel<0>, dim3(grid), dim3(kPolyThreads), 0, t0, w, h, w, tiles_x, lo, hi, t1, w, nullptr);
  if (rc) return rc;
  rc = launch(ctx, dilate_kernel<1>, dim3(grid), dim3(kPolyThreads), 0, t1, w, h, w, tiles_x, lo, hi, d_mask,
              mask_pitch, d_count);
  if (rc) return rc;
  unsigned long long n = 0;
  rc = ipa_stage_out(ctx, {{&n, d_count, sizeof(n)}});
  if (rc) return rc;
  *count = (double)n;
  return IPA_OK;
}

int ipa_clip01_dev(ipa_ctx* ctx, void* d_img, int dtype, int h, int w, long pitch) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  if (!float_dtype(dtype)) IPA_UNSUPPORTED(ctx, "clip01: frames are float32 / float64 (got dtype %d)", dtype);
  IPA_REQUIRE(ctx, d_img, "clip01: null pointer");
  int tiles_x;
  unsigned grid;
  const int rc = frame_args(ctx, "clip01", h, w, &tiles_x, &grid);
  if (rc) return rc;
  IPA_REQUIRE(ctx, pitch >= w, "clip01: pitch smaller than width");
  return by_float(dtype, [&](auto e) {
    return launch(ctx, clip01_kernel<decltype(e)>, dim3(grid), dim3(kPolyThreads), 0, d_img, pitch, h, w, tiles_x);
  });
}

}  // extern "C"
