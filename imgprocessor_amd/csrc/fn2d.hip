// fn2d.hip — least-squares fits of a vignetting function to a masked flat field on gfx950: what
// camera/flatField/postprocessing/function.py does through fancytools' fit2dArrayToFn, with the two functions
// the reference fits (camera/flatField/postProcessing.py:50-74).
//   ipa_fn2d_normal_dev  function.py:35-37           the sums of one Levenberg-Marquardt trial over the valid pixels
//   ipa_fn2d_eval_dev    function.py:35-40, :42      the fitted function into the masked pixels / every pixel / an
//                                                    outgrid, and the maximum of the result
//   ipa_fn2d_divide_dev  function.py:42              img2 /= img2.max()
//
// The model's x is the ROW index and its y the COLUMN index, as np.where(mask) and np.fromfunction hand them over.
//   IPA_FN2D_KW   equations/vignetting.py:21-37, tilt = 0   params {f, alpha, cx, cy}
//       dx = x - cx;  dy = y - cy;  d = sqrt(dx*dx + dy*dy);  t = d / f;  q = 1 + t*t
//       A = 1.0 / (q*q);  G = 1 - alpha*d;  val = A*G
//   IPA_FN2D_AOV  equations/angleOfView.py:29-40            params {tan(a), c0, c1}; the fitted parameter is a
//       dx = x - c0;  dy = y - c1;  val = 1 / sqrt(1 + tan_a * ((dx*dx + dy*dy) / c0))
// eval computes exactly this in double, nothing fused (Makefile + pragma), and rounds once into the frame's type:
// bit for bit numpy's value of the reference's expressions (tests/fn2d_ref.py, tests/golden/fn2d.npz).
//
// normal.  With model value m, Jacobian J (P = 4 or 1 columns) and r = z - m the call returns the upper triangle
// of J^T J row by row, J^T r, S = sum r*r and the number of valid pixels: 16 doubles for KW, 4 for AoV.  It uses a
// cheaper formulation of m than eval does - one division per pixel, what is constant along a row hoisted - spelled
// out at Model<.>::terms and restated operation by operation in tests/fn2d_ref.py.  alpha * dx / d is 0 where
// d == 0.  Masked pixels are selected out, never multiplied by zero: a NaN under the mask enters nothing.
// A wave walks rows 4 (g + k grid) + wave, k = 0, 1, ..; its lanes stride along the row and keep the sums in
// registers over all their rows; one butterfly over the wave adds them in a fixed order, thread e of the
// workgroup adds entry e of the four waves, wave 0 first, into one slab per workgroup, and a second launch adds
// the slabs through merge_partials (reduce.hpp).  No float atomics: two calls give identical bits.
#include "common.hpp"
#include "frame_args.hpp"
#include "launch.hpp"
#include "reduce.hpp"

#pragma clang fp contract(off)

namespace ipa {
namespace {

constexpr int kFnThreads = 256;
constexpr int kFnWaves = kFnThreads / 64;
constexpr int kFnMaxGrid = 2048;
constexpr int kFnAhead = 4;          // pixels a lane has in flight along its row
constexpr int kFnMaxParams = 4;

struct FnPar {
  double p[kFnMaxParams];
};

template <int MODEL>
struct Model;

template <>
struct Model<IPA_FN2D_KW> {
  static constexpr int P = 4;
  static constexpr int NPAR = 4;
  // the reference's operation order (equations/vignetting.py:23-37)
  static __device__ __forceinline__ double value(const FnPar& k, double x, double y) {
    const double dx = x - k.p[2], dy = y - k.p[3];
    const double d = sqrt(dx * dx + dy * dy);
    const double t = d / k.p[0];
    const double q = 1.0 + t * t;
    const double A = 1.0 / (q * q);
    const double G = 1.0 - k.p[1] * d;
    return A * G;
  }
  // per call: {1 / f^2, 4 / f^2, 4 / f^3}
  struct Hoist {
    double inv_f2, k4, k4f;
  };
  static __device__ __forceinline__ Hoist hoist(const FnPar& k) {
    const double f2 = k.p[0] * k.p[0];
    return {1.0 / f2, 4.0 / f2, 4.0 / (f2 * k.p[0])};
  }
  // m and dm / d{f, alpha, cx, cy} at a pixel of a row with dx2 = dx * dx
  static __device__ __forceinline__ double terms(const FnPar& k, const Hoist& c, double dx, double dx2, double y,
                                                 double (&J)[P]) {
    const double dy = y - k.p[3];
    const double r2 = dx2 + dy * dy;
    const double d = sqrt(r2);
    const double q = 1.0 + r2 * c.inv_f2;
    const double dd = d == 0.0 ? 1.0 : d;
    const double wq = 1.0 / (q * dd);             // the one division: 1 / q and 1 / d from it
    const double iq = wq * dd;
    const double id = d == 0.0 ? 0.0 : wq * q;
    const double A = iq * iq;
    const double G = 1.0 - k.p[1] * d;
    const double gaq = G * A * iq;
    const double cc = gaq * c.k4 + A * k.p[1] * id;
    J[0] = gaq * c.k4f * r2;
    J[1] = -(A * d);
    J[2] = cc * dx;
    J[3] = cc * dy;
    return A * G;
  }
};

template <>
struct Model<IPA_FN2D_AOV> {
  static constexpr int P = 1;
  static constexpr int NPAR = 3;
  // equations/angleOfView.py:37-40
  static __device__ __forceinline__ double value(const FnPar& k, double x, double y) {
    const double dx = x - k.p[1], dy = y - k.p[2];
    return 1.0 / sqrt(1.0 + k.p[0] * ((dx * dx + dy * dy) / k.p[1]));
  }
  // per call: {1 / c0, -(1 + tan_a^2) / 2}: d tan(a) / da = 1 + tan(a)^2
  struct Hoist {
    double inv_c0, hs;
  };
  static __device__ __forceinline__ Hoist hoist(const FnPar& k) {
    return {1.0 / k.p[1], -0.5 * (1.0 + k.p[0] * k.p[0])};
  }
  static __device__ __forceinline__ double terms(const FnPar& k, const Hoist& c, double dx, double dx2, double y,
                                                 double (&J)[P]) {
    const double dy = y - k.p[2];
    const double g = (dx2 + dy * dy) * c.inv_c0;
    const double u = 1.0 + k.p[0] * g;
    const double m = 1.0 / sqrt(u);
    J[0] = c.hs * (m * m * m) * g;
    return m;
  }
};

__host__ __device__ constexpr int fn_entries(int P) { return P * (P + 1) / 2 + P + 2; }

// ---------------------------------------------------------------- normal equations
template <int P>
struct NormalSums {
  double v[fn_entries(P)];   // upper triangle of J^T J by rows | J^T r | sum r * r | valid pixels (exact below 2^53)
  __device__ __forceinline__ void add(const double (&J)[P], double r) {
    int e = 0;
#pragma unroll
    for (int i = 0; i < P; i++)
#pragma unroll
      for (int j = i; j < P; j++) v[e++] += J[i] * J[j];
#pragma unroll
    for (int i = 0; i < P; i++) v[e++] += J[i] * r;
    v[e++] += r * r;
    v[e] += 1.0;
  }
};

// slab[blockIdx.x][e]
template <typename E, int MODEL>
__global__ void __launch_bounds__(kFnThreads)
fn2d_normal_kernel(FnPar par, const E* __restrict__ img, long pitch, const unsigned char* __restrict__ mask,
                   long mask_pitch, int h, int w, int iters, double* __restrict__ slab) {
  using M = Model<MODEL>;
  constexpr int P = M::P, NE = fn_entries(P);
  __shared__ double waves[kFnWaves][NE];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const typename M::Hoist c = M::hoist(par);
  NormalSums<P> s;
#pragma unroll
  for (int e = 0; e < NE; e++) s.v[e] = 0.0;
  for (int it = 0; it < iters; it++) {
    const long row = ((long)it * gridDim.x + blockIdx.x) * kFnWaves + wave;
    if (row >= h) break;
    const E* __restrict__ p = img + row * pitch;
    const unsigned char* __restrict__ m = mask ? mask + row * mask_pitch : nullptr;
    const double dx = (double)row - par.p[MODEL == IPA_FN2D_KW ? 2 : 1];
    const double dx2 = dx * dx;
    double J[P];
    int x = lane;
    for (; x + (kFnAhead - 1) * 64 < w; x += kFnAhead * 64) {
      E z[kFnAhead];
      unsigned char mk[kFnAhead];
#pragma unroll
      for (int k = 0; k < kFnAhead; k++) {
        z[k] = p[x + k * 64];
        mk[k] = m ? m[x + k * 64] : (unsigned char)0;
      }
#pragma unroll
      for (int k = 0; k < kFnAhead; k++)
        if (!mk[k]) {
          const double mv = M::terms(par, c, dx, dx2, (double)(x + k * 64), J);
          s.add(J, (double)z[k] - mv);
        }
    }
    for (; x < w; x += 64)
      if (!m || !m[x]) {
        const double mv = M::terms(par, c, dx, dx2, (double)x, J);
        s.add(J, (double)p[x] - mv);
      }
  }
  // butterfly: every lane ends with the same bits, partners add the same two values
#pragma unroll
  for (int d = 32; d > 0; d >>= 1)
#pragma unroll
    for (int e = 0; e < NE; e++) s.v[e] += __shfl_xor(s.v[e], d);
  if (lane == 0)
#pragma unroll
    for (int e = 0; e < NE; e++) waves[wave][e] = s.v[e];
  __syncthreads();
  if (t < NE) {
    double acc = 0.0;
    for (int wv = 0; wv < kFnWaves; wv++) acc += waves[wv][t];
    slab[(long)blockIdx.x * NE + t] = acc;
  }
}

// one workgroup per entry adds the slabs: thread t takes slabs t, t + 256, .., then the tree
__global__ void __launch_bounds__(kFnThreads)
fn2d_sum_columns(const double* __restrict__ part, int n_part, int ne, double* __restrict__ out) {
  __shared__ double lds[kFnThreads];
  const double s = merge_partials<kFnThreads>(part + blockIdx.x, n_part, 0.0, lds, ne);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// ---------------------------------------------------------------- evaluation
// numpy's maximum: a NaN on either side gives NaN
struct NanMax {
  double v;
};
__device__ inline NanMax merge(NanMax a, NanMax b) {
  if (a.v != a.v) return a;
  if (b.v != b.v) return b;
  return a.v < b.v ? b : a;
}

struct FnEvalArgs {
  const void* in;               // FILL: the frame
  long in_pitch;
  const unsigned char* mask;    // FILL: non-zero = replace; NULL: every pixel
  long mask_pitch;
  const double *gy, *gx;        // GRID: pixel positions, the row position from gy
  long grid_pitch;
  int oh, ow;                   // the pixels written
  int tiles_x;
  void* out;
  long out_pitch;
  NanMax* part;                 // one maximum per tile or NULL
};

template <typename E, int MODEL, int MODE>
__global__ void __launch_bounds__(kFnThreads)
fn2d_eval_kernel(FnPar par, FnEvalArgs a) {
  __shared__ NanMax lds[kFnThreads];
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int x = tx * 64 + (threadIdx.x & 63), y = ty * 4 + (threadIdx.x >> 6);
  const E* in = (const E*)a.in;
  E* out = (E*)a.out;
  NanMax top = {-INFINITY};
  if (x < a.ow && y < a.oh) {
    bool replace = true;
    if (MODE == IPA_POLY_FILL && a.mask) replace = a.mask[(long)y * a.mask_pitch + x] != 0;
    E nv;
    if (replace) {
      double px = (double)x, py = (double)y;
      if (MODE == IPA_POLY_GRID) {
        px = a.gx[(long)y * a.grid_pitch + x];
        py = a.gy[(long)y * a.grid_pitch + x];
      }
      nv = (E)Model<MODEL>::value(par, py, px);   // the model's x is the row
      out[(long)y * a.out_pitch + x] = nv;
    } else {
      nv = in[(long)y * a.in_pitch + x];
      if (out != in) out[(long)y * a.out_pitch + x] = nv;
    }
    top.v = (double)nv;
  }
  if (a.part) {   // uniform over the launch
    top = block_merge<kFnThreads>(top, lds);
    if (threadIdx.x == 0) a.part[blockIdx.x] = top;
  }
}

__global__ void __launch_bounds__(kFnThreads)
fn2d_max_partials(const NanMax* __restrict__ part, int n_part, double* __restrict__ out) {
  __shared__ NanMax lds[kFnThreads];
  const NanMax s = merge_partials<kFnThreads>(part, n_part, NanMax{-INFINITY}, lds);
  if (threadIdx.x == 0) out[0] = s.v;
}

template <typename E>
__global__ void __launch_bounds__(kFnThreads)
fn2d_divide_kernel(E* __restrict__ img, long pitch, int h, int w, int tiles_x, E div) {
  int x, y;
  if (!tile_px(tiles_x, h, w, x, y)) return;
  img[(long)y * pitch + x] = img[(long)y * pitch + x] / div;
}

bool float_dtype(int dtype) { return dtype == IPA_F32 || dtype == IPA_F64; }

// the parameters of a model as the kernels take them; 0: unknown model
int load_params(int model, const double* params, FnPar* par) {
  const int n = model == IPA_FN2D_KW ? Model<IPA_FN2D_KW>::NPAR : model == IPA_FN2D_AOV ? Model<IPA_FN2D_AOV>::NPAR : 0;
  for (int k = 0; k < kFnMaxParams; k++) par->p[k] = k < n ? params[k] : 0.0;
  return n;
}

template <typename E, int MODEL>
int eval_launch(ipa_ctx* ctx, int mode, unsigned grid, const FnPar& par, const FnEvalArgs& a) {
  const int rc = pick<IPA_POLY_FILL, IPA_POLY_ALL, IPA_POLY_GRID>(mode, [&](auto m) {
    return launch(ctx, fn2d_eval_kernel<E, MODEL, decltype(m)::value>, dim3(grid), dim3(kFnThreads), 0, par, a);
  });
  return rc == kNotCovered ? IPA_ERR_BAD_ARG : rc;
}

}  // namespace
}  // namespace ipa

using namespace ipa;

extern "C" {

int ipa_fn2d_normal_dev(ipa_ctx* ctx, const void* d_img, int dtype, int h, int w, long pitch,
                        const unsigned char* d_mask, long mask_pitch, int model, const double* params, double* sums) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  if (!float_dtype(dtype)) IPA_UNSUPPORTED(ctx, "fn2d_normal: frames are float32 / float64 (got dtype %d)", dtype);
  IPA_REQUIRE(ctx, model == IPA_FN2D_KW || model == IPA_FN2D_AOV, "fn2d_normal: unknown model %d", model);
  IPA_REQUIRE(ctx, d_img && params && sums, "fn2d_normal: null pointer");
  IPA_REQUIRE(ctx, h > 0 && w > 0, "fn2d_normal: empty image");
  IPA_REQUIRE(ctx, pitch >= w && (!d_mask || mask_pitch >= w), "fn2d_normal: pitch smaller than width");
  FnPar par;
  load_params(model, params, &par);
  const int ne = fn_entries(model == IPA_FN2D_KW ? Model<IPA_FN2D_KW>::P : Model<IPA_FN2D_AOV>::P);
  const long quads = ((long)h + kFnWaves - 1) / kFnWaves;
  long cap = (long)(ctx->cu_count > 0 ? ctx->cu_count : 256) * 8;
  cap = cap < kFnMaxGrid ? cap : kFnMaxGrid;
  const int grid = (int)(quads < cap ? quads : cap);
  const int iters = (int)((quads + grid - 1) / grid);
  double *slab, *res;
  int rc = stage_ws(ctx, slot(&slab, (size_t)grid * ne), slot(&res, ne));
  if (rc) return rc;
  rc = by_float(dtype, [&](auto e) {
    using E = decltype(e);
    return pick<IPA_FN2D_KW, IPA_FN2D_AOV>(model, [&](auto m) {
      return launch(ctx, fn2d_normal_kernel<E, decltype(m)::value>, dim3(grid), dim3(kFnThreads), 0, par, d_img, pitch,
                    d_mask, mask_pitch, h, w, iters, slab);
    });
  });
  if (rc) return rc == kNotCovered ? IPA_ERR_BAD_ARG : rc;
  rc = launch(ctx, fn2d_sum_columns, dim3(ne), dim3(kFnThreads), 0, slab, grid, ne, res);
  if (rc) return rc;
  return ipa_stage_out(ctx, {{sums, res, (size_t)ne * sizeof(double)}});
}

int ipa_fn2d_eval_dev(ipa_ctx* ctx, int model, const double* params, int mode, const void* d_in, int dtype, int h,
                      int w, long in_pitch, const unsigned char* d_mask, long mask_pitch, const double* d_gy,
                      const double* d_gx, int gh, int gw, long grid_pitch, void* d_out, long out_pitch,
                      double* maximum) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  if (!float_dtype(dtype)) IPA_UNSUPPORTED(ctx, "fn2d_eval: frames are float32 / float64 (got dtype %d)", dtype);
  IPA_REQUIRE(ctx, model == IPA_FN2D_KW || model == IPA_FN2D_AOV, "fn2d_eval: unknown model %d", model);
  IPA_REQUIRE(ctx, mode == IPA_POLY_FILL || mode == IPA_POLY_ALL || mode == IPA_POLY_GRID,
              "fn2d_eval: unknown mode %d", mode);
  IPA_REQUIRE(ctx, params && d_out, "fn2d_eval: null pointer");
  IPA_REQUIRE(ctx, h > 0 && w > 0, "fn2d_eval: empty image");
  const size_t es = ipa_dtype_size(dtype);
  const int oh = mode == IPA_POLY_GRID ? gh : h, ow = mode == IPA_POLY_GRID ? gw : w;
  IPA_REQUIRE(ctx, oh > 0 && ow > 0, "fn2d_eval: empty outgrid");
  IPA_REQUIRE(ctx, out_pitch >= ow, "fn2d_eval: pitch smaller than width");
  const Span out = span2d(d_out, oh, ow, out_pitch, es);
  if (mode == IPA_POLY_GRID) {
    IPA_REQUIRE(ctx, d_gy && d_gx && grid_pitch >= gw, "fn2d_eval: null outgrid or pitch smaller than width");
    IPA_REQUIRE(ctx, !overlap(out, span2d(d_gy, gh, gw, grid_pitch, 8)) &&
                         !overlap(out, span2d(d_gx, gh, gw, grid_pitch, 8)),
                "fn2d_eval: the result overlaps the outgrid");
    d_in = nullptr;
    d_mask = nullptr;
  } else if (mode == IPA_POLY_ALL) {
    d_in = nullptr;
    d_mask = nullptr;
  } else {
    IPA_REQUIRE(ctx, d_in, "fn2d_eval: a fill needs the frame");
    IPA_REQUIRE(ctx, in_pitch >= w && (!d_mask || mask_pitch >= w), "fn2d_eval: pitch smaller than width");
    // in place means the very same frame: every pixel is read before it is written by its own lane
    IPA_REQUIRE(ctx, (d_in == d_out && in_pitch == out_pitch) || !overlap(out, span2d(d_in, h, w, in_pitch, es)),
                "fn2d_eval: the result overlaps the frame without being it");
    IPA_REQUIRE(ctx, !overlap(out, span2d(d_mask, h, w, mask_pitch, 1)), "fn2d_eval: the result overlaps the mask");
  }
  int tiles_x;
  unsigned grid;
  int rc = frame_args(ctx, "fn2d_eval", oh, ow, &tiles_x, &grid);
  if (rc) return rc;
  NanMax* part = nullptr;
  double* res = nullptr;
  if (maximum) {
    rc = stage_ws(ctx, slot(&part, grid), slot(&res, 1));
    if (rc) return rc;
  }
  FnPar par;
  load_params(model, params, &par);
  const FnEvalArgs a = {d_in, in_pitch, d_mask, mask_pitch, d_gy, d_gx, grid_pitch, oh, ow, tiles_x,
                        d_out, out_pitch, part};
  rc = by_float(dtype, [&](auto e) {
    using E = decltype(e);
    if (model == IPA_FN2D_KW) return eval_launch<E, IPA_FN2D_KW>(ctx, mode, grid, par, a);
    return eval_launch<E, IPA_FN2D_AOV>(ctx, mode, grid, par, a);
  });
  if (rc || !maximum) return rc;
  rc = launch(ctx, fn2d_max_partials, dim3(1), dim3(kFnThreads), 0, part, (int)grid, res);
  if (rc) return rc;
  return ipa_stage_out(ctx, {{maximum, res, sizeof(double)}});
}

int ipa_fn2d_divide_dev(ipa_ctx* ctx, void* d_img, int dtype, int h, int w, long pitch, double div) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  if (!float_dtype(dtype)) IPA_UNSUPPORTED(ctx, "fn2d_divide: frames are float32 / float64 (got dtype %d)", dtype);
  IPA_REQUIRE(ctx, d_img, "fn2d_divide: null pointer");
  int tiles_x;
  unsigned grid;
  const int rc = frame_args(ctx, "fn2d_divide", h, w, &tiles_x, &grid);
  if (rc) return rc;
  IPA_REQUIRE(ctx, pitch >= w, "fn2d_divide: pitch smaller than width");
  return by_float(dtype, [&](auto e) {
    using E = decltype(e);
    return launch(ctx, fn2d_divide_kernel<E>, dim3(grid), dim3(kFnThreads), 0, d_img, pitch, h, w, tiles_x, (E)div);
  });
}

}  // extern "C"
