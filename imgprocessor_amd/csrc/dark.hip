// dark.hip — dark current calibration on gfx950: what camera/DarkCurrentMap.py needs around the
// single-time-effect kernel of ste.hip.
//   ipa_pair_min_dev          features/SingleTimeEffectDetection.py:39-42 (np.min((i1, i2), axis=0),
//                             the image handed to oneImageNLF)
//   ipa_nlf_threshold_dev     features/SingleTimeEffectDetection.py:44 (nlf(avg) * nStd) for the three
//                             functions camera/NoiseLevelFunction.py:94-151 can return
//   ipa_stack_linregress_dev  camera/DarkCurrentMap.py:61-80 (getLinearityFunction)
//   ipa_dark_current_eval_dev camera/CameraCalibration.py:509-519 (offset + ascent * t, limited)
//   ipa_cast_trunc_dev        camera/DarkCurrentMap.py:108-114 (`i[:] = avg` into imgs[0].dtype)
//
// Everything is float64, every operation correctly rounded and unfused (Makefile + pragma), NaN
// goes where numpy sends it.  All five are streaming kernels: one pixel per lane, no LDS, no
// atomics.  The fit keeps a pixel's samples in registers between its three sums for T <= 16, so
// every frame value comes from HBM once; longer stacks read the samples again per sum.  Where rows,
// frames and outputs are aligned for it, a lane of the fit owns 4 (uint8, uint16) or 2 (float32)
// adjacent pixels and loads and stores them as one vector.
//
// UNPINNED: fancytools.math.linRegressUsingMasked2dArrays, which getLinearityFunction calls, is
// neither part of the reference tree nor installed where the fixtures are made.  The least-squares
// definition in the header (means, centred sums in frame order, rms residual) is this project's.
#include "common.hpp"
#include "frame_args.hpp"
#include "launch.hpp"
#include "nlf_fn.hpp"

#pragma clang fp contract(off)

namespace ipa {
namespace {

constexpr int kDarkThreads = 256;   // a 64 x 4 tile
constexpr int kDarkMaxT = 64;
constexpr int kDarkRegT = 16;       // longest stack held in registers

struct Times {
  double x[kDarkMaxT];
};

template <typename T>
__global__ void __launch_bounds__(kDarkThreads)
pair_min_kernel(const T* __restrict__ f0, const T* __restrict__ f1, int h, int w, long pitch0, long pitch1,
                int tiles_x, double* __restrict__ out, long out_pitch) {
  int x, y;
  if (!tile_px(tiles_x, h, w, x, y)) return;
  out[(long)y * out_pitch + x] = np_min((double)f0[(long)y * pitch0 + x], (double)f1[(long)y * pitch1 + x]);
}

__global__ void __launch_bounds__(kDarkThreads)
nlf_threshold_kernel(const double* __restrict__ xs, int h, int w, long pitch, int tiles_x, NlfParams f,
                     double nstd, double* __restrict__ thr, long thr_pitch) {
  int x, y;
  if (!tile_px(tiles_x, h, w, x, y)) return;
  thr[(long)y * thr_pitch + x] = nlf_eval(f, xs[(long)y * pitch + x]) * nstd;
}

struct RegressArgs {
  const void* stack;
  long pitch, frame_stride;
  int T, h, w, tiles_x;
  double mx_intensity, min_ascent, mid_x;   // mid_x = 0.5 * (min(x) + max(x)) over all T times
  double* offset;
  double* ascent;
  double* error;
  long out_pitch;
};

// pixels per lane: 4 or 8 bytes of every frame per lane where rows, frames and outputs are
// aligned to that (regress_vec_ok), else 1
template <typename T> constexpr int kRegressPx = sizeof(T) <= 2 ? 4 : sizeof(T) == 4 ? 2 : 1;

// A lane owns PX adjacent pixels of a row (a tile is 64 * PX x 4 pixels) and fits them one after
// the other.  REG > 0: the samples of a stack of T <= REG frames stay in registers, in their
// element type; REG == 0: read per sum.
template <typename T, int REG, int PX>
__global__ void __launch_bounds__(kDarkThreads)
stack_linregress_kernel(RegressArgs a, Times t) {
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int x0 = (tx * 64 + (threadIdx.x & 63)) * PX, y = ty * 4 + (threadIdx.x >> 6);
  if (x0 >= a.w || y >= a.h) return;
  const int npx = min(PX, a.w - x0);   // < PX in the last lane of a row whose width is no multiple
  const T* px = (const T*)a.stack + (long)y * a.pitch + x0;
  constexpr int N = REG > 0 ? REG : 1;
  PxVec<T, PX> raw[N];
  if constexpr (REG > 0) {
#pragma unroll
    for (int k = 0; k < N; k++) {
      if (k >= a.T) continue;
      const T* p = px + (long)k * a.frame_stride;
      if (PX == 1 || npx == PX) {
        raw[k] = *(const PxVec<T, PX>*)p;
      } else {
#pragma unroll
        for (int j = 0; j < PX; j++) raw[k].v[j] = j < npx ? p[j] : T(0);
      }
    }
  }
  PxVec<double, PX> r_off, r_asc, r_err;
  // pixel j of the lane; j is a compile-time constant, so raw and the results stay in registers
  auto fit = [&](auto jc) {
    constexpr int j = decltype(jc)::value;
    r_off.v[j] = r_asc.v[j] = r_err.v[j] = 0.0;
    if (j >= npx) return;
    auto sample = [&](int k) -> double { return (double)px[(long)k * a.frame_stride + j]; };
    // valid: !(y > mxIntensity) - a NaN sample counts and poisons the pixel, as `imgs > mxIntensity` does
    int n = 0;
    double sx = 0.0, sy = 0.0;
    if constexpr (REG > 0) {
#pragma unroll
      for (int k = 0; k < N; k++) {
        if (k >= a.T) break;
        const double v = (double)raw[k].v[j];
        if (!(v > a.mx_intensity)) {
          n++;
          sx += t.x[k];
          sy += v;
        }
      }
    } else {
      for (int k = 0; k < a.T; k++) {
        const double v = sample(k);
        if (!(v > a.mx_intensity)) {
          n++;
          sx += t.x[k];
          sy += v;
        }
      }
    }
    const double dn = (double)n;
    const double mx = sx / dn, my = sy / dn;
    double sxx = 0.0, sxy = 0.0;
    if constexpr (REG > 0) {
#pragma unroll
      for (int k = 0; k < N; k++) {
        if (k >= a.T) break;
        const double v = (double)raw[k].v[j];
        if (!(v > a.mx_intensity)) {
          const double dx = t.x[k] - mx;
          sxx += dx * dx;
          sxy += dx * (v - my);
        }
      }
    } else {
      for (int k = 0; k < a.T; k++) {
        const double v = sample(k);
        if (!(v > a.mx_intensity)) {
          const double dx = t.x[k] - mx;
          sxx += dx * dx;
          sxy += dx * (v - my);
        }
      }
    }
    double ascent = sxy / sxx;
    double offset = my - ascent * mx;
    double se = 0.0;
    if constexpr (REG > 0) {
#pragma unroll
      for (int k = 0; k < N; k++) {
        if (k >= a.T) break;
        const double v = (double)raw[k].v[j];
        if (!(v > a.mx_intensity)) {
          const double r = v - (offset + ascent * t.x[k]);
          se += r * r;
        }
      }
    } else {
      for (int k = 0; k < a.T; k++) {
        const double v = sample(k);
        if (!(v > a.mx_intensity)) {
          const double r = v - (offset + ascent * t.x[k]);
          se += r * r;
        }
      }
    }
    // getLinearityFunction's own steps (:73-78)
    if (ascent != ascent) ascent = 0.0;
    if (a.min_ascent > 0.0 && ascent < a.min_ascent) {
      offset = offset + a.mid_x * ascent;
      ascent = 0.0;
    }
    r_off.v[j] = offset;
    r_asc.v[j] = ascent;
    r_err.v[j] = sqrt(se / dn);
  };
  fit(std::integral_constant<int, 0>{});
  if constexpr (PX > 1) fit(std::integral_constant<int, 1>{});
  if constexpr (PX > 2) {
    fit(std::integral_constant<int, 2>{});
    fit(std::integral_constant<int, 3>{});
  }
  static_assert(PX == 1 || PX == 2 || PX == 4, "1, 2 or 4 pixels per lane");
  const long o = (long)y * a.out_pitch + x0;
  if (PX == 1 || npx == PX) {
    *(PxVec<double, PX>*)(a.offset + o) = r_off;
    *(PxVec<double, PX>*)(a.ascent + o) = r_asc;
    *(PxVec<double, PX>*)(a.error + o) = r_err;
  } else {
#pragma unroll
    for (int j = 0; j < PX; j++)
      if (j < npx) {
        a.offset[o + j] = r_off.v[j];
        a.ascent[o + j] = r_asc.v[j];
        a.error[o + j] = r_err.v[j];
      }
  }
}

// may every lane load `px` adjacent samples of every frame, and store `px` results, as one vector?
bool regress_vec_ok(const RegressArgs& a, size_t es, int px) {
  const size_t in = es * px, out = 8 * (size_t)px;
  return (uintptr_t)a.stack % in == 0 && (a.pitch * es) % in == 0 && (a.frame_stride * es) % in == 0 &&
         (uintptr_t)a.offset % out == 0 && (uintptr_t)a.ascent % out == 0 && (uintptr_t)a.error % out == 0 &&
         a.out_pitch % px == 0;
}

template <typename O>
__global__ void __launch_bounds__(kDarkThreads)
dark_eval_kernel(const double* __restrict__ offset, const double* __restrict__ ascent, int h, int w, long pitch,
                 int tiles_x, double t, double limit, O* __restrict__ out, long out_pitch) {
  int x, y;
  if (!tile_px(tiles_x, h, w, x, y)) return;
  const long i = (long)y * pitch + x;
  double bg = offset[i] + ascent[i] * t;
  if (bg > limit) bg = limit;   // NaN stays
  out[(long)y * out_pitch + x] = (O)bg;
}

template <typename O>
__global__ void __launch_bounds__(kDarkThreads)
cast_trunc_kernel(const double* __restrict__ in, int h, int w, long pitch, int tiles_x, O* __restrict__ out,
                  long out_pitch) {
  int x, y;
  if (!tile_px(tiles_x, h, w, x, y)) return;
  out[(long)y * out_pitch + x] = (O)in[(long)y * pitch + x];
}

}  // namespace
}  // namespace ipa

using namespace ipa;

extern "C" {

int ipa_pair_min_dev(ipa_ctx* ctx, const void* d_f0, const void* d_f1, int dtype, int h, int w, long pitch0,
                     long pitch1, double* d_out, long out_pitch) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  IPA_REQUIRE(ctx, d_f0 && d_f1 && d_out, "pair_min: null pointer");
  int tiles_x;
  unsigned grid;
  int rc = frame_args(ctx, "pair_min", h, w, &tiles_x, &grid);
  if (rc) return rc;
  IPA_REQUIRE(ctx, pitch0 >= w && pitch1 >= w && out_pitch >= w, "pair_min: pitch smaller than width");
  if (!known_dtype(dtype))
    IPA_UNSUPPORTED(ctx, "pair_min: frames are uint8 / uint16 / float32 / float64 (got dtype %d)", dtype);
  const size_t es = ipa_dtype_size(dtype);
  const Span out = span2d(d_out, h, w, out_pitch, 8);
  IPA_REQUIRE(ctx, !overlap(out, span2d(d_f0, h, w, pitch0, es)) && !overlap(out, span2d(d_f1, h, w, pitch1, es)),
              "pair_min does not run in place");
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return launch(ctx, pair_min_kernel<T>, dim3(grid), dim3(kDarkThreads), 0, d_f0, d_f1, h, w, pitch0, pitch1,
                  tiles_x, d_out, out_pitch);
  });
}

int ipa_nlf_threshold_dev(ipa_ctx* ctx, const double* d_x, int h, int w, long pitch, int kind,
                          const double* params, double nstd, double* d_thr, long thr_pitch) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  IPA_REQUIRE(ctx, d_x && d_thr && params, "nlf_threshold: null pointer");
  int tiles_x;
  unsigned grid;
  int rc = frame_args(ctx, "nlf_threshold", h, w, &tiles_x, &grid);
  if (rc) return rc;
  IPA_REQUIRE(ctx, pitch >= w && thr_pitch >= w, "nlf_threshold: pitch smaller than width");
  const int n_params = nlf_param_count(kind);
  IPA_REQUIRE(ctx, n_params, "nlf_threshold: unknown kind %d", kind);
  // in place is fine - a lane reads its pixel before it writes it -, a partial overlap is not
  const bool same = d_x == d_thr && pitch == thr_pitch;
  IPA_REQUIRE(ctx, same || !overlap(span2d(d_x, h, w, pitch, 8), span2d(d_thr, h, w, thr_pitch, 8)),
              "nlf_threshold: x and thr overlap without being the same array");
  NlfParams f;
  f.kind = kind;
  for (int i = 0; i < 5; i++) f.p[i] = i < n_params ? params[i] : 0.0;
  return launch(ctx, nlf_threshold_kernel, dim3(grid), dim3(kDarkThreads), 0, d_x, h, w, pitch, tiles_x, f, nstd,
                d_thr, thr_pitch);
}

int ipa_stack_linregress_dev(ipa_ctx* ctx, const void* d_stack, int dtype, int T, int h, int w, long pitch,
                             long frame_stride, const double* times, double mx_intensity, double min_ascent,
                             double* d_offset, double* d_ascent, double* d_error, long out_pitch) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  if (T > kDarkMaxT) IPA_UNSUPPORTED(ctx, "stack_linregress: at most %d frames (got %d)", kDarkMaxT, T);
  IPA_REQUIRE(ctx, T >= 2, "stack_linregress: a line needs at least 2 frames (got %d)", T);
  IPA_REQUIRE(ctx, d_stack && times && d_offset && d_ascent && d_error, "stack_linregress: null pointer");
  int tiles_x;
  unsigned grid;
  int rc = frame_args(ctx, "stack_linregress", h, w, &tiles_x, &grid);
  if (rc) return rc;
  IPA_REQUIRE(ctx, pitch >= w && out_pitch >= w, "stack_linregress: pitch smaller than width");
  IPA_REQUIRE(ctx, frame_stride >= (long)(h - 1) * pitch + w, "stack_linregress: frames overlap");
  if (!known_dtype(dtype))
    IPA_UNSUPPORTED(ctx, "stack_linregress: frames are uint8 / uint16 / float32 / float64 (got dtype %d)", dtype);
  const Span spans[] = {span2d(d_offset, h, w, out_pitch, 8), span2d(d_ascent, h, w, out_pitch, 8),
                        span2d(d_error, h, w, out_pitch, 8),
                        span_stack(d_stack, T, h, w, pitch, frame_stride, ipa_dtype_size(dtype))};
  IPA_REQUIRE(ctx, !written_overlaps(spans, 3), "stack_linregress: stack and outputs overlap");
  Times t;
  double lo = times[0], hi = times[0];
  for (int k = 0; k < kDarkMaxT; k++) {
    t.x[k] = k < T ? times[k] : 0.0;
    if (k < T) {   // np.min / np.max: a NaN time wins
      lo = (times[k] < lo || times[k] != times[k]) ? times[k] : lo;
      hi = (times[k] > hi || times[k] != times[k]) ? times[k] : hi;
    }
  }
  RegressArgs a;
  a.stack = d_stack;
  a.pitch = pitch;
  a.frame_stride = frame_stride;
  a.T = T;
  a.h = h;
  a.w = w;
  a.tiles_x = tiles_x;
  a.mx_intensity = mx_intensity;
  a.min_ascent = min_ascent;
  a.mid_x = 0.5 * (lo + hi);
  a.offset = d_offset;
  a.ascent = d_ascent;
  a.error = d_error;
  a.out_pitch = out_pitch;
  const int reg = T <= 4 ? 4 : T <= 8 ? 8 : T <= kDarkRegT ? kDarkRegT : 0;
  return by_dtype(dtype, [&](auto e) {
    using E = decltype(e);
    return pick<4, 8, kDarkRegT, 0>(reg, [&](auto r) {
      constexpr int R = decltype(r)::value;
      constexpr int P = kRegressPx<E>;
      if constexpr (P > 1) {
        if (regress_vec_ok(a, sizeof(E), P)) {
          RegressArgs v = a;
          v.tiles_x = (w + 64 * P - 1) / (64 * P);
          return launch(ctx, stack_linregress_kernel<E, R, P>, dim3((unsigned)v.tiles_x * ((h + 3) / 4)),
                        dim3(kDarkThreads), 0, v, t);
        }
      }
      return launch(ctx, stack_linregress_kernel<E, R, 1>, dim3(grid), dim3(kDarkThreads), 0, a, t);
    });
  });
}

int ipa_dark_current_eval_dev(ipa_ctx* ctx, const double* d_offset, const double* d_ascent, int h, int w,
                              long pitch, double t, double limit, void* d_out, int out_dtype, long out_pitch) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  IPA_REQUIRE(ctx, d_offset && d_ascent && d_out, "dark_current_eval: null pointer");
  int tiles_x;
  unsigned grid;
  int rc = frame_args(ctx, "dark_current_eval", h, w, &tiles_x, &grid);
  if (rc) return rc;
  IPA_REQUIRE(ctx, pitch >= w && out_pitch >= w, "dark_current_eval: pitch smaller than width");
  if (out_dtype != IPA_F32 && out_dtype != IPA_F64)
    IPA_UNSUPPORTED(ctx, "dark_current_eval: the output is float32 / float64 (got dtype %d)", out_dtype);
  const Span out = span2d(d_out, h, w, out_pitch, ipa_dtype_size(out_dtype));
  IPA_REQUIRE(ctx, !overlap(out, span2d(d_offset, h, w, pitch, 8)) && !overlap(out, span2d(d_ascent, h, w, pitch, 8)),
              "dark_current_eval does not run in place");
  return by_float(out_dtype, [&](auto o) {
    using O = decltype(o);
    return launch(ctx, dark_eval_kernel<O>, dim3(grid), dim3(kDarkThreads), 0, d_offset, d_ascent, h, w, pitch,
                  tiles_x, t, limit, d_out, out_pitch);
  });
}

int ipa_cast_trunc_dev(ipa_ctx* ctx, const double* d_in, int h, int w, long pitch, void* d_out, int out_dtype,
                       long out_pitch) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  IPA_REQUIRE(ctx, d_in && d_out, "cast_trunc: null pointer");
  int tiles_x;
  unsigned grid;
  int rc = frame_args(ctx, "cast_trunc", h, w, &tiles_x, &grid);
  if (rc) return rc;
  IPA_REQUIRE(ctx, pitch >= w && out_pitch >= w, "cast_trunc: pitch smaller than width");
  if (!known_dtype(out_dtype))
    IPA_UNSUPPORTED(ctx, "cast_trunc: the output is uint8 / uint16 / float32 / float64 (got dtype %d)", out_dtype);
  IPA_REQUIRE(ctx, !overlap(span2d(d_in, h, w, pitch, 8), span2d(d_out, h, w, out_pitch, ipa_dtype_size(out_dtype))),
              "cast_trunc does not run in place");
  return by_dtype(out_dtype, [&](auto o) {
    using O = decltype(o);
    return launch(ctx, cast_trunc_kernel<O>, dim3(grid), dim3(kDarkThreads), 0, d_in, h, w, pitch, tiles_x, d_out,
                  out_pitch);
  });
}

}  // extern "C"
