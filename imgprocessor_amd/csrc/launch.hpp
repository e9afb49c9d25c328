// launch.hpp — how the entry points (stencils*.hip, interp_more.hip, idw.hip, resize.hip, nan_to_zero, the
// calibration units, conv.hip) get from run-time arguments to ONE typed kernel launch.  Host code, no state:
//   by_float(dtype, f)       f(float{}) or f(double{}); the caller has refused other dtypes
//   by_dtype(dtype, f)       the same over the four element types of known_dtype()
//   pick<Vs...>(v, f)        f(std::integral_constant<., V>{}) for the listed V equal to v,
//                            kNotCovered when there is none
//   pick_or_last<Vs...>      the same with the last listed value as the fallback
//   launch(ctx, kernel, ...) on ctx's device and stream, every argument converted to the kernel's
//                            declared parameter type; returns the status of the launch
// The calibration units reserve their workspace and read their results back through stage_ws() (frame_args.hpp) and
// ipa_stage_out (common.hpp), and reduce through reduce.hpp.
// conv.hip launches its own kernels through launch().  The wave launchers it routes to (wave_sep.hip, wave_conv_big.hip,
// the tail of fused_impl.hpp) and the rest of the hot path (remap*, fused*, tile_warp*) fill their parameters while they
// size their grids and write hipLaunchKernelGGL themselves; the wave launchers return hipGetLastError's status.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace ipa {

// pick(): no listed value matches.  Every IPA_* status is <= 0 (IPA_OK 0, the errors negative), so
// no status can be mistaken for it; it must not reach a caller of the C ABI.
constexpr int kNotCovered = 1;
static_assert(IPA_OK == 0 && IPA_ERR_BAD_ARG < 0 && IPA_ERR_UNSUPPORTED < 0 && IPA_ERR_HIP < 0 &&
                  IPA_ERR_OOM < 0 && IPA_ERR_NO_DEVICE < 0, "kNotCovered must differ from every status");

template <typename F>
int by_float(int dtype, F&& f) {
  return dtype == IPA_F32 ? f(float{}) : f(double{});
}

inline bool known_dtype(int dtype) {
  return dtype == IPA_U8 || dtype == IPA_U16 || dtype == IPA_F32 || dtype == IPA_F64;
}

// f(T{}) for the element type of `dtype`; the caller has refused unknown dtypes
template <typename F>
int by_dtype(int dtype, F&& f) {
  switch (dtype) {
    case IPA_U8: return f((unsigned char)0);
    case IPA_U16: return f((unsigned short)0);
    case IPA_F32: return f(float{});
    default: return f(double{});
  }
}

template <auto... Vs, typename V, typename F>
int pick(V v, F&& f) {
  int rc = kNotCovered;
  (void)((v == Vs ? (rc = f(std::integral_constant<decltype(Vs), Vs>{}), true) : false) || ...);
  return rc;
}

template <auto... Vs, typename V, typename F>
int pick_or_last(V v, F&& f) {
  constexpr V vs[] = {Vs...};
  return pick<Vs...>(((v == Vs) || ...) ? v : vs[sizeof...(Vs) - 1], f);
}

// static_cast, not a C cast: void* becomes the kernel's T*, int widens to long - and a float*
// handed to a double* parameter, or a const pointer to a writable one, does not compile.
template <typename... KA, typename... A>
int launch(ipa_ctx* ctx, void (*kernel)(KA...), dim3 grid, dim3 block, size_t lds, A... args) {
  static_assert(sizeof...(KA) == sizeof...(A), "argument count differs from the kernel's");
  IPA_HIP(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(kernel, grid, block, lds, ctx->stream, static_cast<KA>(args)...);
  IPA_HIP(ctx, hipGetLastError());
  return IPA_OK;
}

}  // namespace ipa

// stencils_ydep.hip, for ipa_local_std_dev (stencils.hip): the 256-px wave kernel of the square half
// windows 1..5 (local_std_path() == 1).  The launch's status, or ipa::kNotCovered for any other hkx.
int ipa_local_std_wave_launch(ipa_ctx* ctx, const void* img, const void* blurred, int dtype, int h,
                              int w, long pitch, long bpitch, int hkx, int hky, void* out,
                              long opitch);
