// conv_paths.hpp — which kernel ipa_conv2d_dev / ipa_sepconv2d_dev (conv.hip) launch, as host
// arithmetic in ONE place: the launchers call these, and ipa_conv_path (include/imgproc_hip.h)
// reports them without a context, so that the tests can prove on which side of every threshold
// a case stands.  0 = refused, 1.. = the kernels in the order given per function.
#pragma once
#include <cstddef>

#include "../../include/imgproc_hip.h"
#include "conv_tile.hpp"

namespace ipa {

static inline bool conv_float(int dtype) { return dtype == IPA_F32 || dtype == IPA_F64; }

// ipa_conv2d_dev, after the rank-1 routing of a dense float32 9x9 (that one depends on the
// kernel's VALUES and the knob rank1_sep, and is observed through the counter rank1_routed):
// 1 = marching wave (wave_stencil.hpp: float32, no mask, square 3/5/7, and 9/11 while the knob
//     big_wave is on),
// 2 = LDS tile (conv_kernel: float32 square 3..11 otherwise, float64 square 3/5/7),
// 3 = generic (conv_generic_kernel: any shape of at most 65536 taps)
enum { kConvRefused = 0, kConvWave = 1, kConvTile = 2, kConvGeneric = 3 };
constexpr long kConvGenericMaxTaps = 65536;
static inline int conv2d_path(int dtype, int kh, int kw, bool masked, bool big_wave) {
  if (!conv_float(dtype) || kh < 1 || kw < 1) return kConvRefused;
  bool fast = (kh == kw) && (kh == 3 || kh == 5 || kh == 7 || kh == 9 || kh == 11);
  if (fast && dtype == IPA_F64 && kh > 7) fast = false;  // f64: tuned path instantiated to 7x7
  if (fast && dtype == IPA_F32 && (kh <= 7 || big_wave) && !masked) return kConvWave;
  if (fast) return kConvTile;
  return (long)kh * kw <= kConvGenericMaxTaps ? kConvGeneric : kConvRefused;
}

// ipa_sepconv2d_dev.  The LDS kernel (sepconv_kernel) holds two planes of a 128 x 32 tile:
// (32 + 2 (nky / 2)) input rows and 32 rows after the y pass, each 128 + 2 hxa wide, hxa the x
// radius rounded up to 4
constexpr int kSepMaxTaps = 63;                    // per axis: SepWeights travels as kernel argument
constexpr size_t kSepLdsGiveUp = 150 * 1024;       // above: the generic kernel, axis by axis
constexpr size_t kSepLdsOptIn = 64 * 1024;         // above: hipFuncAttributeMaxDynamicSharedMemorySize
static inline size_t sepconv_lds(size_t esize, int nky, int nkx) {
  const int hxa = ((nkx / 2 + 3) / 4) * 4;
  return (size_t)(2 * kTileH + 2 * (nky / 2)) * (kTileW + 2 * hxa) * esize;
}
// too long for the kernel argument table or the LDS planes
static inline bool sepconv_long(size_t esize, int nky, int nkx) {
  return nky > kSepMaxTaps || nkx > kSepMaxTaps || sepconv_lds(esize, nky, nkx) > kSepLdsGiveUp;
}
// float32, equal short tap counts: the wave-marching separable kernel (wave_sep.hip)
static inline bool sepconv_wave(int dtype, int nky, int nkx) {
  return dtype == IPA_F32 && nky == nkx && (nky == 3 || nky == 5 || nky == 7 || nky == 9);
}
// An even tap count is refused only where the kernel is short: long ones go to the generic kernel,
// which centres at k / 2 like scipy.  (esize of the image's dtype whatever it is, 0 if unknown: the
// launcher refuses short even taps before it looks at the dtype.)
static inline bool sepconv_taps_ok(size_t esize, int nky, int nkx) {
  return sepconv_long(esize, nky, nkx) || ((nky == 0 || (nky & 1)) && (nkx == 0 || (nkx & 1)));
}
// 1 = marching separable wave, 2 = LDS kernel within 64 KiB, 3 = LDS kernel with the dynamic-LDS
// opt-in, 4 = two launches of the generic kernel through a temporary, 5 = one launch of the
// generic kernel (a long kernel on one axis only).  The launcher switches on this value.
enum { kSepRefused = 0, kSepWave = 1, kSepLds = 2, kSepLdsBig = 3, kSepTwoGeneric = 4,
       kSepOneGeneric = 5 };
static inline int sepconv2d_path(int dtype, int nky, int nkx) {
  if (!conv_float(dtype) || nky < 0 || nkx < 0) return kSepRefused;
  const size_t es = dtype == IPA_F32 ? 4 : 8;
  if (!sepconv_taps_ok(es, nky, nkx)) return kSepRefused;
  if (sepconv_long(es, nky, nkx)) {
    if (nky == 0 || nkx == 0)
      return conv2d_path(dtype, nky ? nky : 1, nkx ? nkx : 1, false, true) == kConvGeneric
                 ? kSepOneGeneric : kSepRefused;
    return conv2d_path(dtype, nky, 1, false, true) == kConvGeneric &&
                   conv2d_path(dtype, 1, nkx, false, true) == kConvGeneric
               ? kSepTwoGeneric : kSepRefused;
  }
  if (sepconv_wave(dtype, nky, nkx)) return kSepWave;
  return sepconv_lds(es, nky, nkx) <= kSepLdsOptIn ? kSepLds : kSepLdsBig;
}

}  // namespace ipa
