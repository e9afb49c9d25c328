// interp_paths.hpp — the constants and predicates by which the kernels and launchers of
// interp_more.hip and resize.hip choose a branch or a kernel, in ONE place: they call these, and
// ipa_interp_path (include/imgproc_hip.h) reports them without a context, so that the tests can
// prove on which side of every boundary a case stands.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/imgproc_hip.h"

namespace ipa {

static inline bool interp_float(int dtype) { return dtype == IPA_F32 || dtype == IPA_F64; }

// 1 / d^power: 2 and 1 have kernels without pow, 0 = the generic one
static inline int idw_power_pick(double power) { return power == 2.0 ? 2 : (power == 1.0 ? 1 : 0); }

// ---------------------------------------------------------------- t / ny by a multiplication --
// a = (t * M) >> 20 with M = ceil(2^20 / ny) is t / ny while t * ny < 2^20 (M errs by less than
// one part in 2^20 / ny).  cross_local_avg_kernel: t < nt, the window's positions;
// circular_idw_kernel: t < nx * ny.
constexpr int kFastDivShift = 20;
__host__ __device__ inline bool cross_fastdiv(int nt, int ny) {
  return (long)nt * ny < (1l << kFastDivShift);
}
__host__ __device__ inline bool circular_fastdiv(int nx, int ny) {
  return ny > 0 && (long)nx * ny * ny < (1l << kFastDivShift);
}
__host__ __device__ inline unsigned fastdiv_mul(int ny) {
  return ((1u << kFastDivShift) + (unsigned)ny - 1u) / (unsigned)ny;
}

// ---------------------------------------------------------------- cross average --
// pixels of a row one wave looks after: the wave works through ITS masked pixels one after the
// other, so a hole costs the launch the time of the wave with the most hole pixels (4K with a
// 200 x 400 hole + 2 % scattered, kernel 5: 64 per wave 906 us, 16 per wave 852)
#ifndef IPA_CROSS_SEG
#define IPA_CROSS_SEG 16
#endif
constexpr int kCrossSeg = IPA_CROSS_SEG;
constexpr int kCrossBallotSteps = 8;   // steps of each of the four searches taken from one ballot
constexpr int kCrossSearchPass = 64;   // steps per pass of cross_search, columns / rows per chunk
                                       // of cross_row_last_kernel / cross_prev_row_kernel

// ---------------------------------------------------------------- point spread --
// ps_sweep_kernel: ONE workgroup of kPsWaves waves, one progress word per row in LDS
constexpr int kPsWaves = 16;
constexpr int kPsMaxRows = 16000;
static inline bool point_spread_rows_ok(int h) { return h <= kPsMaxRows; }

// ---------------------------------------------------------------- fastFilter's statistics --
constexpr int kStatMax = 4096;   // window elements a wave keeps in LDS (doubles)
static inline long fast_stat_per_axis(int ksize, int every) {
  return (2L * ksize + every - 1) / every;
}
static inline bool fast_stat_fits(int ksize, int every) {
  const long per_axis = fast_stat_per_axis(ksize, every);
  return per_axis * per_axis <= kStatMax;
}

// ---------------------------------------------------------------- resize --
// the vertical pass with four result pixels per lane: rows of the intermediate (dw elements
// apart, at tmp) and of the result 4-element aligned
static inline bool resize_vec4(int dw, long dpitch, uintptr_t dst, uintptr_t tmp, size_t esize) {
  return dw % 4 == 0 && dpitch % 4 == 0 && dst % (4 * esize) == 0 && tmp % (4 * esize) == 0;
}
// OpenCV's rule (resize.cpp): INTER_LINEAR at an exact 2 x 2 reduction IS the area average
// ("interpolation == INTER_LINEAR && is_area_fast && iscale_x == 2 && iscale_y == 2")
static inline bool resize_linear_is_area(int sh, int sw, int dh, int dw) {
  return sw == 2 * dw && sh == 2 * dh;
}
static inline double resize_scale(int ssize, int dsize) {
  return 1.0 / ((double)dsize / (double)ssize);
}
// INTER_AREA: 0 = refused (enlarging), 1 = area_fast_kernel (both scales integers; *isx, *isy),
// 2 = area_kernel (decimation tables)
static inline int resize_area_path(double scale_x, double scale_y, int* isx, int* isy) {
  if (!(scale_x >= 1 && scale_y >= 1)) return 0;
  *isx = (int)nearbyint(scale_x);
  *isy = (int)nearbyint(scale_y);
  return fabs(scale_x - *isx) < DBL_EPSILON && fabs(scale_y - *isy) < DBL_EPSILON ? 1 : 2;
}

}  // namespace ipa
