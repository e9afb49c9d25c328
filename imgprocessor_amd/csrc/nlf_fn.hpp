// nlf_fn.hpp — the noise level function as the kernels evaluate it (ste.hip, nlf.hip, dark.hip,
// flat.hip): camera/NoiseLevelFunction.py:94-151 in float64, every operation correctly rounded; and
// the 3 x 3 median of nlf.hip and flat.hip.  Translation units that include it are built with FP
// contraction off.
#pragma once

#include <float.h>

#include "../../include/imgproc_hip.h"

namespace ipa {

// numpy's maximum / minimum as they run here (np.max / np.min over axis 0, np.maximum): NaN in
// either operand propagates; on equal operands the second one is returned.
__device__ inline double np_max(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ inline double np_min(double a, double b) { return (a < b || a != a) ? a : b; }

// boundedFunction(x, minY, ax, ay) = maximum(nan_to_num(ay * sqrt(x - ax)), minY)
__device__ inline double bounded_nlf(double x, double min_y, double ax, double ay) {
  double y = ay * sqrt(x - ax);
  if (y != y) y = 0.0;
  else if (y == __builtin_inf()) y = DBL_MAX;
  else if (y == -__builtin_inf()) y = -DBL_MAX;
  return np_max(y, min_y);
}

// one of the three functions camera/NoiseLevelFunction.py can return (ipa_nlf_kind), by value
struct NlfParams {
  int kind;
  double p[5];
};
// parameters of a kind: 3 / 5 / 1, 0 for an unknown kind
inline int nlf_param_count(int kind) {
  return kind == IPA_NLF_BOUNDED_SQRT ? 3 : kind == IPA_NLF_CLIPPED_POLY ? 5 : kind == IPA_NLF_CONSTANT ? 1 : 0;
}
__device__ inline double nlf_eval(const NlfParams& f, double v) {
  if (f.kind == IPA_NLF_BOUNDED_SQRT) return bounded_nlf(v, f.p[0], f.p[1], f.p[2]);
  if (f.kind == IPA_NLF_CLIPPED_POLY) {
    // np.clip: minimum(maximum(x, x0), x1), a NaN x passes through both
    double c = v < f.p[3] ? f.p[3] : v;
    c = c > f.p[4] ? f.p[4] : c;
    // np.polyval's Horner loop, from y = 0
    double n = 0.0 * c + f.p[0];
    n = n * c + f.p[1];
    return n * c + f.p[2];
  }
  return f.p[0];
}

// compare-exchange with numpy's NaN rule: a NaN reaches both outputs
__device__ inline void cswap(double& a, double& b) {
  const double lo = np_min(a, b), hi = np_max(a, b);
  a = lo;
  b = hi;
}
__device__ inline double med3(double a, double b, double c) {
  return np_max(np_min(a, b), np_min(np_max(a, b), c));
}
// scipy.ndimage.median_filter(., 3) at one pixel: rank 4 of the window c[column][row], which is
// sorted along its columns on return.  A NaN in the window gives NaN.
__device__ inline double median9(double (&c)[3][3]) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
    cswap(c[i][0], c[i][1]);
    cswap(c[i][1], c[i][2]);
    cswap(c[i][0], c[i][1]);
  }
  // sorted columns: the median of 9 is the median of (largest minimum, median of the medians,
  // smallest maximum)
  const double lo = np_max(np_max(c[0][0], c[1][0]), c[2][0]);
  const double mid = med3(c[0][1], c[1][1], c[2][1]);
  const double hi = np_min(np_min(c[0][2], c[1][2]), c[2][2]);
  return med3(lo, mid, hi);
}

}  // namespace ipa
