// nlf_fn.hpp — the noise level function as the kernels evaluate it (ste.hip, nlf.hip):
// camera/NoiseLevelFunction.py:94-107 in float64, every operation correctly rounded.  Translation
// units that include it are built with FP contraction off.
#pragma once

#include <float.h>

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

}  // namespace ipa
