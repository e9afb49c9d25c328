// reduce.hpp — the one workgroup reduction of the calibration units (nlf.hip, flat.hip, poly.hip, spot.hip,
// steps.hip, fn2d.hip).  Device side.  Every fixed-order sum of those units is two stages of it:
//   1  workgroup b of `grid` walks its share of the frame, every lane folds its samples into a value of its own in
//      the order it meets them, block_merge() folds the lanes, lane 0 stores partial b;
//   2  one workgroup: merge_partials() - lane t folds partials t, t + THREADS, ..., then block_merge() again.
// Values combine through an unqualified merge(a, b): the unit's own overload for its struct (found by argument
// dependent lookup), or the ones below for a plain double or int.  The order of both stages is part of the units'
// contract - "two calls give identical bits", and tests/test_gpu_reduce_order.py restates it bit for bit
// (tests/reduce_ref.py) - so the grid of stage 1 stays a number in the unit that owns it.
#pragma once
#include "common.hpp"

namespace ipa {

__device__ inline double merge(double a, double b) { return a + b; }
__device__ inline int merge(int a, int b) { return a + b; }

// The tree over the workgroup's THREADS lanes, top down: in the step of width s = THREADS / 2, .., 1 lane t < s
// becomes merge(lane t, lane t + s).  Every lane returns lane 0's result.  `lds` holds THREADS values and is free
// again after the caller's next barrier.
template <int THREADS, typename P>
__device__ inline P block_merge(P v, P* lds) {
  const int t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (int s = THREADS / 2; s > 0; s >>= 1) {
    if (t < s) lds[t] = merge(lds[t], lds[t + s]);
    __syncthreads();
  }
  return lds[0];
}

// stage 2: lane t folds part[t * stride], part[(t + THREADS) * stride], .. onto `identity` in that order, then the tree
template <int THREADS, typename P>
__device__ inline P merge_partials(const P* part, int n_part, P identity, P* lds, long stride = 1) {
  for (int p = threadIdx.x; p < n_part; p += THREADS) identity = merge(identity, part[p * stride]);
  return block_merge<THREADS>(identity, lds);
}

}  // namespace ipa
