// frame_args.hpp — what the eleven calibration units (ste.hip, nlm.hip, nlf.hip, dark.hip, flat.hip, tss.hip,
// ovs.hip, poly.hip, spot.hip, steps.hip, fn2d.hip) share.  Host side: the byte spans of pitched frames and frame stacks with their overlap checks,
// the checks and grid of the 64 x 4 tiles, and stage_ws(): the workspace of a call as a list of typed slots over
// ipa_stage_in (common.hpp), which ipa_stage_out answers at the call's end.  Device side, for the streaming per-pixel
// kernels of dark / flat / tss / ovs: a lane's pixel on that tile grid and vectors of adjacent pixels.  launch.hpp holds
// the known element types, the dispatch on them and the typed launch; reduce.hpp the workgroup reduction of the units
// that sum a frame up (block_merge, merge_partials).
#pragma once
#include "common.hpp"

namespace ipa {

// pixel of this lane on the 64 x 4 tile grid; false outside the image
__device__ inline bool tile_px(int tiles_x, int h, int w, int& x, int& y) {
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  x = tx * 64 + (threadIdx.x & 63);
  y = ty * 4 + (threadIdx.x >> 6);
  return x < w && y < h;
}

// PX adjacent pixels of a row, loaded and stored as one vector
template <typename T, int PX>
struct alignas(sizeof(T) * PX) PxVec {
  T v[PX];
};

struct Span {
  const void* p;
  size_t bytes;
};
// n frames of h rows of w elements, `stride` elements from one frame to the next; empty for a null pointer
inline Span span_stack(const void* p, int n, int h, long w, long pitch, long stride, size_t es) {
  return {p, p ? ((size_t)(n - 1) * stride + (size_t)(h - 1) * pitch + w) * es : 0};
}
inline Span span2d(const void* p, int h, long w, long pitch, size_t es) { return span_stack(p, 1, h, w, pitch, 0, es); }
inline bool overlap(Span a, Span b) {
  if (!a.p || !b.p) return false;
  const char *pa = (const char*)a.p, *pb = (const char*)b.p;
  return pa < pb + b.bytes && pb < pa + a.bytes;
}
// does one of the first k spans - the arrays a call writes - overlap any other of the n?
template <int N>
bool written_overlaps(const Span (&s)[N], int k) {
  for (int i = 0; i < k; i++)
    for (int j = 0; j < N; j++)
      if (j != i && overlap(s[i], s[j])) return true;
  return false;
}

// ipa_stage_in with every slot's pointer in its own type: slot(&p, n) is n elements of *p, uploaded from `host`
// where one is given; p is null for n == 0.
//   Moments* part;  double* res;
//   rc = stage_ws(ctx, slot(&part, grid), slot(&res, 5));
template <typename T>
struct WsSlot {
  T** p;
  size_t n;
  const T* host;
};
template <typename T>
WsSlot<T> slot(T** p, size_t n, const T* host = nullptr) { return {p, n, host}; }
template <typename... T>
int stage_ws(ipa_ctx* ctx, WsSlot<T>... s) {
  char* d[sizeof...(T)];
  const int rc = ipa_stage_in(ctx, {{s.host, s.n * sizeof(T)}...}, d);
  if (rc) return rc;
  int i = 0;
  ((*s.p = (T*)d[i++]), ...);
  return IPA_OK;
}

// the checks every call shares; *tiles_x and *grid for the 64 x 4 tiles
inline int frame_args(ipa_ctx* ctx, const char* what, int h, int w, int* tiles_x, unsigned* grid) {
  IPA_REQUIRE(ctx, h > 0 && w > 0, "%s: empty image", what);
  const long tx = (w + 63) / 64, ty = (h + 3) / 4;
  IPA_REQUIRE(ctx, tx * ty <= 0x7fffffffL, "%s: image too large", what);
  *tiles_x = (int)tx;
  *grid = (unsigned)(tx * ty);
  return IPA_OK;
}

}  // namespace ipa
