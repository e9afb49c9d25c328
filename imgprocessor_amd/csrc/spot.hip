// spot.hip — the flat field from spot images on gfx950: camera/flatField/vignettingFromSpotAverage.py
// ("Method B": one small bright device imaged at many positions), and the three primitives it needs.
//   ipa_spot_range_dev       skimage threshold_otsu's all-equal test and np.histogram's range (:56)
//   ipa_spot_histogram_dev   np.histogram(img.ravel(), nbins) under threshold_otsu (:56)
//   ipa_spot_mask_dev        minimum_filter(img > t, 3) (:61)
//   ipa_label_dev            skimage.measure.label / scipy.ndimage.label (:61)
//   ipa_label_sizes_dev      (spots == i).sum() for every i (:63)
//   ipa_label_largest_dev    np.argmax(spot_sizes) + 1 and the sums under center_of_mass (:66, :72)
//   ipa_spot_take_dev        mx2, fitimg[spot] = img[spot], mask[spot] = 1 (:72-77)
//
// A frame is uint8 / uint16 / float32 / float64 with a pitch; every value is (double)px - bg, one IEEE
// subtraction as numpy's `img -= avgBg` (contraction off: Makefile + pragma).  Everything up to the
// take is integer or selection arithmetic and equals numpy / skimage / scipy bit for bit.
//
// Labelling is a union-find whose roots are the SMALLEST linear index y * w + x of their component:
// every union points the larger root at the smaller, so parent indices strictly decrease along every
// chain and the consecutive numbers, given in the order of the roots, are those of a raster scan for
// first pixels.  Six launches, each reading what the one before wrote:
//   1 tile      64 x 16 tiles labelled in LDS; every pixel's global parent = its tile's root
//   2 seam      pixels on a tile's top row, left and right column unite with their neighbours in
//               other tiles: atomicMin on the global parents, agent-scope loads
//   3 flatten   every pixel finds its root and points at it; roots counted per block of 1024
//               consecutive linear indices
//   4 scan      one workgroup: exclusive scan of the block counts, the total is n
//   5 number    the roots of a block get offset + rank + 1, stored at parent[root] as -1 - number
//   6 write     label = number of the pixel's root
// No loop anywhere waits for another workgroup: a find or a union only ever follows or lowers parent
// indices, and a stale read is an older - still valid - ancestor.
#include "common.hpp"
#include "frame_args.hpp"
#include "launch.hpp"
#include "reduce.hpp"

#pragma clang fp contract(off)

namespace ipa {
namespace {

constexpr int kSpotThreads = 256;
constexpr int kSpotMaxBins = 2048;    // edges + four wave tables of u32: 48 KB of LDS
constexpr int kSpotMaxGrid = 1024;
constexpr int kRun = 8;               // consecutive pixels of one row per lane (histogram)
constexpr long kSpotMaxPixels = 0x7fffffffL;   // linear indices are int32
constexpr int kTW = 64, kTH = 16, kTilePx = kTW * kTH;   // labelling tile; four pixels per thread
constexpr int kSeamThreads = 128;

// the frame as the reference sees it after `img -= avgBg`
struct SpotSrc {
  const void* img;
  const double* bg;   // NULL: bg_value
  long pitch, bg_pitch;
  double bg_value;
};

template <typename T>
__device__ inline double src_px(const SpotSrc& s, int y, int x) {
  const double v = (double)((const T*)s.img)[(long)y * s.pitch + x];
  return v - (s.bg ? s.bg[(long)y * s.bg_pitch + x] : s.bg_value);
}

// ---------------------------------------------------------------- range
struct Range {
  double mn, mx;
  unsigned long long nan, inf;
};
__device__ inline Range merge(const Range& a, const Range& b) {
  return {b.mn < a.mn ? b.mn : a.mn, b.mx > a.mx ? b.mx : a.mx, a.nan + b.nan, a.inf + b.inf};
}

// a unit is 256 consecutive pixels of one row
template <typename T>
__global__ void __launch_bounds__(kSpotThreads)
spot_range_kernel(SpotSrc s, int h, int w, Range* __restrict__ part) {
  __shared__ Range lds[kSpotThreads];
  const long upr = (w + kSpotThreads - 1) / kSpotThreads, units = (long)h * upr;
  Range m = {__builtin_inf(), -__builtin_inf(), 0, 0};
  for (long u = blockIdx.x; u < units; u += gridDim.x) {
    const long y = u / upr;
    const int x = (int)(u - y * upr) * kSpotThreads + threadIdx.x;
    if (x >= w) continue;
    const double v = src_px<T>(s, (int)y, x);
    if (v != v) {
      m.nan++;
      continue;
    }
    if (v == __builtin_inf() || v == -__builtin_inf()) m.inf++;
    m.mn = v < m.mn ? v : m.mn;
    m.mx = v > m.mx ? v : m.mx;
  }
  m = block_merge<kSpotThreads>(m, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = m;
}

// res = {min, max, NaN count, +-inf count, the first pixel}
template <typename T>
__global__ void __launch_bounds__(kSpotThreads)
spot_range_final(SpotSrc s, const Range* __restrict__ part, int n_part, double* __restrict__ res) {
  __shared__ Range lds[kSpotThreads];
  const Range m = merge_partials<kSpotThreads>(part, n_part, {__builtin_inf(), -__builtin_inf(), 0, 0}, lds);
  if (threadIdx.x != 0) return;
  res[0] = m.mn;
  res[1] = m.mx;
  res[2] = (double)m.nan;
  res[3] = (double)m.inf;
  res[4] = src_px<T>(s, 0, 0);
}

// ---------------------------------------------------------------- histogram
// np.histogram's rule for equal bins: the estimate k = (intp)((x - e[0]) * norm), k == nbins -> nbins - 1,
// then its two corrections against the edge table - so that e[k] <= x < e[k + 1], the last bin closed.
// Every wave owns one table of nbins u32 in LDS; a lane takes kRun consecutive pixels of one row and
// merges equal-bin neighbours in registers before it touches the table.  Integer adds only: the
// counts do not depend on any order.  LDS: edges | counts[waves][nbins].
template <typename T>
__global__ void __launch_bounds__(kSpotThreads)
spot_hist_kernel(SpotSrc s, int h, int w, const double* __restrict__ edges, int nbins, double norm,
                 unsigned* __restrict__ slab) {
  extern __shared__ double lds[];
  const int waves = kSpotThreads >> 6, wave = threadIdx.x >> 6;
  double* e = lds;
  unsigned* cnts = (unsigned*)(e + nbins + 1);
  for (int i = threadIdx.x; i <= nbins; i += kSpotThreads) e[i] = edges[i];
  for (int i = threadIdx.x; i < waves * nbins; i += kSpotThreads) cnts[i] = 0u;
  __syncthreads();
  unsigned* wcnt = cnts + wave * nbins;
  const long rpr = (w + kRun - 1) / kRun, nruns = (long)h * rpr;
  const long stride = (long)gridDim.x * kSpotThreads;
  const double e0 = e[0];
  for (long r = (long)blockIdx.x * kSpotThreads + threadIdx.x; r < nruns; r += stride) {
    const long y = r / rpr;
    const int x0 = (int)(r - y * rpr) * kRun, x1 = min(x0 + kRun, w);
    int bin = -1;
    unsigned n = 0;
    for (int x = x0; x < x1; x++) {
      const double v = src_px<T>(s, (int)y, x);
      const double f = (v - e0) * norm;
      // the caller has refused non-finite values; the clamp keeps a wild estimate inside the table
      int k = f >= (double)nbins ? nbins - 1 : (f > 0.0 ? (int)f : 0);
      if (v < e[k] && k > 0) k--;
      if (v >= e[k + 1] && k != nbins - 1) k++;
      if (k != bin) {
        if (n) atomicAdd(&wcnt[bin], n);
        bin = k;
        n = 0;
      }
      n++;
    }
    if (n) atomicAdd(&wcnt[bin], n);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < nbins; b += kSpotThreads) {
    unsigned c = 0u;
    for (int wv = 0; wv < waves; wv++) c += cnts[wv * nbins + b];
    slab[(long)blockIdx.x * nbins + b] = c;
  }
}

// one thread per bin adds the workgroups' slabs
__global__ void __launch_bounds__(kSpotThreads)
spot_hist_final(const unsigned* __restrict__ slab, int n_slab, int nbins, unsigned long long* __restrict__ cnt) {
  const int b = blockIdx.x * kSpotThreads + threadIdx.x;
  if (b >= nbins) return;
  unsigned long long c = 0;
  for (int g = 0; g < n_slab; g++) c += slab[(long)g * nbins + b];
  cnt[b] = c;
}

// ---------------------------------------------------------------- spot mask
// minimum_filter(img > t, 3) of a bool image with scipy's `reflect` border: the 3 x 3 erosion in
// which positions beyond the frame do not count.  NaN > t is false.
template <typename T>
__global__ void __launch_bounds__(kSpotThreads)
spot_mask_kernel(SpotSrc s, int h, int w, int tiles_x, double t, unsigned char* __restrict__ mask, long mask_pitch) {
  int x, y;
  if (!tile_px(tiles_x, h, w, x, y)) return;
  bool all = true;
#pragma unroll
  for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
    for (int dx = -1; dx <= 1; dx++) {
      const int yy = y + dy, xx = x + dx;
      if (yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
      all = all && (src_px<T>(s, yy, xx) > t);
    }
  }
  mask[(long)y * mask_pitch + x] = all ? 1 : 0;
}

// ---------------------------------------------------------------- labelling: union-find
// SCOPE: __HIP_MEMORY_SCOPE_WORKGROUP for a tile's table in LDS, __HIP_MEMORY_SCOPE_AGENT for the
// global parents other workgroups are lowering at the same time (each XCD has its own L2).
template <int SCOPE>
__device__ inline int uf_load(const int* par, int i) {
  return __hip_atomic_load(par + i, __ATOMIC_RELAXED, SCOPE);
}

// the root of i.  Terminates: a parent is never larger than its child, so i strictly decreases
// until par[i] == i; nothing here waits for another thread to write.
template <int SCOPE>
__device__ inline int uf_find(const int* par, int i) {
  for (int p = uf_load<SCOPE>(par, i); p != i; p = uf_load<SCOPE>(par, i)) i = p;
  return i;
}

// One set out of those of a and b, the smaller root on top.  Terminates: every pass either returns
// or replaces the larger of the two indices by a strictly smaller one (a root found below it, or the
// parent another thread gave it in the meantime); no pass waits for anybody's progress.
template <int SCOPE>
__device__ inline void uf_unite(int* par, int a, int b) {
  for (;;) {
    a = uf_find<SCOPE>(par, a);
    b = uf_find<SCOPE>(par, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = __hip_atomic_fetch_min(par + a, b, __ATOMIC_RELAXED, SCOPE);
    if (old == a) return;   // a was a root and points at b now
    a = old;                // a had a parent old < a already: its set and b's are still to be joined
  }
}

// phase 1: one 64 x 16 tile in LDS.  Local indices ly * 64 + lx keep the raster order of the global
// ones, so the tile's local roots are its smallest global indices.
__global__ void __launch_bounds__(kSpotThreads)
label_tile_kernel(const unsigned char* __restrict__ mask, int h, int w, long mask_pitch, int tiles_x, int conn8,
                  int* __restrict__ parent) {
  constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
  __shared__ int lp[kTilePx];
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x0 = tx * kTW, y0 = ty * kTH;
  const int lx = threadIdx.x & 63, r0 = threadIdx.x >> 6;   // rows r0, r0 + 4, r0 + 8, r0 + 12
  const int gx = x0 + lx;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int ly = r0 + 4 * k, gy = y0 + ly, l = ly * kTW + lx;
    const bool fg = gx < w && gy < h && mask[(long)gy * mask_pitch + gx] != 0;
    lp[l] = fg ? l : -1;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int ly = r0 + 4 * k, l = ly * kTW + lx;
    if (uf_load<WG>(lp, l) < 0) continue;
    if (lx > 0 && uf_load<WG>(lp, l - 1) >= 0) uf_unite<WG>(lp, l, l - 1);
    if (ly == 0) continue;
    if (uf_load<WG>(lp, l - kTW) >= 0) uf_unite<WG>(lp, l, l - kTW);
    if (!conn8) continue;
    if (lx > 0 && uf_load<WG>(lp, l - kTW - 1) >= 0) uf_unite<WG>(lp, l, l - kTW - 1);
    if (lx < kTW - 1 && uf_load<WG>(lp, l - kTW + 1) >= 0) uf_unite<WG>(lp, l, l - kTW + 1);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int ly = r0 + 4 * k, gy = y0 + ly, l = ly * kTW + lx;
    if (gx >= w || gy >= h) continue;
    int r = lp[l];
    if (r >= 0) {
      r = uf_find<WG>(lp, l);
      r = (int)((long)(y0 + (r >> 6)) * w + x0 + (r & 63));
    }
    parent[(long)gy * w + gx] = r;
  }
}

// phase 2: the foreground pixels on a tile's top row, left column and right column unite with
// their backward neighbours (left, up; with 8 neighbours also up-left and up-right) that lie in
// ANOTHER tile - every adjacency across a seam is one of those.  Background parents are -1.
__global__ void __launch_bounds__(kSeamThreads)
label_seam_kernel(int* __restrict__ parent, int h, int w, int tiles_x, int conn8) {
  constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int t = threadIdx.x;
  int lx, ly;
  if (t < kTW) {
    lx = t, ly = 0;
  } else if (t < kTW + kTH - 1) {
    lx = 0, ly = t - kTW + 1;
  } else if (t < kTW + 2 * (kTH - 1)) {
    lx = kTW - 1, ly = t - (kTW + kTH - 1) + 1;
  } else {
    return;
  }
  const int gx = tx * kTW + lx, gy = ty * kTH + ly;
  if (gx >= w || gy >= h) return;
  const int p = (int)((long)gy * w + gx);
  if (uf_load<AG>(parent, p) < 0) return;
  const int ndir = conn8 ? 4 : 2;
  for (int d = 0; d < ndir; d++) {
    const int dx = d == 0 ? -1 : (d == 1 ? 0 : (d == 2 ? -1 : 1)), dy = d == 0 ? 0 : -1;
    const int qx = gx + dx, qy = gy + dy;
    if (qx < 0 || qx >= w || qy < 0) continue;
    if (qx / kTW == tx && qy / kTH == ty) continue;   // the same tile: joined in LDS
    const int q = (int)((long)qy * w + qx);
    if (uf_load<AG>(parent, q) < 0) continue;
    uf_unite<AG>(parent, p, q);
  }
}

// phase 3: a block is 1024 consecutive linear indices, four per thread.  No union runs any more, so
// a find ends at the component's final root; the pixel then points at it directly (an atomic minimum:
// parents only ever decrease, and whoever walks through this pixel meanwhile meets an ancestor either
// way), which shortens the chains the later workgroups walk.  labels <- the root (-1 for
// background), counts[block] <- the number of roots among the block's pixels.
__global__ void __launch_bounds__(kSpotThreads)
label_flatten_kernel(int* __restrict__ parent, long npx, int w, int* __restrict__ labels, long label_pitch,
                     int* __restrict__ counts) {
  constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;
  __shared__ int lds[kSpotThreads];
  const long i0 = (long)blockIdx.x * kTilePx + threadIdx.x * 4;
  int c = 0;
  for (int k = 0; k < 4; k++) {
    const long i = i0 + k;
    if (i >= npx) break;
    int r = -1;
    if (uf_load<AG>(parent, (int)i) >= 0) {
      r = uf_find<AG>(parent, (int)i);
      if (r != (int)i) __hip_atomic_fetch_min(parent + i, r, __ATOMIC_RELAXED, AG);
    }
    const long y = i / w;
    labels[y * label_pitch + (i - y * w)] = r;
    c += r == (int)i;
  }
  c = block_merge<kSpotThreads>(c, lds);
  if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

// phase 4: one workgroup.  counts[b] <- the sum of the counts before b; *total <- n.
__global__ void __launch_bounds__(kSpotThreads)
label_scan_kernel(int* __restrict__ counts, int n_blocks, int* __restrict__ total) {
  __shared__ int lds[kSpotThreads];
  const int t = threadIdx.x;
  const int chunk = (n_blocks + kSpotThreads - 1) / kSpotThreads;
  const int b0 = min(t * chunk, n_blocks), b1 = min(b0 + chunk, n_blocks);
  int s = 0;
  for (int b = b0; b < b1; b++) s += counts[b];
  lds[t] = s;
  __syncthreads();
  for (int d = 1; d < kSpotThreads; d <<= 1) {   // inclusive scan over the threads' sums
    const int v = t >= d ? lds[t - d] : 0;
    __syncthreads();
    lds[t] += v;
    __syncthreads();
  }
  int run = lds[t] - s;
  for (int b = b0; b < b1; b++) {
    const int c = counts[b];
    counts[b] = run;
    run += c;
  }
  if (t == kSpotThreads - 1) *total = lds[t];
}

// phase 5: the roots of a block, in index order, get offset + 1, + 2, ...; parent[root] <- -1 - number
// (<= -2: a background parent stays -1).  Only root entries are written and nobody reads parent here.
__global__ void __launch_bounds__(kSpotThreads)
label_number_kernel(int* __restrict__ parent, const int* __restrict__ labels, long label_pitch, long npx, int w,
                    const int* __restrict__ offsets) {
  __shared__ int lds[kSpotThreads];
  const int t = threadIdx.x;
  const long i0 = (long)blockIdx.x * kTilePx + t * 4;
  bool root[4];
  int c = 0;
  for (int k = 0; k < 4; k++) {
    const long i = i0 + k;
    root[k] = false;
    if (i >= npx) continue;
    const long y = i / w;
    root[k] = labels[y * label_pitch + (i - y * w)] == (int)i;
    c += root[k];
  }
  lds[t] = c;
  __syncthreads();
  for (int d = 1; d < kSpotThreads; d <<= 1) {
    const int v = t >= d ? lds[t - d] : 0;
    __syncthreads();
    lds[t] += v;
    __syncthreads();
  }
  int num = offsets[blockIdx.x] + lds[t] - c + 1;
  for (int k = 0; k < 4; k++)
    if (root[k]) parent[i0 + k] = -1 - num++;
}

// phase 6
__global__ void __launch_bounds__(kSpotThreads)
label_write_kernel(const int* __restrict__ parent, int h, int w, int tiles_x, int* __restrict__ labels,
                   long label_pitch) {
  int x, y;
  if (!tile_px(tiles_x, h, w, x, y)) return;
  const int r = labels[(long)y * label_pitch + x];
  labels[(long)y * label_pitch + x] = r < 0 ? 0 : -1 - parent[r];
}

// ---------------------------------------------------------------- sizes
// sizes[L - 1] += the pixels of label L.  A wave takes 64 consecutive pixels of a row at a time and
// retires them label by label: a ballot finds the lanes that share the first pending lane's label
// and their count goes out as ONE add.  A label that holds a quarter of the wave's pixels or more
// is kept in registers over the wave's whole share of the frame, so a frame-filling component - or
// the giant component of a dense random field - costs one add per wave, not one per pixel.
// Integer adds: exact in any order.
__global__ void __launch_bounds__(kSpotThreads)
label_sizes_kernel(const int* __restrict__ labels, int h, int w, long pitch, int n,
                   unsigned long long* __restrict__ sizes) {
  const int lane = threadIdx.x & 63;
  const long upr = (w + 63) / 64, units = (long)h * upr;
  const long n_waves = (long)gridDim.x * (kSpotThreads >> 6);
  int cur_label = 0;                // the wave's kept label and its count: the same in every lane
  unsigned long long cur = 0;
  for (long u = ((long)blockIdx.x * kSpotThreads + threadIdx.x) >> 6; u < units; u += n_waves) {
    const long y = u / upr;
    const int x = (int)(u - y * upr) * 64 + lane;
    int l = x < w ? labels[y * pitch + x] : 0;
    if (l < 0 || l > n) l = 0;      // a label beyond the caller's count is not counted
    unsigned long long pending = __ballot(l != 0);
    // every pass retires the lanes of one label: at most 64 passes, and nobody else is waited for
    while (pending) {
      const int leader = __ffsll(pending) - 1;
      const int lf = __shfl(l, leader);
      const unsigned long long mine = __ballot(l == lf);
      const unsigned long long total = (unsigned long long)__popcll(mine);
      if (lf == cur_label) {
        cur += total;
      } else if (total >= 16) {
        if (lane == 0 && cur) atomicAdd(&sizes[cur_label - 1], cur);
        cur_label = lf;
        cur = total;
      } else if (lane == leader) {
        atomicAdd(&sizes[lf - 1], total);
      }
      pending &= ~mine;
    }
  }
  if (lane == 0 && cur) atomicAdd(&sizes[cur_label - 1], cur);
}

// ---------------------------------------------------------------- largest component
struct Best {
  long long size;
  int label;   // 0: none
};
// the larger size; on a tie the lower label (np.argmax's first maximum)
__device__ inline Best merge(const Best& a, const Best& b) {
  if (b.label == 0) return a;
  if (a.label == 0) return b;
  return (b.size > a.size || (b.size == a.size && b.label < a.label)) ? b : a;
}

__global__ void __launch_bounds__(kSpotThreads)
largest_kernel(const unsigned long long* __restrict__ sizes, int n, Best* __restrict__ part) {
  __shared__ Best lds[kSpotThreads];
  Best m = {0, 0};
  for (long i = (long)blockIdx.x * kSpotThreads + threadIdx.x; i < n; i += (long)gridDim.x * kSpotThreads)
    m = merge(m, Best{(long long)sizes[i], (int)i + 1});
  m = block_merge<kSpotThreads>(m, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = m;
}

// res = {label, size, sum_y, sum_x} as int64; the two sums start at 0 for the next kernel
__global__ void __launch_bounds__(kSpotThreads)
largest_final(const Best* __restrict__ part, int n_part, long long* __restrict__ res) {
  __shared__ Best lds[kSpotThreads];
  const Best m = merge_partials<kSpotThreads>(part, n_part, {0, 0}, lds);
  if (threadIdx.x != 0) return;
  res[0] = m.label;
  res[1] = m.size;
  res[2] = 0;
  res[3] = 0;
}

struct CoordSum {
  unsigned long long y, x;
};
__device__ inline CoordSum merge(const CoordSum& a, const CoordSum& b) { return {a.y + b.y, a.x + b.x}; }

// the integer coordinate sums of the pixels of label res[0]: per workgroup in LDS, then one add
__global__ void __launch_bounds__(kSpotThreads)
coord_sum_kernel(const int* __restrict__ labels, int h, int w, long pitch, long long* __restrict__ res) {
  __shared__ CoordSum lds[kSpotThreads];
  const int label = (int)res[0];
  const long upr = (w + kSpotThreads - 1) / kSpotThreads, units = (long)h * upr;
  CoordSum m = {0, 0};
  for (long u = blockIdx.x; u < units; u += gridDim.x) {
    const long y = u / upr;
    const int x = (int)(u - y * upr) * kSpotThreads + threadIdx.x;
    if (x < w && labels[y * pitch + x] == label) {
      m.y += (unsigned long long)y;
      m.x += (unsigned long long)x;
    }
  }
  m = block_merge<kSpotThreads>(m, lds);
  if (threadIdx.x == 0 && (m.y | m.x)) {
    atomicAdd((unsigned long long*)&res[2], m.y);
    atomicAdd((unsigned long long*)&res[3], m.x);
  }
}

// ---------------------------------------------------------------- take
struct Take {
  double sum, mx;
  unsigned long long n, nan;
};
__device__ inline Take merge(const Take& a, const Take& b) {
  return {a.sum + b.sum, b.mx > a.mx ? b.mx : a.mx, a.n + b.n, a.nan + b.nan};
}

// The pixels of `label` (labels != NULL) or the whole rows row[0], row[1] (n_rows of them):
// fit[p] = frame[p] - bg, mask[p] = 1; the partial {sum, max, count} of the workgroup.  A unit is
// 256 consecutive pixels of one row and the grid depends on the frame's size alone: the sum is
// added in one fixed order.
template <typename T>
__global__ void __launch_bounds__(kSpotThreads)
spot_take_kernel(SpotSrc s, int h, int w, const int* __restrict__ labels, long label_pitch, int label, int row_a,
                 int row_b, int n_rows, double* __restrict__ fit, long fit_pitch, unsigned char* __restrict__ mask,
                 long mask_pitch, Take* __restrict__ part) {
  __shared__ Take lds[kSpotThreads];
  const long upr = (w + kSpotThreads - 1) / kSpotThreads, units = (long)(labels ? h : n_rows) * upr;
  Take m = {0.0, -__builtin_inf(), 0, 0};
  for (long u = blockIdx.x; u < units; u += gridDim.x) {
    const long k = u / upr;
    const int x = (int)(u - k * upr) * kSpotThreads + threadIdx.x;
    const int y = labels ? (int)k : (k == 0 ? row_a : row_b);
    if (x >= w || (labels && labels[(long)y * label_pitch + x] != label)) continue;
    const double v = src_px<T>(s, y, x);
    fit[(long)y * fit_pitch + x] = v;
    mask[(long)y * mask_pitch + x] = 1;
    m.n++;
    m.sum += v;
    if (v != v) m.nan++;
    else m.mx = v > m.mx ? v : m.mx;
  }
  m = block_merge<kSpotThreads>(m, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = m;
}

// res = {max (NaN if any value is, as np.max), sum, count}
__global__ void __launch_bounds__(kSpotThreads)
spot_take_final(const Take* __restrict__ part, int n_part, double* __restrict__ res) {
  __shared__ Take lds[kSpotThreads];
  const Take m = merge_partials<kSpotThreads>(part, n_part, {0.0, -__builtin_inf(), 0, 0}, lds);
  if (threadIdx.x != 0) return;
  res[0] = m.nan ? __builtin_nan("") : m.mx;
  res[1] = m.sum;
  res[2] = (double)m.n;
}

// ---------------------------------------------------------------- host side
// workgroups of a grid-stride launch: what the work needs, at most kSpotMaxGrid - the frame's size
// alone decides, so that a fixed-order sum has the same order on every device
int stride_grid(long needed) {
  const long g = needed < kSpotMaxGrid ? needed : kSpotMaxGrid;
  return (int)(g > 1 ? g : 1);
}

// the checks of the calls that read a frame minus its background
int check_src(ipa_ctx* ctx, const char* what, const void* d_img, int dtype, int h, int w, long pitch,
              const double* d_bg, long bg_pitch) {
  IPA_REQUIRE(ctx, d_img, "%s: null image", what);
  IPA_REQUIRE(ctx, h > 0 && w > 0, "%s: empty image", what);
  IPA_REQUIRE(ctx, (long)h * w <= kSpotMaxPixels, "%s: 2^31 pixels or more", what);
  IPA_REQUIRE(ctx, pitch >= w && (!d_bg || bg_pitch >= w), "%s: pitch smaller than width", what);
  if (!known_dtype(dtype))
    IPA_UNSUPPORTED(ctx, "%s: frames are uint8 / uint16 / float32 / float64 (got dtype %d)", what, dtype);
  return IPA_OK;
}

int check_labels(ipa_ctx* ctx, const char* what, const int* d_labels, int h, int w, long pitch) {
  IPA_REQUIRE(ctx, d_labels, "%s: null labels", what);
  IPA_REQUIRE(ctx, h > 0 && w > 0, "%s: empty image", what);
  IPA_REQUIRE(ctx, (long)h * w <= kSpotMaxPixels, "%s: 2^31 pixels or more", what);
  IPA_REQUIRE(ctx, pitch >= w, "%s: pitch smaller than width", what);
  return IPA_OK;
}

int sizes_call(ipa_ctx* ctx, const int* d_labels, int h, int w, long pitch, int n, unsigned long long* d_sizes) {
  IPA_HIP(ctx, hipSetDevice(ctx->device));
  IPA_HIP(ctx, hipMemsetAsync(d_sizes, 0, (size_t)n * 8, ctx->stream));
  const long units = (long)h * ((w + 63) / 64), waves = kSpotThreads / 64;
  return launch(ctx, label_sizes_kernel, dim3(stride_grid((units + waves - 1) / waves)), dim3(kSpotThreads), 0,
                d_labels, h, w, pitch, n, d_sizes);
}

}  // namespace
}  // namespace ipa

using namespace ipa;

extern "C" {

int ipa_spot_range_dev(ipa_ctx* ctx, const void* d_img, int dtype, int h, int w, long pitch, const double* d_bg,
                       long bg_pitch, double bg, double* range) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  int rc = check_src(ctx, "spot_range", d_img, dtype, h, w, pitch, d_bg, bg_pitch);
  if (rc) return rc;
  IPA_REQUIRE(ctx, range, "spot_range: null result");
  const long units = (long)h * ((w + kSpotThreads - 1) / kSpotThreads);
  const int grid = stride_grid(units);
  Range* part;
  double* res;
  rc = stage_ws(ctx, slot(&part, grid), slot(&res, 5));
  if (rc) return rc;
  const SpotSrc src = {d_img, d_bg, pitch, bg_pitch, bg};
  rc = by_dtype(dtype, [&](auto e) {
    using T = decltype(e);
    const int r = launch(ctx, spot_range_kernel<T>, dim3(grid), dim3(kSpotThreads), 0, src, h, w, part);
    if (r) return r;
    return launch(ctx, spot_range_final<T>, dim3(1), dim3(kSpotThreads), 0, src, part, grid, res);
  });
  if (rc) return rc;
  return ipa_stage_out(ctx, {{range, res, 5 * sizeof(double)}});
}

int ipa_spot_histogram_dev(ipa_ctx* ctx, const void* d_img, int dtype, int h, int w, long pitch, const double* d_bg,
                           long bg_pitch, double bg, const double* edges, int nbins, unsigned long long* counts) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  if (nbins > kSpotMaxBins) IPA_UNSUPPORTED(ctx, "spot_histogram: at most %d bins (got %d)", kSpotMaxBins, nbins);
  int rc = check_src(ctx, "spot_histogram", d_img, dtype, h, w, pitch, d_bg, bg_pitch);
  if (rc) return rc;
  IPA_REQUIRE(ctx, edges && counts && nbins >= 1, "spot_histogram: null table or no bins");
  IPA_REQUIRE(ctx, edges[nbins] > edges[0], "spot_histogram: the last edge must lie above the first");
  const double norm = (double)nbins / (edges[nbins] - edges[0]);
  const size_t lds = (size_t)(nbins + 1) * 8 + (size_t)(kSpotThreads / 64) * nbins * 4;
  const long nruns = (long)h * ((w + kRun - 1) / kRun);
  const int grid = stride_grid((nruns + kSpotThreads - 1) / kSpotThreads);
  double* d_edges;
  unsigned long long* d_cnt;
  unsigned* d_slab;
  rc = stage_ws(ctx, slot(&d_edges, nbins + 1, edges), slot(&d_cnt, nbins), slot(&d_slab, (size_t)grid * nbins));
  if (rc) return rc;
  const SpotSrc src = {d_img, d_bg, pitch, bg_pitch, bg};
  rc = by_dtype(dtype, [&](auto e) {
    return launch(ctx, spot_hist_kernel<decltype(e)>, dim3(grid), dim3(kSpotThreads), lds, src, h, w, d_edges, nbins,
                  norm, d_slab);
  });
  if (rc) return rc;
  rc = launch(ctx, spot_hist_final, dim3((nbins + kSpotThreads - 1) / kSpotThreads), dim3(kSpotThreads), 0,
              d_slab, grid, nbins, d_cnt);
  if (rc) return rc;
  return ipa_stage_out(ctx, {{counts, d_cnt, (size_t)nbins * 8}});
}

int ipa_spot_mask_dev(ipa_ctx* ctx, const void* d_img, int dtype, int h, int w, long pitch, const double* d_bg,
                      long bg_pitch, double bg, double t, unsigned char* d_mask, long mask_pitch) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  int rc = check_src(ctx, "spot_mask", d_img, dtype, h, w, pitch, d_bg, bg_pitch);
  if (rc) return rc;
  IPA_REQUIRE(ctx, d_mask && mask_pitch >= w, "spot_mask: null mask or pitch smaller than width");
  const Span spans[] = {span2d(d_mask, h, w, mask_pitch, 1), span2d(d_img, h, w, pitch, ipa_dtype_size(dtype)),
                        span2d(d_bg, h, w, bg_pitch, 8)};
  IPA_REQUIRE(ctx, !written_overlaps(spans, 1), "spot_mask does not run in place");
  int tiles_x;
  unsigned grid;
  rc = frame_args(ctx, "spot_mask", h, w, &tiles_x, &grid);
  if (rc) return rc;
  const SpotSrc src = {d_img, d_bg, pitch, bg_pitch, bg};
  return by_dtype(dtype, [&](auto e) {
    return launch(ctx, spot_mask_kernel<decltype(e)>, dim3(grid), dim3(kSpotThreads), 0, src, h, w, tiles_x, t, d_mask,
                  mask_pitch);
  });
}

int ipa_label_dev(ipa_ctx* ctx, const unsigned char* d_mask, int h, int w, long mask_pitch, int connectivity,
                  int* d_labels, long label_pitch, int* n) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  IPA_REQUIRE(ctx, d_mask && n, "label: null pointer");
  int rc = check_labels(ctx, "label", d_labels, h, w, label_pitch);
  if (rc) return rc;
  IPA_REQUIRE(ctx, mask_pitch >= w, "label: pitch smaller than width");
  IPA_REQUIRE(ctx, connectivity == 1 || connectivity == 2, "label: connectivity is 1 or 2 (got %d)", connectivity);
  IPA_REQUIRE(ctx, !overlap(span2d(d_labels, h, w, label_pitch, 4), span2d(d_mask, h, w, mask_pitch, 1)),
              "label: the labels overlap the mask");
  const long npx = (long)h * w;
  const int tiles_x = (w + kTW - 1) / kTW, tiles = tiles_x * ((h + kTH - 1) / kTH);
  const int n_blocks = (int)((npx + kTilePx - 1) / kTilePx);
  int *parent, *counts, *d_n;
  rc = stage_ws(ctx, slot(&parent, npx), slot(&counts, n_blocks), slot(&d_n, 1));
  if (rc) return rc;
  const int conn8 = connectivity == 2;
  rc = launch(ctx, label_tile_kernel, dim3(tiles), dim3(kSpotThreads), 0, d_mask, h, w, mask_pitch, tiles_x, conn8,
              parent);
  if (rc) return rc;
  rc = launch(ctx, label_seam_kernel, dim3(tiles), dim3(kSeamThreads), 0, parent, h, w, tiles_x, conn8);
  if (rc) return rc;
  rc = launch(ctx, label_flatten_kernel, dim3(n_blocks), dim3(kSpotThreads), 0, parent, npx, w, d_labels, label_pitch,
              counts);
  if (rc) return rc;
  rc = launch(ctx, label_scan_kernel, dim3(1), dim3(kSpotThreads), 0, counts, n_blocks, d_n);
  if (rc) return rc;
  rc = launch(ctx, label_number_kernel, dim3(n_blocks), dim3(kSpotThreads), 0, parent, d_labels, label_pitch, npx, w,
              counts);
  if (rc) return rc;
  int tx;
  unsigned grid;
  rc = frame_args(ctx, "label", h, w, &tx, &grid);
  if (rc) return rc;
  rc = launch(ctx, label_write_kernel, dim3(grid), dim3(kSpotThreads), 0, parent, h, w, tx, d_labels, label_pitch);
  if (rc) return rc;
  return ipa_stage_out(ctx, {{n, d_n, sizeof(int)}});
}

int ipa_label_sizes_dev(ipa_ctx* ctx, const int* d_labels, int h, int w, long label_pitch, int n,
                        long long* d_sizes) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  const int rc = check_labels(ctx, "label_sizes", d_labels, h, w, label_pitch);
  if (rc) return rc;
  IPA_REQUIRE(ctx, n >= 0 && (n == 0 || d_sizes), "label_sizes: null sizes or a negative count");
  if (n == 0) return IPA_OK;
  IPA_REQUIRE(ctx, !overlap(span2d(d_labels, h, w, label_pitch, 4), Span{d_sizes, (size_t)n * 8}),
              "label_sizes: the sizes overlap the labels");
  return sizes_call(ctx, d_labels, h, w, label_pitch, n, (unsigned long long*)d_sizes);
}

int ipa_label_largest_dev(ipa_ctx* ctx, const int* d_labels, int h, int w, long label_pitch, int n,
                          long long* result) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  int rc = check_labels(ctx, "label_largest", d_labels, h, w, label_pitch);
  if (rc) return rc;
  IPA_REQUIRE(ctx, result && n >= 0, "label_largest: null result or a negative count");
  if (n == 0) {
    result[0] = result[1] = result[2] = result[3] = 0;
    return IPA_OK;
  }
  const int grid = stride_grid(((long)n + kSpotThreads - 1) / kSpotThreads);
  unsigned long long* sizes;
  Best* d_part;
  long long* d_res;
  rc = stage_ws(ctx, slot(&sizes, n), slot(&d_part, grid), slot(&d_res, 4));
  if (rc) return rc;
  rc = sizes_call(ctx, d_labels, h, w, label_pitch, n, sizes);
  if (rc) return rc;
  rc = launch(ctx, largest_kernel, dim3(grid), dim3(kSpotThreads), 0, sizes, n, d_part);
  if (rc) return rc;
  rc = launch(ctx, largest_final, dim3(1), dim3(kSpotThreads), 0, d_part, grid, d_res);
  if (rc) return rc;
  const long units = (long)h * ((w + kSpotThreads - 1) / kSpotThreads);
  rc = launch(ctx, coord_sum_kernel, dim3(stride_grid(units)), dim3(kSpotThreads), 0, d_labels, h, w, label_pitch,
              d_res);
  if (rc) return rc;
  return ipa_stage_out(ctx, {{result, d_res, 4 * sizeof(long long)}});
}

int ipa_spot_take_dev(ipa_ctx* ctx, const void* d_img, int dtype, int h, int w, long pitch, const double* d_bg,
                      long bg_pitch, double bg, const int* d_labels, long label_pitch, int label, int row_a,
                      int row_b, double* d_fit, long fit_pitch, unsigned char* d_mask, long mask_pitch,
                      double* result) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  int rc = check_src(ctx, "spot_take", d_img, dtype, h, w, pitch, d_bg, bg_pitch);
  if (rc) return rc;
  IPA_REQUIRE(ctx, d_fit && d_mask && result, "spot_take: null pointer");
  IPA_REQUIRE(ctx, fit_pitch >= w && mask_pitch >= w && (!d_labels || label_pitch >= w),
              "spot_take: pitch smaller than width");
  if (d_labels)
    IPA_REQUIRE(ctx, label >= 1, "spot_take: labels start at 1 (got %d)", label);
  else
    IPA_REQUIRE(ctx, row_a >= 0 && row_a < h && row_b >= 0 && row_b < h,
                "spot_take: rows %d and %d of a frame of %d rows", row_a, row_b, h);
  const Span spans[] = {span2d(d_fit, h, w, fit_pitch, 8),
                        span2d(d_mask, h, w, mask_pitch, 1),
                        span2d(d_img, h, w, pitch, ipa_dtype_size(dtype)),
                        span2d(d_bg, h, w, bg_pitch, 8),
                        span2d(d_labels, h, w, label_pitch, 4)};
  IPA_REQUIRE(ctx, !written_overlaps(spans, 2), "spot_take: an output overlaps another array");
  const int n_rows = row_a == row_b ? 1 : 2;
  const long units = (long)(d_labels ? h : n_rows) * ((w + kSpotThreads - 1) / kSpotThreads);
  const int grid = stride_grid(units);
  Take* part;
  double* res;
  rc = stage_ws(ctx, slot(&part, grid), slot(&res, 3));
  if (rc) return rc;
  const SpotSrc src = {d_img, d_bg, pitch, bg_pitch, bg};
  rc = by_dtype(dtype, [&](auto e) {
    return launch(ctx, spot_take_kernel<decltype(e)>, dim3(grid), dim3(kSpotThreads), 0, src, h, w, d_labels,
                  label_pitch, label, row_a, row_b, n_rows, d_fit, fit_pitch, d_mask, mask_pitch, part);
  });
  if (rc) return rc;
  rc = launch(ctx, spot_take_final, dim3(1), dim3(kSpotThreads), 0, part, grid, res);
  if (rc) return rc;
  return ipa_stage_out(ctx, {{result, res, 3 * sizeof(double)}});
}

}  // extern "C"
