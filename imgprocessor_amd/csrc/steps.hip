// steps.hip — the flat field from discrete steps on gfx950: what camera/flatField/vignettingFromDiscreteSteps.py
// ("Method D" with known device positions) does before its post-processing.
//   ipa_cell_means_dev       :228-246  the thresholded mean of every grid cell of every frame
//                                      (array/subCell2D.py: subCell2DFnArray with the cell function of :228-234)
//   ipa_steps_separate_dev   :257-281, :316  the iterative separation of device and flat field on the cell grid
//   ipa_offset_meshgrid_dev  interpolate/offsetMeshgrid.py:18-27  the two coordinate arrays of the rescale
//   ipa_isnan_mask_dev       :289  np.isnan(ff) as a uint8 mask
//
// Cell means.  A workgroup owns one row segment: up to kCellSegRows rows of one cell row of one frame, over the
// whole width of the grid.  It walks that strip in chunks of 256 columns that start at multiples of 256 ELEMENTS
// of the row, whatever column the first cell starts at: lane t reads column x0 + t of every row, so a wave reads
// 64 adjacent elements of a row per load and the loads of a chunk are as aligned as the row itself is.  A lane
// sums its column over the segment's rows serially (at most 32 terms), then the 256 column sums are added per
// cell by a segmented Hillis-Steele scan in LDS - a fixed tree - and the lane on a cell's last column stores the
// cell's partial sum and count; a cell wider than a chunk carries its running partial from chunk to chunk, left to
// right.  A second launch adds a cell's row segments top to bottom and takes the mean.  Every frame element is
// read once, nothing of frame size is written, no atomics: two calls give identical bits.
//
// The separation loop is one launch of one workgroup: a lane owns device cells in one phase and grid cells in the
// next, barriers between the phases, the flat field and the object in LDS where they fit (a workspace otherwise).
// Lane 0 forms the deviation and the stop decision, every lane reads it from one LDS word after a barrier.
//
// Everything is float64, every division IEEE, nothing fused (Makefile + pragma).
#include "common.hpp"
#include "frame_args.hpp"
#include "launch.hpp"
#include "reduce.hpp"

#include <math.h>
#include <string.h>

#include <vector>

#pragma clang fp contract(off)

namespace ipa {
namespace {

constexpr int kStepsMaxN = 64;
constexpr int kCellThreads = 256;
constexpr int kCellSegRows = 32;          // rows of a row segment: a lane's serial run
constexpr long kCellMaxParts = 1L << 24;  // frames * cell rows * segments per cell row * cell columns
constexpr int kSepThreads = 256;
constexpr int kSepLds = 6144;             // doubles of LDS for the flat field and the object (48 KiB)
constexpr int kSepMaxCells = 1 << 16;     // grid cells, and device cells, of the separation loop
constexpr int kSepMaxIter = 10000;
constexpr int kTileThreads = 256;

// ---- (a) partial sums of one row segment ------------------------------------------------------------------------
template <typename E, typename B, bool HasBg>
__global__ void __launch_bounds__(kCellThreads)
cell_partials_kernel(const E* __restrict__ frames, long pitch, long stride, const B* __restrict__ bg, long bg_pitch,
                     double thresh, const int* __restrict__ row_edges, const int* __restrict__ col_edges, int g0,
                     int g1, int segs, double* __restrict__ part_sum, int* __restrict__ part_cnt) {
  __shared__ double s_sum[2][kCellThreads];
  __shared__ int s_cnt[2][kCellThreads];
  __shared__ double s_carry_sum;
  __shared__ int s_carry_cnt;
  const int t = threadIdx.x;
  unsigned b = blockIdx.x;
  const int s = (int)(b % (unsigned)segs);
  b /= (unsigned)segs;
  const int i = (int)(b % (unsigned)g0);
  const int n = (int)(b / (unsigned)g0);
  const int r0 = row_edges[i] + s * kCellSegRows;
  const int r_end = row_edges[i + 1];
  const int c_begin = col_edges[0], c_end = col_edges[g1];
  if (r0 >= r_end || c_begin >= c_end) return;   // uniform: before any barrier
  const int r1 = r0 + kCellSegRows < r_end ? r0 + kCellSegRows : r_end;
  const E* f = frames + (long)n * stride;
  const long out = ((long)(n * g0 + i) * segs + s) * g1;
  if (t == 0) {
    s_carry_sum = 0.0;
    s_carry_cnt = 0;
  }
  for (int x0 = c_begin & ~(kCellThreads - 1); x0 < c_end; x0 += kCellThreads) {
    const int x = x0 + t;
    const bool in = x >= c_begin && x < c_end;
    double sum = 0.0;
    int cnt = 0;
    int j = 0, cs = x, ce = x + 1;   // a lane outside the grid is a segment of its own, worth 0
    if (in) {
      int lo = 0, hi = g1;           // col_edges[lo] <= x < col_edges[hi]: the one non-empty cell that holds x
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (col_edges[mid] <= x) lo = mid;
        else hi = mid;
      }
      j = lo;
      cs = col_edges[lo];
      ce = col_edges[lo + 1];
      const E* p = f + (long)r0 * pitch + x;
      const B* q = HasBg ? bg + (long)r0 * bg_pitch + x : nullptr;
#pragma unroll 8
      for (int r = r0; r < r1; r++) {
        double v = (double)*p;
        p += pitch;
        if (HasBg) {
          v -= (double)*q;
          q += bg_pitch;
        }
        if (v > thresh) {   // a NaN is no sample
          sum += v;
          cnt++;
        }
      }
    }
    // segmented inclusive scan over the chunk's 256 column sums: lane t gathers the lanes of its cell to its left
    const int seg0 = cs > x0 ? cs - x0 : 0;
    int cur = 0;
    s_sum[0][t] = sum;
    s_cnt[0][t] = cnt;
    __syncthreads();
    for (int d = 1; d < kCellThreads; d <<= 1) {
      if (t - d >= seg0) {
        sum = s_sum[cur][t - d] + sum;
        cnt = s_cnt[cur][t - d] + cnt;
      }
      cur ^= 1;
      s_sum[cur][t] = sum;
      s_cnt[cur][t] = cnt;
      __syncthreads();
    }
    const bool cont = in && cs < x0;   // the cell began in an earlier chunk: its partial so far is the carry
    if (cont) {
      sum = s_carry_sum + sum;
      cnt = s_carry_cnt + cnt;
    }
    if (in && x + 1 == ce) {
      part_sum[out + j] = sum;
      part_cnt[out + j] = cnt;
    }
    __syncthreads();                   // every lane has read the carry
    if (t == kCellThreads - 1 && in && x + 1 < ce) {
      s_carry_sum = sum;
      s_carry_cnt = cnt;
    }
    // the scan's barriers of the next chunk stand between this store and the next read of the carry
  }
}

// ---- (b) a cell's row segments, top to bottom, and the mean ------------------------------------------------------
__global__ void __launch_bounds__(kCellThreads)
cell_finish_kernel(const double* __restrict__ part_sum, const int* __restrict__ part_cnt,
                   const int* __restrict__ row_edges, const int* __restrict__ col_edges, long cells, int g0, int g1,
                   int segs, double* __restrict__ grid) {
  const long idx = (long)blockIdx.x * kCellThreads + threadIdx.x;
  if (idx >= cells) return;
  const int j = (int)(idx % g1);
  const long ni = idx / g1;          // n * g0 + i
  const int i = (int)(ni % g0);
  const int rows = row_edges[i + 1] - row_edges[i], cols = col_edges[j + 1] - col_edges[j];
  const long size = (long)rows * cols;
  double v = (double)NAN;
  if (size > 0) {
    const int ns = (rows + kCellSegRows - 1) / kCellSegRows;
    const long base = ni * segs * g1 + j;
    double sum = part_sum[base];
    long cnt = part_cnt[base];
    for (int s = 1; s < ns; s++) {
      sum += part_sum[base + (long)s * g1];
      cnt += part_cnt[base + (long)s * g1];
    }
    if (2 * cnt >= size) v = sum / (double)cnt;   // "majority is background" -> NaN
  }
  grid[idx] = v;
}

// ---- (c) the separation loop --------------------------------------------------------------------------------------
struct StepRect {
  int q0, q1, qq0, qq1, l0, l1;   // device rows / columns from q, grid rows / columns from qq, l0 x l1 cells
};

// np.nanmean(axis=0) one term at a time: NaN -> 0, a sum in frame order that STARTS with the first term
__device__ __forceinline__ void nan_term(double v, int k, double& acc, int& cnt) {
  const bool isn = v != v;
  const double z = isn ? 0.0 : v;
  acc = k == 0 ? z : acc + z;
  cnt += isn ? 0 : 1;
}

// the initial flat field's maximum as reduce.hpp merges it
struct NanMax {
  double v;
};
__device__ inline NanMax merge(NanMax a, NanMax b) { return {fmax(a.v, b.v)}; }

__global__ void __launch_bounds__(kSepThreads)
steps_separate_kernel(const double* __restrict__ grid, int n, int g0, int g1, int n0, int n1,
                      const int* __restrict__ rects, double bg_value, int subtract_bg, int max_iter, double max_dev,
                      double* ws, double* __restrict__ ff_out, double* __restrict__ avg_out,
                      int* __restrict__ density, int* __restrict__ iter_out, double* __restrict__ dev_out) {
  __shared__ double s_arr[kSepLds];
  __shared__ double s_red[kSepThreads];
  __shared__ int s_redc[kSepThreads];
  __shared__ int s_rect[kStepsMaxN * 6];
  __shared__ int s_stop;
  __shared__ double s_dev;
  const int t = threadIdx.x;
  const int G = g0 * g1, D = n0 * n1;
  double* ff = ws ? ws : s_arr;
  double* avg = ff + G;
  for (int k = t; k < n * 6; k += kSepThreads) s_rect[k] = rects[k];

  // :258-261 the initial flat field, and :316 the point density
  double mx = (double)NAN;
  for (int c = t; c < G; c += kSepThreads) {
    double acc = 0.0;
    int cnt = 0;
    for (int k = 0; k < n; k++) nan_term(grid[(long)k * G + c], k, acc, cnt);
    double m = acc / (double)cnt;
    if (subtract_bg) m -= bg_value;
    ff[c] = m;
    density[c] = cnt;
    mx = fmax(mx, m);   // np.nanmax: a NaN only where nothing else is
  }
  mx = block_merge<kSepThreads>(NanMax{mx}, (NanMax*)s_red).v;
  for (int c = t; c < G; c += kSepThreads) ff[c] = ff[c] / mx;
  __syncthreads();

  int iter = 0;
  for (;;) {
    iter++;
    // :269-271 the object: per device cell the mean over the frames of device / flat field
    for (int c = t; c < D; c += kSepThreads) {
      const int a = c / n1, b = c - a * n1;
      double acc = 0.0;
      int cnt = 0;
      for (int k = 0; k < n; k++) {
        const int* r = s_rect + k * 6;
        const int da = a - r[0], db = b - r[1];
        double o = (double)NAN;
        if (da >= 0 && da < r[4] && db >= 0 && db < r[5]) {
          const int gc = (r[2] + da) * g1 + r[3] + db;
          o = grid[(long)k * G + gc] / ff[gc];
        }
        nan_term(o, k, acc, cnt);
      }
      avg[c] = acc / (double)cnt;
    }
    __syncthreads();
    // :273-277 the next flat field: per grid cell the mean over the frames of device / object
    double ssq = 0.0;
    int sc = 0;
    for (int c = t; c < G; c += kSepThreads) {
      const int y = c / g1, x = c - y * g1;
      double acc = 0.0;
      int cnt = 0;
      for (int k = 0; k < n; k++) {
        const int* r = s_rect + k * 6;
        const int dy = y - r[2], dx = x - r[3];
        double v = (double)NAN;
        if (dy >= 0 && dy < r[4] && dx >= 0 && dx < r[5])
          v = grid[(long)k * G + c] / avg[(r[0] + dy) * n1 + r[1] + dx];
        nan_term(v, k, acc, cnt);
      }
      const double f2 = acc / (double)cnt;
      const double df = ff[c] - f2;
      const double sq = df * df;
      if (sq == sq) {
        ssq += sq;
        sc++;
      }
      ff[c] = f2;   // only this lane reads ff[c] in this phase
    }
    // block_merge's tree, written out on two arrays: one {sum, count} struct pads to 16 bytes, and with that 1 KiB
    // more of LDS a compute unit holds two of these workgroups instead of three
    s_red[t] = ssq;
    s_redc[t] = sc;
    __syncthreads();
    for (int d = kSepThreads / 2; d > 0; d >>= 1) {
      if (t < d) {
        s_red[t] = s_red[t] + s_red[t + d];
        s_redc[t] = s_redc[t] + s_redc[t + d];
      }
      __syncthreads();
    }
    if (t == 0) {
      const double dev = sqrt(s_red[0] / (double)s_redc[0]);   // RMS; 0 / 0 -> NaN runs to the cap
      s_dev = dev;
      s_stop = (dev < max_dev || iter > max_iter + 1) ? 1 : 0;
    }
    __syncthreads();
    if (s_stop) break;   // one LDS word, read after the barrier: uniform
  }
  for (int c = t; c < G; c += kSepThreads) ff_out[c] = ff[c];
  for (int c = t; c < D; c += kSepThreads) avg_out[c] = avg[c];
  if (t == 0) {
    *iter_out = iter;
    *dev_out = s_dev;
  }
}

// ---- (d) np.meshgrid(np.linspace(start1, stop1, w), np.linspace(start0, stop0, h)) ----------------------------------
template <typename T>
__global__ void __launch_bounds__(kTileThreads)
offset_meshgrid_kernel(double start0, double step0, double stop0, double start1, double step1, double stop1, int h,
                       int w, int tiles_x, T* __restrict__ yy, T* __restrict__ xx, long pitch) {
  int x, y;
  if (!tile_px(tiles_x, h, w, x, y)) return;
  const double vy = (h > 1 && y == h - 1) ? stop0 : (double)y * step0 + start0;
  const double vx = (w > 1 && x == w - 1) ? stop1 : (double)x * step1 + start1;
  yy[(long)y * pitch + x] = (T)vy;
  xx[(long)y * pitch + x] = (T)vx;
}

// ---- (e) np.isnan ------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(kTileThreads)
isnan_mask_kernel(const T* __restrict__ in, long pitch, int h, int w, int tiles_x, unsigned char* __restrict__ mask,
                  long mask_pitch) {
  int x, y;
  if (!tile_px(tiles_x, h, w, x, y)) return;
  const T v = in[(long)y * pitch + x];
  mask[(long)y * mask_pitch + x] = v != v ? 1 : 0;
}

// a table of g + 1 edges: monotone, within [0, size]
bool edges_ok(const int* e, int g, int size) {
  if (e[0] < 0 || e[g] > size) return false;
  for (int k = 0; k < g; k++)
    if (e[k] > e[k + 1]) return false;
  return true;
}

}  // namespace
}  // namespace ipa

using namespace ipa;

extern "C" {

int ipa_cell_means_dev(ipa_ctx* ctx, const void* d_frames, int dtype, int n, int h, int w, long pitch,
                       long frame_stride, const void* d_bg, int bg_dtype, long bg_pitch, double thresh,
                       const int* row_edges, int g0, const int* col_edges, int g1, double* d_grid) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  if (n > kStepsMaxN) IPA_UNSUPPORTED(ctx, "cell_means: at most %d frames (got %d)", kStepsMaxN, n);
  IPA_REQUIRE(ctx, n >= 1, "cell_means: needs at least one frame (got %d)", n);
  IPA_REQUIRE(ctx, d_frames && row_edges && col_edges && d_grid, "cell_means: null pointer");
  IPA_REQUIRE(ctx, h > 0 && w > 0, "cell_means: empty image");
  if (w >= (1 << 26)) IPA_UNSUPPORTED(ctx, "cell_means: rows of at most 2^26 - 1 elements (got %d)", w);
  IPA_REQUIRE(ctx, pitch >= w && (!d_bg || bg_pitch >= w), "cell_means: pitch smaller than width");
  IPA_REQUIRE(ctx, frame_stride >= (long)(h - 1) * pitch + w, "cell_means: frames overlap");
  if (!known_dtype(dtype) || (d_bg && !known_dtype(bg_dtype)))
    IPA_UNSUPPORTED(ctx, "cell_means: frames and background are uint8 / uint16 / float32 / float64 (got dtypes %d, %d)",
                    dtype, bg_dtype);
  IPA_REQUIRE(ctx, g0 >= 1 && g1 >= 1, "cell_means: empty grid (%d x %d)", g0, g1);
  if ((long)g0 * g1 > kCellMaxParts) IPA_UNSUPPORTED(ctx, "cell_means: at most 2^24 cells a frame (got %d x %d)", g0, g1);
  IPA_REQUIRE(ctx, edges_ok(row_edges, g0, h) && edges_ok(col_edges, g1, w),
              "cell_means: the cell edges must not decrease and must lie within the frame");
  int segs = 1;
  for (int i = 0; i < g0; i++) {
    const int ns = (row_edges[i + 1] - row_edges[i] + kCellSegRows - 1) / kCellSegRows;
    if (ns > segs) segs = ns;
  }
  const long parts = (long)n * g0 * segs * g1;
  if (parts > kCellMaxParts)
    IPA_UNSUPPORTED(ctx, "cell_means: frames * cell rows * row segments * cell columns = %ld exceeds 2^24 "
                    "(a row segment is %d rows of a cell row; the tallest cell row has %d)", parts, kCellSegRows, segs);
  const long cells = (long)n * g0 * g1;
  const Span spans[] = {span2d(d_grid, 1, cells, cells, 8),
                        span_stack(d_frames, n, h, w, pitch, frame_stride, ipa_dtype_size(dtype)),
                        span2d(d_bg, h, w, bg_pitch, d_bg ? ipa_dtype_size(bg_dtype) : 1)};
  IPA_REQUIRE(ctx, !written_overlaps(spans, 1), "cell_means: the grid overlaps an input");
  double* part_sum;
  int* part_cnt;
  int rc = stage_ws(ctx, slot(&part_sum, parts), slot(&part_cnt, parts));
  if (rc) return rc;
  // both edge tables in one upload
  std::vector<int> edges((size_t)g0 + g1 + 2);
  memcpy(edges.data(), row_edges, ((size_t)g0 + 1) * sizeof(int));
  memcpy(edges.data() + g0 + 1, col_edges, ((size_t)g1 + 1) * sizeof(int));
  void* d_edges;
  rc = ipa_tab_upload(ctx, edges.data(), edges.size() * sizeof(int), &d_edges);
  if (rc) return rc;
  const int* d_rows = (const int*)d_edges;
  const int* d_cols = d_rows + g0 + 1;
  const unsigned grid = (unsigned)((long)n * g0 * segs);
  rc = by_dtype(dtype, [&](auto e) {
    using E = decltype(e);
    if (!d_bg)
      return launch(ctx, cell_partials_kernel<E, unsigned char, false>, dim3(grid), dim3(kCellThreads), 0, d_frames,
                    pitch, frame_stride, nullptr, 0L, thresh, d_rows, d_cols, g0, g1, segs, part_sum, part_cnt);
    return by_dtype(bg_dtype, [&](auto bt) {
      using B = decltype(bt);
      return launch(ctx, cell_partials_kernel<E, B, true>, dim3(grid), dim3(kCellThreads), 0, d_frames, pitch,
                    frame_stride, d_bg, bg_pitch, thresh, d_rows, d_cols, g0, g1, segs, part_sum, part_cnt);
    });
  });
  if (rc) return rc;
  return launch(ctx, cell_finish_kernel, dim3((unsigned)((cells + kCellThreads - 1) / kCellThreads)),
                dim3(kCellThreads), 0, part_sum, part_cnt, d_rows, d_cols, cells, g0, g1, segs, d_grid);
}

int ipa_steps_separate_dev(ipa_ctx* ctx, const double* d_grid, int n, int g0, int g1, int n0, int n1,
                           const int* rects, double bg_value, int subtract_bg, int max_iter, double max_dev,
                           double* d_ff, double* d_avgobj, int* d_density, int* iterations, double* dev) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  if (n > kStepsMaxN) IPA_UNSUPPORTED(ctx, "steps_separate: at most %d frames (got %d)", kStepsMaxN, n);
  IPA_REQUIRE(ctx, n >= 1, "steps_separate: needs at least one frame (got %d)", n);
  IPA_REQUIRE(ctx, d_grid && rects && d_ff && d_avgobj && d_density && iterations && dev,
              "steps_separate: null pointer");
  IPA_REQUIRE(ctx, g0 >= 1 && g1 >= 1 && n0 >= 1 && n1 >= 1, "steps_separate: empty grid or device");
  IPA_REQUIRE(ctx, max_iter >= 0 && max_iter <= kSepMaxIter, "steps_separate: max_iter must lie in 0 ... %d (got %d)",
              kSepMaxIter, max_iter);
  if ((long)g0 * g1 > kSepMaxCells || (long)n0 * n1 > kSepMaxCells)
    IPA_UNSUPPORTED(ctx, "steps_separate: at most 2^16 grid cells and 2^16 device cells (got %d x %d, %d x %d)", g0, g1,
                    n0, n1);
  for (int k = 0; k < n; k++) {
    const int* r = rects + k * 6;
    IPA_REQUIRE(ctx, r[4] >= 0 && r[5] >= 0 && r[0] >= 0 && r[1] >= 0 && r[2] >= 0 && r[3] >= 0 &&
                         (long)r[0] + r[4] <= n0 && (long)r[1] + r[5] <= n1 && (long)r[2] + r[4] <= g0 &&
                         (long)r[3] + r[5] <= g1,
                "steps_separate: the rectangle of frame %d leaves the device or the grid", k);
  }
  const int G = g0 * g1, D = n0 * n1;
  const Span spans[] = {span2d(d_ff, 1, G, G, 8), span2d(d_avgobj, 1, D, D, 8), span2d(d_density, 1, G, G, 4),
                        span2d(d_grid, 1, (long)n * G, (long)n * G, 8)};
  IPA_REQUIRE(ctx, !written_overlaps(spans, 3), "steps_separate: an output overlaps another array");
  // the flat field and the object go through the workspace where LDS does not hold them (ws null: it does)
  int* d_iter;
  double *d_dev, *ws;
  int rc = stage_ws(ctx, slot(&d_iter, 1), slot(&d_dev, 1), slot(&ws, G + D <= kSepLds ? 0 : G + D));
  if (rc) return rc;
  void* d_rects;
  rc = ipa_tab_upload(ctx, rects, (size_t)n * 6 * sizeof(int), &d_rects);
  if (rc) return rc;
  rc = launch(ctx, steps_separate_kernel, dim3(1), dim3(kSepThreads), 0, d_grid, n, g0, g1, n0, n1, d_rects, bg_value,
              subtract_bg ? 1 : 0, max_iter, max_dev, ws, d_ff, d_avgobj, d_density, d_iter, d_dev);
  if (rc) return rc;
  return ipa_stage_out(ctx, {{iterations, d_iter, sizeof(int)}, {dev, d_dev, sizeof(double)}});
}

int ipa_offset_meshgrid_dev(ipa_ctx* ctx, double start0, double step0, double stop0, double start1, double step1,
                            double stop1, int h, int w, int dtype, void* d_yy, void* d_xx, long pitch) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  IPA_REQUIRE(ctx, d_yy && d_xx, "offset_meshgrid: null pointer");
  int tiles_x;
  unsigned grid;
  const int rc = frame_args(ctx, "offset_meshgrid", h, w, &tiles_x, &grid);
  if (rc != IPA_OK) return rc;
  IPA_REQUIRE(ctx, pitch >= w, "offset_meshgrid: pitch smaller than width");
  if (dtype != IPA_F32 && dtype != IPA_F64)
    IPA_UNSUPPORTED(ctx, "offset_meshgrid: float32 / float64 (got dtype %d)", dtype);
  const size_t es = ipa_dtype_size(dtype);
  IPA_REQUIRE(ctx, !overlap(span2d(d_yy, h, w, pitch, es), span2d(d_xx, h, w, pitch, es)),
              "offset_meshgrid: the two arrays overlap");
  return by_float(dtype, [&](auto e) {
    using T = decltype(e);
    return launch(ctx, offset_meshgrid_kernel<T>, dim3(grid), dim3(kTileThreads), 0, start0, step0, stop0, start1,
                  step1, stop1, h, w, tiles_x, d_yy, d_xx, pitch);
  });
}

int ipa_isnan_mask_dev(ipa_ctx* ctx, const void* d_in, int dtype, int h, int w, long pitch, unsigned char* d_mask,
                       long mask_pitch) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  IPA_REQUIRE(ctx, d_in && d_mask, "isnan_mask: null pointer");
  int tiles_x;
  unsigned grid;
  const int rc = frame_args(ctx, "isnan_mask", h, w, &tiles_x, &grid);
  if (rc != IPA_OK) return rc;
  IPA_REQUIRE(ctx, pitch >= w && mask_pitch >= w, "isnan_mask: pitch smaller than width");
  if (dtype != IPA_F32 && dtype != IPA_F64)
    IPA_UNSUPPORTED(ctx, "isnan_mask: float32 / float64 (got dtype %d)", dtype);
  IPA_REQUIRE(ctx, !overlap(span2d(d_mask, h, w, mask_pitch, 1), span2d(d_in, h, w, pitch, ipa_dtype_size(dtype))),
              "isnan_mask: the mask overlaps the frame");
  return by_float(dtype, [&](auto e) {
    using T = decltype(e);
    return launch(ctx, isnan_mask_kernel<T>, dim3(grid), dim3(kTileThreads), 0, d_in, pitch, h, w, tiles_x, d_mask,
                  mask_pitch);
  });
}

}  // extern "C"
