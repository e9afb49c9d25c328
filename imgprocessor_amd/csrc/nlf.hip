// nlf.hip — noise level function estimation and signal-to-noise maps on gfx950:
//   ipa_nlf_signal_dev     camera/NoiseLevelFunction.py:208-228 (the median-filtered signal)
//   ipa_nlf_moments_dev    camera/NoiseLevelFunction.py:162-173 (_getMinMax: min, max, mean, std)
//   ipa_nlf_bins_dev       camera/NoiseLevelFunction.py:243-271 (the binned |noise| over signal)
//   ipa_snr_map_dev        measure/SNR/SNR.py:59-79
//   ipa_snr_bg_median_dev  measure/SNR/SNR.py:82-87 (the median grid under getBackgroundLevel)
//
// Everything is float64, as the reference is after np.asfarray.  The signal, the background
// grid and the SNR map are chains of single correctly rounded operations and equal numpy's
// bits; FP contraction is off for this file (Makefile + pragma) because numpy never fuses.
//
// The two reductions go through per-workgroup partials that a last small kernel adds in a fixed
// order - no global float atomics.  The moments of a call depend on its grid alone.  The bin
// counts are exact; the bin sums pass through float64 LDS atomics, and where several lanes of a
// wave add to one bin in one instruction the hardware chooses their order: the sums are pinned to
// 1e-12, not to the bit.
//   moments: two passes (sum, then sum of (x - mean)^2), the variance of a frame of mean 60000
//            and std 2 keeps its digits.
//   bins:    a persistent grid; every wave owns one table of nbins x {u32 count, f64 sum} in
//            LDS.  A lane takes a run of kRun consecutive pixels of one row and merges equal-bin
//            neighbours in registers before it touches the table: neighbouring pixels of a real
//            frame mostly share a bin.  The waves' tables merge into one slab row per workgroup,
//            written with plain stores (zeros where the workgroup got no pixel).
#include "common.hpp"
#include "frame_args.hpp"
#include "launch.hpp"
#include "nlf_fn.hpp"
#include "reduce.hpp"

#pragma clang fp contract(off)

namespace ipa {
namespace {

constexpr int kRun = 8;             // consecutive pixels of one row per lane (bins)
constexpr int kNlfThreads = 256;
constexpr int kNlfMaxBins = 2048;   // 24 KB of LDS per wave table
constexpr int kNlfLds = 65536;      // edges + the waves' tables of one workgroup
constexpr int kNlfMaxGrid = 4096;
constexpr long kNlfMaxPixels = 1L << 30;   // column indices rounded up to a run stay in an int

// The frame(s) of a call as the reference sees them after `img1 - bg`, `img2 - bg`
// (SNR.py:33-40; calcNLF passes no background: x - 0.0 is x).
struct NlfSrc {
  const void* img;
  const void* img2;    // NULL: one image
  const double* bg;    // NULL: bg_value
  long pitch, pitch2, bg_pitch;
  double bg_value;
  int xstep;           // element step between columns (10 under getBackgroundLevel, else 1)
};

template <typename T>
__device__ inline double src_px(const NlfSrc& s, const void* img, long pitch, int y, int x) {
  const double v = (double)((const T*)img)[(long)y * pitch + (long)x * s.xstep];
  return v - (s.bg ? s.bg[(long)y * s.bg_pitch + x] : s.bg_value);
}

// signal = median_filter(img, 3) or median_filter(0.5 * (img + img2), 3): rank 4 of the 9
// (median9 of nlf_fn.hpp), the edge pixel repeated.  A NaN in the window gives NaN (scipy's answer
// there is unspecified).
template <typename T>
__global__ void __launch_bounds__(kNlfThreads)
nlf_signal_kernel(NlfSrc s, int h, int w, int tiles_x, double* __restrict__ out, long out_pitch) {
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x = tx * 64 + (threadIdx.x & 63), y = ty * 4 + (threadIdx.x >> 6);
  if (x >= w || y >= h) return;
  double c[3][3];   // [column][row]
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const int xx = min(max(x + i - 1, 0), w - 1);
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const int yy = min(max(y + j - 1, 0), h - 1);
      double v = src_px<T>(s, s.img, s.pitch, yy, xx);
      if (s.img2) v = 0.5 * (v + src_px<T>(s, s.img2, s.pitch2, yy, xx));
      c[i][j] = v;
    }
  }
  out[(long)y * out_pitch + x] = median9(c);
}

// ---------------------------------------------------------------- moments
struct Moments {
  double sum, mn, mx;
  unsigned long long nan;
};
__device__ inline Moments merge(const Moments& a, const Moments& b) {
  return {a.sum + b.sum, b.mn < a.mn ? b.mn : a.mn, b.mx > a.mx ? b.mx : a.mx, a.nan + b.nan};
}

// pass 0: sum / min / max / NaN count of the non-NaN values; pass 1: sum of (x - mean)^2 with
// the mean of pass 0 read from res[2].  A unit is 256 consecutive pixels of one row.
template <typename T, int PASS>
__global__ void __launch_bounds__(kNlfThreads)
nlf_moments_kernel(const T* __restrict__ img, int h, int w, long pitch,
                   const double* __restrict__ res, Moments* __restrict__ part) {
  __shared__ Moments lds[kNlfThreads];
  const long upr = (w + kNlfThreads - 1) / kNlfThreads, units = (long)h * upr;
  const double mean = PASS ? res[2] : 0.0;
  Moments m = {0.0, __builtin_inf(), -__builtin_inf(), 0};
  for (long u = blockIdx.x; u < units; u += gridDim.x) {
    const long y = u / upr;
    const int x = (int)(u - y * upr) * kNlfThreads + threadIdx.x;
    if (x >= w) continue;
    const double v = (double)img[y * pitch + x];
    if (v != v) {
      m.nan++;
    } else if (PASS) {
      const double d = v - mean;
      m.sum += d * d;
    } else {
      m.sum += v;
      m.mn = v < m.mn ? v : m.mn;
      m.mx = v > m.mx ? v : m.mx;
    }
  }
  m = block_merge<kNlfThreads>(m, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = m;
}

// one workgroup: the partials in workgroup order.  res = {min, max, mean, std, NaN count}
template <int PASS>
__global__ void __launch_bounds__(kNlfThreads)
nlf_moments_final(const Moments* __restrict__ part, int n_part, long n_px, double* __restrict__ res) {
  __shared__ Moments lds[kNlfThreads];
  const Moments m = merge_partials<kNlfThreads>(part, n_part, {0.0, __builtin_inf(), -__builtin_inf(), 0}, lds);
  if (threadIdx.x != 0) return;
  const double n = (double)(n_px - (long)m.nan);
  if (PASS) {
    res[3] = sqrt(m.sum / n);
  } else {
    res[0] = m.mn;
    res[1] = m.mx;
    res[2] = m.sum / n;
    res[4] = (double)m.nan;
  }
}

// ---------------------------------------------------------------- bins
// a lane's run of equal-bin pixels, not yet in the wave's table
struct BinRun {
  int bin;
  unsigned n;
  double sum;
};
__device__ inline void run_flush(const BinRun& r, unsigned* cnt, double* sum) {
  if (r.n) {
    atomicAdd(&cnt[r.bin], r.n);
    atomicAdd(&sum[r.bin], r.sum);
  }
}
__device__ inline void run_add(BinRun& r, int bin, double v, unsigned* cnt, double* sum) {
  if (bin != r.bin) {
    run_flush(r, cnt, sum);
    r = {bin, 0u, 0.0};
  }
  r.n++;
  r.sum += v;
}

struct BinArgs {
  NlfSrc src;
  const double* signal;
  long signal_pitch;
  int h, w;
  const double* edges;   // nbins + 1, device
  int nbins;
  double step, factor;
  int rms;
  unsigned* slab_cnt;    // [grid][nbins]
  double* slab_sum;
};

// Bin n holds e[n] <= signal <= e[n + 1], both ends inclusive (:259): a pixel on an interior edge
// is in two bins, a NaN in none.  k = floor((s - e[0]) / step) is a guess - the table's edges are
// accumulated sums, not e[0] + n * step - so membership of k - 1, k, k + 1 is settled against the
// table itself.  LDS: edges | sums[waves][nbins] | counts[waves][nbins].
template <typename T>
__global__ void __launch_bounds__(kNlfThreads)
nlf_bins_kernel(BinArgs a) {
  extern __shared__ double lds[];
  const int nbins = a.nbins, waves = blockDim.x >> 6;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double* e = lds;
  double* sums = e + nbins + 1;
  unsigned* cnts = (unsigned*)(sums + waves * nbins);
  for (int i = threadIdx.x; i <= nbins; i += blockDim.x) e[i] = a.edges[i];
  for (int i = threadIdx.x; i < waves * nbins; i += blockDim.x) {
    sums[i] = 0.0;
    cnts[i] = 0u;
  }
  __syncthreads();
  double* wsum = sums + wave * nbins;
  unsigned* wcnt = cnts + wave * nbins;
  const long rpr = (a.w + kRun - 1) / kRun, nruns = (long)a.h * rpr;
  const long stride = (long)gridDim.x * waves * 64;
  const double e0 = e[0];
  for (long r = ((long)blockIdx.x * waves + wave) * 64 + lane; r < nruns; r += stride) {
    const long y = r / rpr;
    const int x0 = (int)(r - y * rpr) * kRun, x1 = min(x0 + kRun, a.w);
    BinRun first = {-1, 0u, 0.0}, second = {-1, 0u, 0.0};
    for (int x = x0; x < x1; x++) {
      const double s = a.signal[y * a.signal_pitch + x];
      const double v1 = src_px<T>(a.src, a.src.img, a.src.pitch, (int)y, x);
      const double d = a.src.img2
                           ? (v1 - src_px<T>(a.src, a.src.img2, a.src.pitch2, (int)y, x)) / a.factor
                           : (v1 - s) * a.factor;
      const double v = a.rms ? d * d : fabs(d);
      double kd = floor((s - e0) / a.step);
      if (!(kd >= -1.0)) kd = -1.0;   // below the table, NaN, or step == 0 with one bin
      if (kd > (double)nbins) kd = (double)nbins;
      const int k = (int)kd;
      int member = 0;
      for (int n = k - 1; n <= k + 1; n++) {
        if (n < 0 || n >= nbins || !(e[n] <= s && s <= e[n + 1])) continue;
        if (member == 0) {
          run_add(first, n, v, wcnt, wsum);
        } else if (member == 1) {
          run_add(second, n, v, wcnt, wsum);
        } else {
          atomicAdd(&wcnt[n], 1u);
          atomicAdd(&wsum[n], v);
        }
        member++;
      }
    }
    run_flush(first, wcnt, wsum);
    run_flush(second, wcnt, wsum);
  }
  __syncthreads();
  for (int n = threadIdx.x; n < nbins; n += blockDim.x) {
    unsigned c = 0u;
    double s = 0.0;
    for (int wv = 0; wv < waves; wv++) {
      c += cnts[wv * nbins + n];
      s += sums[wv * nbins + n];
    }
    a.slab_cnt[(long)blockIdx.x * nbins + n] = c;
    a.slab_sum[(long)blockIdx.x * nbins + n] = s;
  }
}

struct BinTotal {
  double sum;
  unsigned long long n;
};
__device__ inline BinTotal merge(const BinTotal& a, const BinTotal& b) { return {a.sum + b.sum, a.n + b.n}; }

// one workgroup per bin adds the slabs in a fixed order: thread t takes slabs t, t + 256, ..., then
// the tree over the threads
__global__ void __launch_bounds__(kNlfThreads)
nlf_bins_final(const unsigned* __restrict__ slab_cnt, const double* __restrict__ slab_sum, int n_slab,
               int nbins, unsigned long long* __restrict__ cnt, double* __restrict__ sum) {
  __shared__ BinTotal lds[kNlfThreads];
  const int n = blockIdx.x;
  BinTotal m = {0.0, 0};
  for (int g = threadIdx.x; g < n_slab; g += kNlfThreads) {
    m.n += slab_cnt[(long)g * nbins + n];
    m.sum += slab_sum[(long)g * nbins + n];
  }
  m = block_merge<kNlfThreads>(m, lds);
  if (threadIdx.x == 0) {
    cnt[n] = m.n;
    sum[n] = m.sum;
  }
}

// ---------------------------------------------------------------- SNR map
struct SnrArgs {
  const double* signal;
  long signal_pitch;
  int h, w;
  int form;              // 0: the triple, 1: d_noise, 2: const_noise
  double min_y, ax, ay;
  const double* noise;
  long noise_pitch;
  double const_noise, noise_factor, bg_level;
  double* out;
  long out_pitch;
};

__global__ void __launch_bounds__(kNlfThreads)
snr_map_kernel(SnrArgs a, int tiles_x) {
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x = tx * 64 + (threadIdx.x & 63), y = ty * 4 + (threadIdx.x >> 6);
  if (x >= a.w || y >= a.h) return;
  const double s = a.signal[(long)y * a.signal_pitch + x];
  double noise = a.const_noise;
  if (a.form != 2) {
    noise = a.form == 0 ? bounded_nlf(s, a.min_y, a.ax, a.ay) : a.noise[(long)y * a.noise_pitch + x];
    if (noise < 1.0) noise = 1.0;   // otherwise the SNR could exceed the image value (:64)
  }
  noise = noise * a.noise_factor;
  double snr = (s - a.bg_level) / noise;
  if (snr < 1.0) snr = 1.0;         // NaN stays NaN
  a.out[(long)y * a.out_pitch + x] = snr;
}

// the argument checks of the calls that read the frame(s) of an NlfSrc
int check_src(ipa_ctx* ctx, const char* what, const void* d_img, int dtype, const void* d_img2, int h,
              int w, long pitch, long pitch2, const double* d_bg, long bg_pitch) {
  IPA_REQUIRE(ctx, d_img, "%s: null image", what);
  IPA_REQUIRE(ctx, h > 0 && w > 0, "%s: empty image", what);
  IPA_REQUIRE(ctx, (long)h * w <= kNlfMaxPixels, "%s: more than 2^30 pixels", what);
  IPA_REQUIRE(ctx, pitch >= w && (!d_img2 || pitch2 >= w) && (!d_bg || bg_pitch >= w),
              "%s: pitch smaller than width", what);
  if (!known_dtype(dtype))
    IPA_UNSUPPORTED(ctx, "%s: frames are uint8 / uint16 / float32 / float64 (got dtype %d)", what, dtype);
  return IPA_OK;
}

int signal_call(ipa_ctx* ctx, const char* what, const NlfSrc& src, int dtype, int h, int w, double* d_out,
                long out_pitch) {
  int tiles_x;
  unsigned grid;
  const int rc = frame_args(ctx, what, h, w, &tiles_x, &grid);
  if (rc) return rc;
  return by_dtype(dtype, [&](auto e) {
    return launch(ctx, nlf_signal_kernel<decltype(e)>, dim3(grid), dim3(kNlfThreads), 0, src, h, w, tiles_x, d_out,
                  out_pitch);
  });
}

// one pass of the moments: the partials of `grid` workgroups, then their sum into res
template <int PASS>
int moments_pass(ipa_ctx* ctx, int dtype, int grid, const void* d_img, int h, int w, long pitch, double* res,
                 Moments* part) {
  const int rc = by_dtype(dtype, [&](auto e) {
    return launch(ctx, nlf_moments_kernel<decltype(e), PASS>, dim3(grid), dim3(kNlfThreads), 0, d_img, h, w, pitch,
                  res, part);
  });
  if (rc) return rc;
  return launch(ctx, nlf_moments_final<PASS>, dim3(1), dim3(kNlfThreads), 0, part, grid, (long)h * w, res);
}

// workgroups of a persistent launch: what the work needs, at most `per_cu` per compute unit
// (tuning knob nlf_grid: exactly that many, whatever the work)
int persistent_grid(const ipa_ctx* ctx, long needed, int per_cu) {
  if (ctx->tune.nlf_grid > 0) return ctx->tune.nlf_grid;
  const long cap = (long)(ctx->cu_count > 0 ? ctx->cu_count : 256) * per_cu;
  long g = needed < cap ? needed : cap;
  g = g < kNlfMaxGrid ? g : kNlfMaxGrid;
  return (int)(g > 1 ? g : 1);
}

}  // namespace
}  // namespace ipa

using namespace ipa;

extern "C" {

int ipa_nlf_signal_dev(ipa_ctx* ctx, const void* d_img, int dtype, const void* d_img2, int h, int w,
                       long pitch, long pitch2, const double* d_bg, long bg_pitch, double bg,
                       double* d_signal, long signal_pitch) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  int rc = check_src(ctx, "nlf_signal", d_img, dtype, d_img2, h, w, pitch, pitch2, d_bg, bg_pitch);
  if (rc) return rc;
  IPA_REQUIRE(ctx, d_signal && signal_pitch >= w, "nlf_signal: null signal or pitch smaller than width");
  const size_t es = ipa_dtype_size(dtype);
  const Span spans[] = {span2d(d_signal, h, w, signal_pitch, 8), span2d(d_img, h, w, pitch, es),
                        span2d(d_img2, h, w, pitch2, es), span2d(d_bg, h, w, bg_pitch, 8)};
  IPA_REQUIRE(ctx, !written_overlaps(spans, 1), "nlf_signal does not run in place");
  const NlfSrc src = {d_img, d_img2, d_bg, pitch, pitch2, bg_pitch, bg, 1};
  return signal_call(ctx, "nlf_signal", src, dtype, h, w, d_signal, signal_pitch);
}

int ipa_nlf_moments_dev(ipa_ctx* ctx, const void* d_img, int dtype, int h, int w, long pitch,
                        double* moments) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  IPA_REQUIRE(ctx, d_img && moments, "nlf_moments: null pointer");
  if (!known_dtype(dtype))
    IPA_UNSUPPORTED(ctx, "nlf_moments: frames are uint8 / uint16 / float32 / float64 (got dtype %d)", dtype);
  IPA_REQUIRE(ctx, h > 0 && w > 0 && pitch >= w, "nlf_moments: empty image or pitch smaller than width");
  IPA_REQUIRE(ctx, (long)h * w <= kNlfMaxPixels, "nlf_moments: more than 2^30 pixels");
  const long units = (long)h * ((w + kNlfThreads - 1) / kNlfThreads);
  const int grid = persistent_grid(ctx, units, 8);
  Moments* part;
  double* res;
  int rc = stage_ws(ctx, slot(&part, grid), slot(&res, 5));
  if (rc) return rc;
  rc = moments_pass<0>(ctx, dtype, grid, d_img, h, w, pitch, res, part);
  if (rc) return rc;
  rc = moments_pass<1>(ctx, dtype, grid, d_img, h, w, pitch, res, part);
  if (rc) return rc;
  return ipa_stage_out(ctx, {{moments, res, 5 * sizeof(double)}});
}

int ipa_nlf_bins_dev(ipa_ctx* ctx, const void* d_img, int dtype, const void* d_img2, int h, int w,
                     long pitch, long pitch2, const double* d_bg, long bg_pitch, double bg,
                     const double* d_signal, long signal_pitch, const double* edges, int nbins,
                     double step, double factor, int rms, unsigned long long* counts, double* sums) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  if (nbins > kNlfMaxBins)
    IPA_UNSUPPORTED(ctx, "nlf_bins: at most %d bins (got %d)", kNlfMaxBins, nbins);
  int rc = check_src(ctx, "nlf_bins", d_img, dtype, d_img2, h, w, pitch, pitch2, d_bg, bg_pitch);
  if (rc) return rc;
  IPA_REQUIRE(ctx, d_signal && signal_pitch >= w, "nlf_bins: null signal or pitch smaller than width");
  IPA_REQUIRE(ctx, edges && counts && sums && nbins >= 1, "nlf_bins: null table or no bins");
  IPA_REQUIRE(ctx, step > 0.0 || (step == 0.0 && nbins == 1),
              "nlf_bins: the bin width must be positive (got %g)", step);
  // the widest workgroup whose edges and wave tables fit
  int waves = (int)((kNlfLds - (size_t)(nbins + 1) * 8) / ((size_t)nbins * 12));
  waves = waves > kNlfThreads / 64 ? kNlfThreads / 64 : waves;
  const size_t lds = (size_t)(nbins + 1) * 8 + (size_t)waves * nbins * 12;
  const long nruns = (long)h * ((w + kRun - 1) / kRun);
  const int grid = persistent_grid(ctx, (nruns + waves * 64 - 1) / (waves * 64), 4);
  BinArgs a;
  double *d_edges, *d_sum;
  unsigned long long* d_cnt;
  const size_t slab = (size_t)grid * nbins;
  rc = stage_ws(ctx, slot(&d_edges, nbins + 1, edges), slot(&a.slab_sum, slab), slot(&d_sum, nbins),
                slot(&d_cnt, nbins), slot(&a.slab_cnt, slab));
  if (rc) return rc;
  a.src = {d_img, d_img2, d_bg, pitch, pitch2, bg_pitch, bg, 1};
  a.signal = d_signal;
  a.signal_pitch = signal_pitch;
  a.h = h;
  a.w = w;
  a.edges = d_edges;
  a.nbins = nbins;
  a.step = step;
  a.factor = factor;
  a.rms = rms;
  rc = by_dtype(dtype, [&](auto e) {
    return launch(ctx, nlf_bins_kernel<decltype(e)>, dim3(grid), dim3(waves * 64), lds, a);
  });
  if (rc) return rc;
  rc = launch(ctx, nlf_bins_final, dim3(nbins), dim3(kNlfThreads), 0, a.slab_cnt, a.slab_sum, grid, nbins, d_cnt,
              d_sum);
  if (rc) return rc;
  return ipa_stage_out(ctx, {{counts, d_cnt, (size_t)nbins * 8}, {sums, d_sum, (size_t)nbins * 8}});
}

int ipa_snr_map_dev(ipa_ctx* ctx, const double* d_signal, int h, int w, long pitch, const double* nlf,
                    const double* d_noise, long noise_pitch, double const_noise, double noise_factor,
                    double bg_level, double* d_snr, long snr_pitch) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  IPA_REQUIRE(ctx, d_signal && d_snr, "snr_map: null pointer");
  int tiles_x;
  unsigned grid;
  const int rc = frame_args(ctx, "snr_map", h, w, &tiles_x, &grid);
  if (rc) return rc;
  IPA_REQUIRE(ctx, pitch >= w && snr_pitch >= w && (!d_noise || noise_pitch >= w),
              "snr_map: pitch smaller than width");
  IPA_REQUIRE(ctx, !(nlf && d_noise), "snr_map: a triple or a noise array, not both");
  IPA_REQUIRE(ctx, !overlap(span2d(d_snr, h, w, snr_pitch, 8), span2d(d_noise, h, w, noise_pitch, 8)),
              "snr_map: the map overlaps the noise array");
  SnrArgs a;
  a.signal = d_signal;
  a.signal_pitch = pitch;
  a.h = h;
  a.w = w;
  a.form = nlf ? 0 : d_noise ? 1 : 2;
  a.min_y = nlf ? nlf[0] : 0.0;
  a.ax = nlf ? nlf[1] : 0.0;
  a.ay = nlf ? nlf[2] : 0.0;
  a.noise = d_noise;
  a.noise_pitch = noise_pitch;
  a.const_noise = const_noise;
  a.noise_factor = noise_factor;
  a.bg_level = bg_level;
  a.out = d_snr;
  a.out_pitch = snr_pitch;
  return launch(ctx, snr_map_kernel, dim3(grid), dim3(kNlfThreads), 0, a, tiles_x);
}

int ipa_snr_bg_median_dev(ipa_ctx* ctx, const void* d_img, int dtype, int h, int w, long pitch,
                          double* d_grid, long grid_pitch) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  int rc = check_src(ctx, "snr_bg_median", d_img, dtype, nullptr, h, w, pitch, 0, nullptr, 0);
  if (rc) return rc;
  IPA_REQUIRE(ctx, h > 20 && w > 20, "snr_bg_median: img[10:-10:10, 10:-10:10] is empty for a %d x %d frame",
              h, w);
  const int gh = (h - 20 + 9) / 10, gw = (w - 20 + 9) / 10;
  IPA_REQUIRE(ctx, d_grid && grid_pitch >= gw, "snr_bg_median: null grid or pitch smaller than %d", gw);
  // the sampled frame: origin (10, 10), every 10th row (the pitch) and column (xstep)
  const NlfSrc src = {(const char*)d_img + ((size_t)10 * pitch + 10) * ipa_dtype_size(dtype), nullptr, nullptr,
                      10 * pitch, 0, 0, 0.0, 10};
  return signal_call(ctx, "snr_bg_median", src, dtype, gh, gw, d_grid, grid_pitch);
}

}  // extern "C"
