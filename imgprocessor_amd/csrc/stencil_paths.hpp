// stencil_paths.hpp — which kernel each secondary-stencil entry point launches, as host
// arithmetic in ONE place: the launchers of stencils.hip / stencils_ydep.hip call these, and
// ipa_stencil_path (include/imgproc_hip.h) reports them without a context, so that the tests can
// prove on which side of every threshold a case stands.  0 = refused (IPA_ERR_UNSUPPORTED or a
// bad argument), 1.. = the kernels in the order given per function.
#pragma once
#include <cstddef>

#include "../../include/imgproc_hip.h"

namespace ipa {

static inline size_t stencil_esize(int dtype) { return dtype == IPA_F32 ? 4 : 8; }
static inline bool stencil_float(int dtype) { return dtype == IPA_F32 || dtype == IPA_F64; }

// 1 = 256-px wave kernel (square half window 1..5), 2 = LDS tile kernel (the window of a
// 64 x 4 block within 48 KiB), 3 = generic
static inline size_t local_std_tile_lds(int dtype, int hkx, int hky) {
  return (size_t)(64 + 2 * hky) * (4 + 2 * hkx) * stencil_esize(dtype);
}
static inline int local_std_path(int dtype, int ksize_x, int ksize_y) {
  if (!stencil_float(dtype) || ksize_x < 2 || ksize_y < 2) return 0;
  const int hkx = ksize_x / 2, hky = ksize_y / 2;
  if (hkx == hky && hkx <= 5) return 1;
  return local_std_tile_lds(dtype, hkx, hky) <= 48 * 1024 ? 2 : 3;
}

// the in-place fill: 1 = column-sum kernel (half window <= 32: its cs[4][128] holds 64 + 2k
// columns), 2 = wave kernel.  (Out of place, and fill_mask == 0, always run the plain kernel.)
static inline int masked_mean_fill_path(int dtype, int ksize) {
  if (!stencil_float(dtype) || ksize < 2) return 0;
  return ksize / 2 <= 32 ? 1 : 2;
}

// 1 = wave kernel, 0 = refused: two key buffers of (2k)^2 entries per wave, 4 waves, 64 KiB
static inline size_t masked_median_lds(int dtype, int ksize) {
  const size_t k = (size_t)(ksize / 2);
  return (size_t)4 * 2 * (4 * k * k) * stencil_esize(dtype);
}
static inline int masked_median_path(int dtype, int ksize) {
  if (!stencil_float(dtype) || ksize < 2) return 0;
  return masked_median_lds(dtype, ksize) <= 64 * 1024 ? 1 : 0;
}

// 1 = separable LDS kernel (32-row blocks, source tile + row-maxima plane within 60 KiB),
// 2 = generic
constexpr int kNanMaxRB = 32;
static inline size_t nan_max_sep_lds(int dtype, int ksize) {
  const size_t k = (size_t)(ksize / 2), rb = kNanMaxRB;
  return ((rb + 2 * k) * (64 + 2 * k) + (rb + 2 * k) * 64) * stencil_esize(dtype);
}
static inline int nan_max_path(int dtype, int ksize) {
  if (!stencil_float(dtype) || ksize < 2) return 0;
  return nan_max_sep_lds(dtype, ksize) <= 60 * 1024 ? 1 : 2;
}

// 1 = two passes over byte row distances (255 means "none", so ksize <= 254), 2 = direct
static inline int closest_distance_path(int ksize) {
  if (ksize < 1 || ksize >= 20000) return 0;
  return ksize <= 254 ? 1 : 2;
}

// ksize = HALF window.  1 = separable (a column-factor slot per thread within 60 KiB),
// 2 = generic
static inline size_t pos_intensity_unc_lds(int ksize) {
  return (size_t)(2 * ksize + 1) * 256 * sizeof(double);
}
static inline int pos_intensity_unc_path(int dtype, int ksize) {
  if (!stencil_float(dtype) || ksize < 1) return 0;
  return pos_intensity_unc_lds(ksize) <= 60 * 1024 ? 1 : 2;
}

// 1 = 3x3 selection network, 2 = counting kernel, 0 = its window tile exceeds 64 KiB
static inline size_t median_threshold_lds(int dtype, int size) {
  return (size_t)(4 + size - 1) * ((64 + size - 1) | 1) * stencil_esize(dtype);
}
static inline int median_threshold_path(int dtype, int size) {
  if (!stencil_float(dtype) || size < 1) return 0;
  if (size == 3) return 1;
  return median_threshold_lds(dtype, size) <= 64 * 1024 ? 2 : 0;
}

// ipa_conv_ydep_dev: 1 = LDS tile kernel (window of a 64 x 4 block within 48 KiB), 2 = generic
static inline size_t conv_ydep_tile_lds(int dtype, int k0, int k1) {
  return (size_t)(64 + k1 - 1) * (4 + k0 - 1) * stencil_esize(dtype);
}
static inline int conv_ydep_path(int dtype, int k0, int k1) {
  if (!stencil_float(dtype) || k0 < 1 || k1 < 1 || !(k0 & 1) || !(k1 & 1)) return 0;
  return conv_ydep_tile_lds(dtype, k0, k1) <= 48 * 1024 ? 1 : 2;
}

// ipa_idw_fill_dev (idw.hip; not among ipa_stencil_path's ops).  ksize = HALF window.
// 1 = lanes over the taps, 2 = lanes over the columns of a window row (windows 17..64 wide)
static inline int idw_path(int dtype, int ksize) {
  if (!stencil_float(dtype) || ksize < 1 || ksize > 512) return 0;
  const int kw = 2 * ksize + 1;
  return kw > 16 && kw <= 64 ? 2 : 1;
}

// ipa_var_y_gauss_dev: 1 = tiled kernel (256 px x rb rows per workgroup), else the h x ky x kx
// table is expanded and ipa_conv_ydep_dev runs it: 2 = through its tile kernel, 3 = generic
constexpr int kYdepTW = 256;  // output pixels per workgroup row (4 per lane)
struct var_y_gauss_plan {
  int rb;      // rows per workgroup
  size_t lds;  // bytes of the tiled kernel at rb
  int path;
};
static inline var_y_gauss_plan var_y_gauss_plan_of(int dtype, int ky, int kx) {
  var_y_gauss_plan p = {0, 0, 0};
  if (!stencil_float(dtype) || ky < 1 || kx < 1 || !(ky & 1) || !(kx & 1) || kx > 255 ||
      ky > 4095)
    return p;
  const size_t esz = stencil_esize(dtype);
  const int tw = kYdepTW + kx - 1 + 3;
  auto lds_of = [&](int r) {
    return (size_t)r * ky * 8 + (size_t)kx * 8 + (size_t)(r + ky - 1) * tw * esz;
  };
  // rows per workgroup: ~2 x the kernel height (read amplification <= 1.5) while the tile stays
  // below ~30 KB (5 workgroups per CU), never above 60 KB
  int rb = 2 * ky < 16 ? 16 : (2 * ky + 3) / 4 * 4;
  if (rb > 64) rb = 64;
  while (rb > 8 && lds_of(rb) > 30 * 1024) rb -= 4;
  while (rb > 4 && lds_of(rb) > 60 * 1024) rb -= 4;
  p.rb = rb;
  p.lds = lds_of(rb);
  // windows beyond the tile (stdyrange above ~23 for float32, ~11 for float64): the whole
  // h x ky x kx table is expanded on the device and the generic entry point runs it - any
  // stdyrange the reference accepts works, as before the tiled kernel existed
  p.path = p.lds <= 64 * 1024 ? 1 : 1 + conv_ydep_path(dtype, ky, kx);
  return p;
}

}  // namespace ipa
