// remap.hip — C-ABI entry points of the gather half of the hot path
// (kernels + dispatch: remap_impl.hpp, one translation unit per coordinate source).
#include <math.h>

#define IPA_REMAP_API_TU
#include "remap_impl.hpp"
#include "cv_tables.hpp"

int ipa_remap_launch_map(ipa_ctx*, const RemapCall&, const MapCoord&, int map_vec);
int ipa_remap_launch_undistort(ipa_ctx*, const RemapCall&, const UndistortCoord&);
int ipa_remap_launch_homography(ipa_ctx*, const RemapCall&, const HomographyCoord&);
int ipa_remap_launch_grid(ipa_ctx*, const RemapCall&, const int* cell_rects, const double* cell_M, int n_cells);
int ipa_chain_one_kernel(const ipa_ctx* ctx, int src_dtype, int dst_dtype, int coord_kind, int interp);  // fused.hip: the remap alone as one kernel

// ---------------------------------------------------------------- host side --
static int inv3(const double* m, double* o) {
  double a = m[0], b = m[1], c = m[2], d = m[3], e = m[4], f = m[5], g = m[6], h = m[7], i = m[8];
  double A = e * i - f * h, B = -(d * i - f * g), C = d * h - e * g;
  double det = a * A + b * B + c * C;
  if (det == 0 || det != det) return -1;
  double id = 1.0 / det;
  o[0] = A * id; o[1] = -(b * i - c * h) * id; o[2] = (b * f - c * e) * id;
  o[3] = B * id; o[4] = (a * i - c * g) * id;  o[5] = -(a * f - c * d) * id;
  o[6] = C * id; o[7] = -(a * h - b * g) * id; o[8] = (a * e - b * d) * id;
  return 0;
}

// (fused.hip builds the coordinates of its chains here too)
int make_undistort_coord(ipa_ctx* ctx, const double* K, const double* d, const double* newK, UndistortCoord* c) {
  IPA_REQUIRE(ctx, K && d && newK, "K, dist5 and newK must be given");
  IPA_REQUIRE(ctx, inv3(newK, c->ir) == 0, "newK is singular");
  c->fx = K[0]; c->fy = K[4]; c->cx = K[2]; c->cy = K[5];
  c->k1 = d[0]; c->k2 = d[1]; c->p1 = d[2]; c->p2 = d[3]; c->k3 = d[4];
  c->affine = (c->ir[6] == 0.0 && c->ir[7] == 0.0 && c->ir[8] == 1.0) ? 1 : 0;
  return IPA_OK;
}

// cv2's interpolation tables (cv_tables.hpp), built once on the host and uploaded once per device.  One allocation each:
// IPA_CV_TABLE_ROWS 384 floats, IPA_CV_TABLE_U8_CUBIC 32 KB (remap_kernel keeps it in LDS), IPA_CV_TABLE_U8_LANCZOS4
// 128 KB (remap_u8_lz_kernel keeps it in the LDS of a 1024-thread workgroup).
static const std::vector<char>& cv_table_host(int which) {
  static const std::vector<char> tabs[3] = {
      [] { std::vector<char> t(cv_tables::kRowsFloats * 4); cv_tables::rows_table((float*)t.data()); return t; }(),
      [] { std::vector<char> t(cv_tables::kTab2dDwords<4> * 4); cv_tables::fixed_tab2d<4>((int*)t.data()); return t; }(),
      [] { std::vector<char> t(cv_tables::kTab2dDwords<8> * 4); cv_tables::fixed_tab2d<8>((int*)t.data()); return t; }()};
  return tabs[which];
}

static std::mutex g_cv_table_mu;
static void* g_cv_table_dev[3][64] = {};

int ipa_cv_table_dev(ipa_ctx* ctx, int which, const void** out) {
  std::lock_guard<std::mutex> lk(g_cv_table_mu);
  const int dev = ctx->device;
  IPA_REQUIRE(ctx, dev >= 0 && dev < 64, "device id out of range");
  if (!g_cv_table_dev[which][dev]) {
    const std::vector<char>& tab = cv_table_host(which);
    void* d = nullptr;
    IPA_HIP(ctx, hipSetDevice(dev));
    IPA_HIP(ctx, hipMalloc(&d, tab.size()));
    IPA_HIP(ctx, hipMemcpy(d, tab.data(), tab.size(), hipMemcpyHostToDevice));
    g_cv_table_dev[which][dev] = d;
  }
  *out = g_cv_table_dev[which][dev];
  return IPA_OK;
}

int ipa_check_interp_border(ipa_ctx* ctx, int interp, int border) {
  int base = interp & 0xff;
  IPA_REQUIRE(ctx, (interp & ~(0xff | IPA_INTER_Q5)) == 0, "unknown interpolation flags 0x%x",
              interp);
  IPA_REQUIRE(ctx,
              base == IPA_INTER_NEAREST || base == IPA_INTER_LINEAR ||
                  base == IPA_INTER_CUBIC_CV || base == IPA_INTER_LANCZOS4 ||
                  base == IPA_INTER_CUBIC_KEYS,
              "unknown interpolation %d", base);
  IPA_REQUIRE(ctx, border >= IPA_BORDER_CONSTANT && border <= IPA_BORDER_REFLECT101,
              "unknown border mode %d", border);
  return IPA_OK;
}

// the host-pointer remaps: argument checks, then source | result | map x | map y staged (the maps where given)
struct Staged {
  char* d[4];   // src, dst, mx, my
  size_t dst_bytes;
};

static int remap_stage(ipa_ctx* ctx, const void* src, int src_dt, int sh, int sw, int dst_dt, int dh,
                       int dw, int n_frames, const float* mapx, const float* mapy, Staged* st) {
  IPA_REQUIRE(ctx, src, "null source");
  IPA_REQUIRE(ctx, sh > 0 && sw > 0 && dh > 0 && dw > 0 && n_frames >= 1, "bad shape");
  size_t ss = ipa_dtype_size(src_dt), ds = ipa_dtype_size(dst_dt);
  IPA_REQUIRE(ctx, ss && ds, "unknown dtype");
  const size_t map_bytes = mapx ? (size_t)dh * dw * 4 : 0;
  st->dst_bytes = (size_t)dh * dw * ds * n_frames;
  return ipa_stage_in(ctx, {{src, (size_t)sh * sw * ss * n_frames}, {nullptr, st->dst_bytes}, {mapx, map_bytes},
                            {mapy, map_bytes}}, st->d);
}

// the float32 maps of a lens model, kept in the context until another model or size is asked for
int ipa_lens_map_cached(ipa_ctx* ctx, const double* K, const double* dist5, const double* newK,
                        int h, int w, float** mx, float** my) {
  double key[25];
  for (int i = 0; i < 9; i++) key[i] = K[i];
  for (int i = 0; i < 5; i++) key[9 + i] = dist5[i];
  for (int i = 0; i < 9; i++) key[14 + i] = newK[i];
  key[23] = (double)h;
  key[24] = (double)w;
  const size_t mb = ((size_t)h * w * 4 + 255) & ~(size_t)255;
  const bool hit = ctx->lens_key_n == 25 && memcmp(ctx->lens_key, key, sizeof(key)) == 0;
  if (!hit) {
    ctx->lens_key_n = 0;
    int rc = ipa_grow_reserve(ctx, &ctx->lens_map, &ctx->lens_map_bytes, 2 * mb, 2 * mb);   // earlier calls may still read the old maps
    if (rc) return rc;
    rc = ipa_build_undistort_map_dev(ctx, K, dist5, newK, h, w, (float*)ctx->lens_map,
                                     (float*)((char*)ctx->lens_map + mb), w);
    if (rc) return rc;
    memcpy(ctx->lens_key, key, sizeof(key));
    ctx->lens_key_n = 25;
  }
  *mx = (float*)ctx->lens_map;
  *my = (float*)((char*)ctx->lens_map + mb);
  return IPA_OK;
}

extern "C" {

int ipa_build_undistort_map_dev(ipa_ctx* ctx, const double* K, const double* dist5,
                                const double* newK, int h, int w, float* d_mapx, float* d_mapy,
                                long map_pitch) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  IPA_REQUIRE(ctx, d_mapx && d_mapy && h > 0 && w > 0 && map_pitch >= w, "bad map arguments");
  UndistortCoord c;
  int rc = make_undistort_coord(ctx, K, dist5, newK, &c);
  if (rc) return rc;
  int vec = aligned_rows(d_mapx, map_pitch, 0, 1, 4, IPA_VEC_ALIGN) &&
            aligned_rows(d_mapy, map_pitch, 0, 1, 4, IPA_VEC_ALIGN);
  dim3 grid((w + 255) / 256, (h + 3) / 4), block(64, 4);
  IPA_HIP(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(build_map_kernel, grid, block, 0, ctx->stream, c, h, w, d_mapx, d_mapy,
                     map_pitch, vec);
  IPA_HIP(ctx, hipGetLastError());
  return IPA_OK;
}

int ipa_build_undistort_map(ipa_ctx* ctx, const double* K, const double* dist5,
                            const double* newK, int h, int w, float* mapx, float* mapy) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  IPA_REQUIRE(ctx, mapx && mapy && h > 0 && w > 0, "bad map arguments");
  const size_t mb = (size_t)h * w * 4;
  char* d[2];
  int rc = ipa_stage_in(ctx, {{nullptr, mb}, {nullptr, mb}}, d);
  if (rc) return rc;
  rc = ipa_build_undistort_map_dev(ctx, K, dist5, newK, h, w, (float*)d[0], (float*)d[1], w);
  if (rc) return rc;
  return ipa_stage_out(ctx, {{mapx, d[0], mb}, {mapy, d[1], mb}});
}

// Round 6 (knob strip_remap): bilinear remaps of uint16 frames INTO float32 - camera frames as
// transformations.toFloatArray ingests them (transformations.py:78-87), the element types of BASELINE C4 - run on
// the marching strips of the fused chains with NO filter (wave_sep_kernel, K = 1: 256-px strips, no halo, both
// passes the identity; fused_sep_c.hip): the gather kernels these calls took stream 64 x 4K in 1.28 ms, the strips in
// 0.90 (maps; -30 %), lens model 1.42 -> 0.89, homography 1.16 -> 1.07; identical bits (tools/strip_remap_probe.py).
// Batches the shared-loop plan puts on the shared-footprint loop (wave_stencil.hpp::shared_loop_plan: a multiple of 4
// frames, from 7 frames on any count) for maps and homographies that do not turn the picture; the lens model by value at
// any count (`any_count`: its map is evaluated once and cached).  uint8 frames (8-bit cameras) the same with maps:
// 1.28 -> 0.93 ms.  float32 frames stay where they are: the tile kernel is level with the strips on maps and 15 - 19 %
// faster on homographies.  (fused.hip::chain_one_kernel, knob sep_u16: the chain's two-launch form would come back here)
static bool strip_remap_takes(const ipa_ctx* ctx, const void* d_src, const void* d_dst, int src_dtype, int dst_dtype,
                              int sh, int sw, long src_pitch, int dh, int dw, long dst_pitch, int n_frames,
                              int interp, int coord_kind, bool any_count) {
  if (!ctx->tune.strip_remap) return false;
  if (shared_loop_plan(ctx, true, any_count ? IPA_WPB : n_frames, true) == kPerFrameLoop) return false;
  if (!ipa_chain_one_kernel(ctx, src_dtype, dst_dtype, coord_kind, interp) || !d_src || !d_dst) return false;
  if ((interp & ~(0xff | IPA_INTER_Q5)) != 0) return false;
  // (what the chain kernels' 32-bit offsets hold; anything else stays with the gather kernels and their checks)
  if (sh <= 0 || sw <= 0 || dh <= 0 || dw <= 0 || src_pitch < sw || dst_pitch < dw || src_pitch >= (1l << 23)) return false;
  if (((size_t)(sh - 1) * src_pitch + sw) * ipa_dtype_size(src_dtype) >= (1ull << 31) || n_frames < 1 || n_frames > 65535) return false;
  return true;
}
static const double kOneTap = 1.0;

int ipa_remap_dev(ipa_ctx* ctx, const void* d_src, int src_dtype, int sh, int sw, long src_pitch,
                  const float* d_mapx, const float* d_mapy, long map_pitch, void* d_dst,
                  int dst_dtype, int dh, int dw, long dst_pitch, int n_frames,
                  long src_frame_stride, long dst_frame_stride, int interp, int border_mode,
                  double border_value) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  ctx->remap_path = 0;
  IPA_REQUIRE(ctx, d_mapx && d_mapy && map_pitch >= dw, "bad map arguments");
  if ((src_dtype == IPA_U16 || src_dtype == IPA_U8) && dst_dtype == src_dtype) {
    // ... and INTO the frames' own integer type with cv2's arithmetic (what LensDistortion.correct returns for camera
    // frames): the same strips, the blend of sampler.hpp::sample_u16_cv / sample_u8_fixed
    // (fused.hip::ipa_strip_remap_int; 1: not a call it covers)
    int rc = ipa_strip_remap_int(ctx, src_dtype, d_src, sh, sw, src_pitch, d_mapx, d_mapy, map_pitch, d_dst, dh, dw,
                                 dst_pitch, n_frames, src_frame_stride, dst_frame_stride, interp, border_mode,
                                 border_value);
    if (rc <= 0) return rc;
  }
  if (strip_remap_takes(ctx, d_src, d_dst, src_dtype, dst_dtype, sh, sw, src_pitch, dh, dw, dst_pitch, n_frames, interp, 0, false)) {
    ctx->strip_remaps++;
    const int crc = ipa_remap_sepconv2d_dev(ctx, d_src, src_dtype, sh, sw, src_pitch, d_mapx, d_mapy, map_pitch, &kOneTap, 1,
                                   &kOneTap, 1, d_dst, dst_dtype, dh, dw, dst_pitch, n_frames, src_frame_stride,
                                   dst_frame_stride, interp, border_mode, border_value, IPA_BORDER_REFLECT,
                                   IPA_BORDER_REFLECT);
    if (crc == IPA_OK) ctx->remap_path |= IPA_REMAP_PATH_STRIP;   // (the chain's own checks passed: enqueued)
    return crc;
  }
  MapCoord c{d_mapx, d_mapy, map_pitch};
  int map_vec = aligned_rows(d_mapx, map_pitch, 0, 1, 4, IPA_VEC_ALIGN) &&
            aligned_rows(d_mapy, map_pitch, 0, 1, 4, IPA_VEC_ALIGN);
  RemapCall a{d_src, src_dtype, sh, sw, src_pitch, d_dst, dst_dtype, dh, dw, dst_pitch,
              n_frames, src_frame_stride, dst_frame_stride, interp, border_mode, border_value};
  return ipa_remap_launch_map(ctx, a, c, map_vec);
}

int ipa_undistort_dev(ipa_ctx* ctx, const void* d_src, int src_dtype, int sh, int sw,
                      long src_pitch, const double* K, const double* dist5, const double* newK,
                      void* d_dst, int dst_dtype, int dh, int dw, long dst_pitch, int n_frames,
                      long src_frame_stride, long dst_frame_stride, int interp, int border_mode,
                      double border_value) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  ctx->remap_path = 0;
  UndistortCoord c;
  int rc = make_undistort_coord(ctx, K, dist5, newK, &c);
  if (rc) return rc;
  if (ctx->tune.lens_cache && src_dtype == IPA_U16 &&   // (through the cached map; uint8 frames: ipa_remap_dev below)
      strip_remap_takes(ctx, d_src, d_dst, src_dtype, dst_dtype, sh, sw, src_pitch, dh, dw, dst_pitch, n_frames, interp, 0, true)) {
    ctx->strip_remaps++;
    const int crc = ipa_undistort_sepconv2d_dev(ctx, d_src, src_dtype, sh, sw, src_pitch, K, dist5, newK, &kOneTap, 1, &kOneTap,
                                       1, d_dst, dst_dtype, dh, dw, dst_pitch, n_frames, src_frame_stride,
                                       dst_frame_stride, interp, border_mode, border_value, IPA_BORDER_REFLECT,
                                       IPA_BORDER_REFLECT);
    if (crc == IPA_OK) ctx->remap_path |= IPA_REMAP_PATH_STRIP;   // (the chain's own checks passed: enqueued)
    return crc;
  }
  // integer frames, batches: the model's float32 coordinates are the same for every frame - through the cached
  // map (bit for bit what the per-pixel evaluation gives; the chains have used it since round 2) instead of
  // evaluating the model per pixel and frame: 64 x 4K uint16 -> uint16 1.77 -> 1.31 ms (float32 frames: level, stay)
  if (ctx->tune.lens_cache && n_frames >= 4 && (src_dtype == IPA_U8 || src_dtype == IPA_U16) && dh > 0 && dw > 0) {
    float *mx = nullptr, *my = nullptr;
    rc = ipa_lens_map_cached(ctx, K, dist5, newK, dh, dw, &mx, &my);
    if (rc) return rc;
    rc = ipa_remap_dev(ctx, d_src, src_dtype, sh, sw, src_pitch, mx, my, dw, d_dst, dst_dtype, dh, dw, dst_pitch,
                       n_frames, src_frame_stride, dst_frame_stride, interp, border_mode, border_value);
    ctx->remap_path |= IPA_REMAP_PATH_LENS_MAP;   // (ipa_remap_dev cleared the word on its entry: one word for the whole call)
    return rc;
  }
  RemapCall a{d_src, src_dtype, sh, sw, src_pitch, d_dst, dst_dtype, dh, dw, dst_pitch,
              n_frames, src_frame_stride, dst_frame_stride, interp, border_mode, border_value};
  return ipa_remap_launch_undistort(ctx, a, c);
}

int ipa_warp_perspective_dev(ipa_ctx* ctx, const void* d_src, int src_dtype, int sh, int sw,
                             long src_pitch, const double* M, void* d_dst, int dst_dtype, int dh,
                             int dw, long dst_pitch, int n_frames, long src_frame_stride,
                             long dst_frame_stride, int interp, int border_mode,
                             double border_value) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  ctx->remap_path = 0;
  IPA_REQUIRE(ctx, M, "null matrix");
  if (strip_remap_takes(ctx, d_src, d_dst, src_dtype, dst_dtype, sh, sw, src_pitch, dh, dw, dst_pitch, n_frames, interp,
                        2, false) &&
      homography_row_drift(M, dh, dw) < 0.2) {   // (see ipa_remap_dev; pictures that turn stay with the gather kernels)
    ctx->strip_remaps++;
    const int crc = ipa_warp_perspective_sepconv2d_dev(ctx, d_src, src_dtype, sh, sw, src_pitch, M, &kOneTap, 1, &kOneTap, 1,
                                              d_dst, dst_dtype, dh, dw, dst_pitch, n_frames, src_frame_stride,
                                              dst_frame_stride, interp, border_mode, border_value,
                                              IPA_BORDER_REFLECT, IPA_BORDER_REFLECT);
    if (crc == IPA_OK) ctx->remap_path |= IPA_REMAP_PATH_STRIP;   // (the chain's own checks passed: enqueued)
    return crc;
  }
  HomographyCoord c;
  for (int i = 0; i < 9; i++) c.m[i] = M[i];
  RemapCall a{d_src, src_dtype, sh, sw, src_pitch, d_dst, dst_dtype, dh, dw, dst_pitch,
              n_frames, src_frame_stride, dst_frame_stride, interp, border_mode, border_value};
  return ipa_remap_launch_homography(ctx, a, c);
}

// PerspectiveCorrection.correctGrid (camera/PerspectiveCorrection.py:281-372): every cell's own
// homography into its own rectangle, one launch (remap_grid.hip)
int ipa_warp_grid_dev(ipa_ctx* ctx, const void* d_src, int src_dtype, int sh, int sw, long src_pitch,
                      const int* cell_rects, const double* cell_M, int n_cells, void* d_dst,
                      int dst_dtype, int dh, int dw, long dst_pitch, int n_frames,
                      long src_frame_stride, long dst_frame_stride, int interp, int border_mode,
                      double border_value) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  ctx->remap_path = 0;
  RemapCall a{d_src, src_dtype, sh, sw, src_pitch, d_dst, dst_dtype, dh, dw, dst_pitch,
              n_frames, src_frame_stride, dst_frame_stride, interp, border_mode, border_value};
  return ipa_remap_launch_grid(ctx, a, cell_rects, cell_M, n_cells);
}

int ipa_cv_table(int which, void* out, size_t cap) {
  if (which < IPA_CV_TABLE_ROWS || which > IPA_CV_TABLE_U8_LANCZOS4) return -1;
  const std::vector<char>& tab = cv_table_host(which);
  if (out && cap >= tab.size()) memcpy(out, tab.data(), tab.size());
  return (int)tab.size();
}

int ipa_remap(ipa_ctx* ctx, const void* src, int src_dtype, int sh, int sw, const float* mapx,
              const float* mapy, void* dst, int dst_dtype, int dh, int dw, int n_frames,
              int interp, int border_mode, double border_value) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  IPA_REQUIRE(ctx, mapx && mapy && dst, "null pointer");
  Staged st;
  int rc = remap_stage(ctx, src, src_dtype, sh, sw, dst_dtype, dh, dw, n_frames, mapx, mapy, &st);
  if (rc) return rc;
  rc = ipa_remap_dev(ctx, st.d[0], src_dtype, sh, sw, sw, (const float*)st.d[2], (const float*)st.d[3], dw, st.d[1],
                     dst_dtype, dh, dw, dw, n_frames, (long)sh * sw, (long)dh * dw, interp,
                     border_mode, border_value);
  if (rc) return rc;
  return ipa_stage_out(ctx, {{dst, st.d[1], st.dst_bytes}});
}

int ipa_undistort(ipa_ctx* ctx, const void* src, int src_dtype, int sh, int sw, const double* K,
                  const double* dist5, const double* newK, void* dst, int dst_dtype, int dh,
                  int dw, int n_frames, int interp, int border_mode, double border_value) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  IPA_REQUIRE(ctx, dst, "null pointer");
  Staged st;
  int rc = remap_stage(ctx, src, src_dtype, sh, sw, dst_dtype, dh, dw, n_frames, nullptr, nullptr, &st);
  if (rc) return rc;
  rc = ipa_undistort_dev(ctx, st.d[0], src_dtype, sh, sw, sw, K, dist5, newK, st.d[1], dst_dtype,
                         dh, dw, dw, n_frames, (long)sh * sw, (long)dh * dw, interp, border_mode,
                         border_value);
  if (rc) return rc;
  return ipa_stage_out(ctx, {{dst, st.d[1], st.dst_bytes}});
}

int ipa_warp_perspective(ipa_ctx* ctx, const void* src, int src_dtype, int sh, int sw,
                         const double* M, void* dst, int dst_dtype, int dh, int dw, int n_frames,
                         int interp, int border_mode, double border_value) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  IPA_REQUIRE(ctx, dst, "null pointer");
  Staged st;
  int rc = remap_stage(ctx, src, src_dtype, sh, sw, dst_dtype, dh, dw, n_frames, nullptr, nullptr, &st);
  if (rc) return rc;
  rc = ipa_warp_perspective_dev(ctx, st.d[0], src_dtype, sh, sw, sw, M, st.d[1], dst_dtype, dh,
                                dw, dw, n_frames, (long)sh * sw, (long)dh * dw, interp,
                                border_mode, border_value);
  if (rc) return rc;
  return ipa_stage_out(ctx, {{dst, st.d[1], st.dst_bytes}});
}

int ipa_warp_grid(ipa_ctx* ctx, const void* src, int src_dtype, int sh, int sw, const int* cell_rects,
                  const double* cell_M, int n_cells, void* dst, int dst_dtype, int dh, int dw,
                  int n_frames, int interp, int border_mode, double border_value) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  IPA_REQUIRE(ctx, dst, "null pointer");
  Staged st;
  int rc = remap_stage(ctx, src, src_dtype, sh, sw, dst_dtype, dh, dw, n_frames, nullptr, nullptr, &st);
  if (rc) return rc;
  rc = ipa_warp_grid_dev(ctx, st.d[0], src_dtype, sh, sw, sw, cell_rects, cell_M, n_cells, st.d[1],
                         dst_dtype, dh, dw, dw, n_frames, (long)sh * sw, (long)dh * dw, interp,
                         border_mode, border_value);
  if (rc) return rc;
  return ipa_stage_out(ctx, {{dst, st.d[1], st.dst_bytes}});
}

}  // extern "C"
