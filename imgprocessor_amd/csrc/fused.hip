// fused.hip — C-ABI entry points of the fused remap -> filter chains (dense K x K: fused_impl.hpp, one translation unit
// per K, and fused_big.hip; separable K + K: fused_sep_impl.hpp, fused_sep_{a,b,c}.hip).
// Every export fills ONE ChainArgs (fused_impl.hpp) from its own argument order - the dense exports take the filter's
// borders as (x, y), the separable ones as (y, x) - and from there the record travels by reference with the coordinates
// (ChainCoords) and the filter beside it: dense_chain / sep_chain (rank-1 route, cached lens map, rotated warps), then
// fused_common / fused_sep_common (one kernel or two launches).  Which kernel a dense chain takes: dense_route, the only
// place that reads big_fused / stream_k / pipe7.
#include "fused_sep_impl.hpp"
#if IPA_WITH_TILE_CHAIN
#include "tile_chain.hpp"   // experiment builds only (tools/tile_chain): tile_chain_try
#endif

using namespace ipa;

// (these three: the status of their launches)
int ipa_fused_sep_launch_a(ipa_ctx*, const FusedCall&, const FusedSep&);  // 3, 5 taps
int ipa_fused_sep_launch_b(ipa_ctx*, const FusedCall&, const FusedSep&);  // 7, 9 taps
int ipa_fused_sep_launch_c(ipa_ctx*, const FusedCall&, const FusedSep&);  // 1 tap: the remap alone
int ipa_fused_sep_launch_c16(ipa_ctx*, const FusedCall&);  // ... uint16 into uint16 (cv2's 16U arithmetic); 1 = not covered
int ipa_fused_sep_launch_c8(ipa_ctx*, const FusedCall&);   // ... uint8 into uint8 (cv2's 8U fixed point); 1 = not covered

// (these four: kNotCovered = no kernel for the call's types, coordinates or interpolation, nothing launched)
int ipa_fused_launch_k3(ipa_ctx*, const FusedCall&);
int ipa_fused_launch_k5(ipa_ctx*, const FusedCall&);
int ipa_fused_launch_k7(ipa_ctx*, const FusedCall&);
int ipa_fused_big_launch(ipa_ctx*, const FusedCall&, int K);  // fused_big.hip
int ipa_check_interp_border(ipa_ctx* ctx, int interp, int border);  // remap.hip
int make_undistort_coord(ipa_ctx* ctx, const double* K, const double* d, const double* newK, UndistortCoord* c);  // remap.hip

// Which chains are ONE kernel (float32 results); the others take two launches through the workspace (two_launch_remap).
// coord_kind 0 maps, 1 lens model, 2 homography - the lens model of a call that goes through its cached map is 0.
//   dense 3 / 5 / 7   float32 frames: bilinear and the two bicubics, any coordinates; uint16 frames: bilinear, maps or the
//                     lens model; uint8 frames: bilinear, maps (fused_k*.hip; 7x7 resident or streamed, see dense_route);
//   dense 9 / 11      map-based bilinear remaps of float32 frames (fused_big.hip, knobs big_fused / stream_k): for the
//                     rest the sampling source plus 9 / 11 running rows exceed the VGPR budget that pays;
//   separable         bilinear, 3 / 5 / 7 / 9 taps (bicubic: built and correct, but 16 taps per sample on the K - 1 extra
//                     halo rows of every strip make it slower than two launches - 4K, 9 taps: 813 vs 694 us); integer
//                     frames (knob sep_u16) also one tap: uint16 with maps or a homography, uint8 with maps.
// Round 6: every other combination the standalone entry points accept - Lanczos4 / nearest taps, uint8 frames, uint16
// frames with a homography or bicubic taps, rectangular or larger kernels - runs as two launches (it returned
// IPA_ERR_UNSUPPORTED before): a caller of the chain gets what remap + filter give, in whatever number of launches.

// The dense rule, the one place it is written.  kStreamed: wave_stencil_big_kernel (fused_big.hip), coefficient rows
// through SGPRs; kResident: wave_stencil_kernel (fused_k*.hip), 3 / 5 / 7 taps.
//   9x9 / 11x11 on float32 frames: one kernel; big_fused = 0 is the tuning knob that sends them through the two launches.
//   7x7 as well: with the sampling source's scalar state, 49 resident coefficients overflow the SGPR file (331 spills);
//   streamed, the 4K chain measured 489 -> 449 us (float32) and 493 -> 460 us (uint16 frames); 5x5 measured slower
//   streamed (0.427 vs 0.399 ms, 16 frames).  stream_k = 9 is the tuning knob that puts 7x7 back on the resident form.
//   shared7 (round 3): batches of uint16 frames whose frames share map rows through LDS (wave_run_strip_shared: bilinear,
//   n_frames a multiple of the workgroup's waves) keep the 7x7 coefficients resident as op_sel pairs on the
//   hand-scheduled loop: C4 64 x 4K 1.475 -> 1.333 ms (knob pipe7 = 0: streamed).  float32 frames measure the same either
//   way (1.484 / 1.484: two more tap registers per footprint, 141 VGPRs) and stay on the streamed kernel.
// *fused_checks: the call has the shape the streamed kernel was built around (7 .. 11 taps, even counts and every
// interpolation included) and has therefore always been validated as a fused call first (fused_fill), also where it
// then takes the two launches: its refusals keep their texts.
enum DenseRoute { kResident, kStreamed, kTwoLaunches };
static DenseRoute dense_route(const ipa_ctx* ctx, int src_dtype, int dst_dtype, int coord_kind, int interp, int kh, int kw,
                              int n_frames, bool* fused_checks = nullptr) {
  const ipa_tuning& t = ctx->tune;
  const int base = interp & 0xff;
  const bool linear = base == IPA_INTER_LINEAR;
  if (fused_checks) *fused_checks = false;
  if (dst_dtype != IPA_F32 || kh != kw) return kTwoLaunches;
  const bool shared7 = kh == 7 && t.pipe7 != 0 && linear && src_dtype == IPA_U16 &&
                       shared_loop_plan(ctx, true, n_frames, true) == kSharedLoop;
  const bool stream_shaped = coord_kind == 0 && t.big_fused != 0 && kh >= t.stream_k && kh >= 7 && kh <= 11 && !shared7 &&
                             (src_dtype == IPA_F32 || (kh == 7 && src_dtype == IPA_U16));
  if (fused_checks) *fused_checks = stream_shaped;
  if (stream_shaped && linear && (kh & 1)) return kStreamed;
  if (!(kh == 3 || kh == 5 || kh == 7)) return kTwoLaunches;
  bool resident = false;
  if (src_dtype == IPA_F32) resident = linear || base == IPA_INTER_CUBIC_CV || base == IPA_INTER_CUBIC_KEYS;
  else if (src_dtype == IPA_U16) resident = linear && coord_kind != 2;
  else resident = src_dtype == IPA_U8 && linear && coord_kind == 0;
  return resident ? kResident : kTwoLaunches;
}
// the separable rule, and with it the rank-1 route of a dense kernel (taps 0: ky and kx differ in length; taps 1: the
// remap alone, remap.hip's strip remap)
static bool chain_one_kernel(const ipa_ctx* ctx, int src_dtype, int dst_dtype, int coord_kind, int interp, int taps) {
  const ipa_tuning& t = ctx->tune;
  if (dst_dtype != IPA_F32 || (interp & 0xff) != IPA_INTER_LINEAR) return false;
  if (!(taps == 3 || taps == 5 || taps == 7 || taps == 9 || (taps == 1 && src_dtype != IPA_F32))) return false;
  if (src_dtype == IPA_F32) return true;
  if (src_dtype == IPA_U16) return t.sep_u16 && coord_kind != 1;
  return src_dtype == IPA_U8 && t.sep_u16 && coord_kind == 0;
}
int ipa_chain_one_kernel(const ipa_ctx* ctx, int src_dtype, int dst_dtype, int coord_kind, int interp) {  // (remap.hip)
  return chain_one_kernel(ctx, src_dtype, dst_dtype, coord_kind, interp, 1);
}

// where a chain's coordinates come from, as its caller gave them
struct ChainCoords {
  int kind;                       // 0 maps, 1 lens model, 2 homography
  const float *mx, *my;           // 0
  long map_pitch;
  const double *K, *dist5, *newK; // 1
  const double* M;                // 2
};
static int chain_coord(ipa_ctx* ctx, const ChainCoords& c, FusedCall& f) {
  f.coord_kind = c.kind;
  if (c.kind == 0) f.map = MapCoord{c.mx, c.my, c.map_pitch};
  else if (c.kind == 1) return make_undistort_coord(ctx, c.K, c.dist5, c.newK, &f.und);
  else for (int i = 0; i < 9; i++) f.hom.m[i] = c.M[i];
  return IPA_OK;
}


// the first of the two launches of a chain that is not one kernel: the remap into the context workspace (float32 frames
// of dh x dw, back to back); the filter follows from there.  Same results: the fused kernels round the remapped rows to
// float32 as well.
static int two_launch_remap(ipa_ctx* ctx, const ChainArgs& a, const ChainCoords& c) {
  IPA_REQUIRE(ctx, a.dh > 0 && a.dw > 0 && a.n_frames >= 1, "empty image");
  int rc = ipa_ws_reserve(ctx, (size_t)a.n_frames * a.dh * a.dw * 4);
  if (rc) return rc;
  const long fs = (long)a.dh * a.dw;
  // chain_path describes the chain's own kernels: the standalone remap may run on the chains' strip launchers (remap.hip),
  // whose bits are not this call's - what it launched stays readable as remap_path
  const unsigned own = ctx->chain_path;
  switch (c.kind) {
    case 0:
      rc = ipa_remap_dev(ctx, a.src, a.src_dtype, a.sh, a.sw, a.src_pitch, c.mx, c.my, c.map_pitch, ctx->ws, IPA_F32,
                         a.dh, a.dw, a.dw, a.n_frames, a.src_frame_stride, fs, a.interp, a.border_mode, a.border_value);
      break;
    case 1:
      rc = ipa_undistort_dev(ctx, a.src, a.src_dtype, a.sh, a.sw, a.src_pitch, c.K, c.dist5, c.newK, ctx->ws, IPA_F32,
                             a.dh, a.dw, a.dw, a.n_frames, a.src_frame_stride, fs, a.interp, a.border_mode,
                             a.border_value);
      break;
    default:
      rc = ipa_warp_perspective_dev(ctx, a.src, a.src_dtype, a.sh, a.sw, a.src_pitch, c.M, ctx->ws, IPA_F32, a.dh, a.dw,
                                    a.dw, a.n_frames, a.src_frame_stride, fs, a.interp, a.border_mode, a.border_value);
  }
  ctx->chain_path = own | IPA_CHAIN_PATH_TWO_LAUNCHES;
  return rc;
}

// validation + everything of a FusedCall that does not depend on the filter
static int fused_fill(ipa_ctx* ctx, FusedCall& f, const ChainArgs& a) {
  IPA_REQUIRE(ctx, a.src && a.dst, "null pointer");
  IPA_REQUIRE(ctx, a.sh > 0 && a.sw > 0 && a.dh > 0 && a.dw > 0, "empty image");
  IPA_REQUIRE(ctx, a.src_pitch >= a.sw && a.dst_pitch >= a.dw, "pitch smaller than width");
  IPA_REQUIRE(ctx, a.src_pitch < (1l << 23), "source pitch must be below 2^23 elements");  // mul24
  IPA_REQUIRE(ctx, a.n_frames >= 1 && a.n_frames <= 65535, "n_frames must be in [1,65535]");
  int rc = ipa_check_interp_border(ctx, a.interp, a.border_mode);
  if (rc) return rc;
  IPA_REQUIRE(ctx, a.conv_border_x >= 0 && a.conv_border_x <= IPA_BORDER_REFLECT101 && a.conv_border_y >= 0 &&
                       a.conv_border_y <= IPA_BORDER_REFLECT101,
              "unknown filter border mode");
  size_t ss = ipa_dtype_size(a.src_dtype), ds = ipa_dtype_size(a.dst_dtype);
  IPA_REQUIRE(ctx, ss && ds, "unknown dtype");
  size_t frame_bytes = ((size_t)(a.sh - 1) * a.src_pitch + a.sw) * ss;
  IPA_REQUIRE(ctx, frame_bytes < (1ull << 31), "source frame too large for 32-bit offsets");
  int base = a.interp & 0xff;
  WaveParams& p = f.p;
  p.dst = (char*)a.dst;
  p.dst_frame_elems = a.dst_frame_stride;
  p.dh = a.dh; p.dw = a.dw; p.dpitch = a.dst_pitch;
  p.cbx = a.conv_border_x; p.cby = a.conv_border_y;
  p.vec_out = aligned_rows(a.dst, a.dst_pitch, a.dst_frame_stride, a.n_frames, ds, IPA_VEC_ALIGN);
  f.src = (const char*)a.src;
  f.src_frame_bytes = a.src_frame_stride * (long)ss;
  f.src_bytes = (unsigned)frame_bytes;
  f.sh = a.sh; f.sw = a.sw; f.spitch = (int)a.src_pitch;
  f.border = a.border_mode; f.q5 = (a.interp & IPA_INTER_Q5) ? 1 : 0;
  f.cubic_a = base == IPA_INTER_CUBIC_KEYS ? -0.5f : -0.75f;
  f.cval = a.border_value;
  f.conv_cval = 0.0;
  f.map_vec = f.coord_kind == 0 && aligned_rows(f.map.mx, f.map.pitch, 0, 1, 4, IPA_VEC_ALIGN) &&
              aligned_rows(f.map.my, f.map.pitch, 0, 1, 4, IPA_VEC_ALIGN);
  f.src_dt = a.src_dtype; f.dst_dt = a.dst_dtype; f.interp_base = base; f.n_frames = a.n_frames;
  f.kernel = nullptr;
  return IPA_OK;
}

// remap -> K x K filter: one kernel where dense_route says so (prefer_two: rotated warps, below), else two launches
// - the remap into the workspace, then the plain filter.  (Calls the two launches would reject themselves go on to the
// fused path's own checks.)
static int fused_common(ipa_ctx* ctx, const ChainArgs& a, const ChainCoords& c, const double* kernel, int kh, int kw,
                        bool prefer_two = false) {
  bool fused_checks;
  const DenseRoute route =
      dense_route(ctx, a.src_dtype, a.dst_dtype, c.kind, a.interp, kh, kw, a.n_frames, &fused_checks);
  FusedCall f;
  int rc = IPA_OK;
  if (route == kTwoLaunches && fused_checks && kernel) {   // (maps: chain_coord cannot fail)
    chain_coord(ctx, c, f);
    if ((rc = fused_fill(ctx, f, a))) return rc;
  }
  if (route != kTwoLaunches ? prefer_two
                            : a.dst_dtype == IPA_F32 && a.dh > 0 && a.dw > 0 && a.n_frames >= 1 && kh >= 1 && kw >= 1) {
    if ((rc = two_launch_remap(ctx, a, c))) return rc;
    return ipa_conv2d_dev(ctx, ctx->ws, IPA_F32, a.dh, a.dw, a.dw, kernel, kh, kw, nullptr, 0, a.dst, a.dst_pitch,
                          a.n_frames, (long)a.dh * a.dw, a.dst_frame_stride, a.conv_border_x, a.conv_border_y, 0.0);
  }
  IPA_REQUIRE(ctx, kernel, "null pointer");
  if (kh != kw || !(kh == 3 || kh == 5 || kh == 7 || kh == 9 || kh == 11))
    IPA_UNSUPPORTED(ctx, "fused remap+filter is built for square 3/5/7/9/11 kernels (got %dx%d); "
                         "use ipa_remap_dev + ipa_conv2d_dev", kh, kw);
  if ((rc = chain_coord(ctx, c, f))) return rc;
  if ((rc = fused_fill(ctx, f, a))) return rc;
  f.kernel = kernel;
  IPA_HIP(ctx, hipSetDevice(ctx->device));
  rc = kNotCovered;   // (a call that is here for the checks above alone: no route, no launch)
  if (route == kStreamed) rc = ipa_fused_big_launch(ctx, f, kh);
  else if (route == kResident && kh == 3) rc = ipa_fused_launch_k3(ctx, f);
  else if (route == kResident && kh == 5) rc = ipa_fused_launch_k5(ctx, f);
  else if (route == kResident && kh == 7) rc = ipa_fused_launch_k7(ctx, f);
  if (rc == kNotCovered)
    IPA_UNSUPPORTED(ctx, "fused remap+filter: src dtype %d -> dst dtype %d not supported "
                         "(float32->float32 and uint16->float32 are)", a.src_dtype, a.dst_dtype);
  if (rc) return rc;
  IPA_HIP(ctx, hipGetLastError());
  return IPA_OK;
}

// remap -> separable filter: one kernel (wave_sep_kernel) where chain_one_kernel says so, else two launches as above
static int fused_sep_common(ipa_ctx* ctx, const ChainArgs& a, const ChainCoords& c, const double* ky, int nky,
                            const double* kx, int nkx, bool prefer_two = false) {
  FusedCall f;
  int rc = chain_coord(ctx, c, f);
  if (rc) return rc;
  IPA_REQUIRE(ctx, ky && kx && nky > 0 && nkx > 0 && (nky & 1) && (nkx & 1),
              "ky / kx must be given with odd lengths");
  IPA_REQUIRE(ctx, a.dst_dtype == IPA_F32, "remap + separable filter writes float32");
  if (prefer_two || !chain_one_kernel(ctx, a.src_dtype, a.dst_dtype, c.kind, a.interp, nky == nkx ? nky : 0)) {
    if ((rc = two_launch_remap(ctx, a, c))) return rc;
    return ipa_sepconv2d_dev(ctx, ctx->ws, IPA_F32, a.dh, a.dw, a.dw, ky, nky, kx, nkx, a.dst, a.dst_pitch, a.n_frames,
                             (long)a.dh * a.dw, a.dst_frame_stride, a.conv_border_y, a.conv_border_x, 0.0);
  }
  if ((rc = fused_fill(ctx, f, a))) return rc;
  FusedSep q{ky, kx, nky, 0.0f};
  IPA_HIP(ctx, hipSetDevice(ctx->device));
  if (nky == 1) return ipa_fused_sep_launch_c(ctx, f, q);
  return nky <= 5 ? ipa_fused_sep_launch_a(ctx, f, q) : ipa_fused_sep_launch_b(ctx, f, q);
}

// A homography whose output rows drift across source rows (a rotation of a few degrees) is where
// the fused kernels lose: their gathers pay per cache line a wave touches (16 x 4K, perspective
// warp + separable 9+9: 0.33 ms at no rotation, 0.47 at 7 degrees, 0.72 at 15, 1.52 at 45).  For batches
// the tile warp kernel takes (remap_impl.hpp: tile_warp_pays) the chain then runs as two
// launches - tile warp into the workspace, filter - whose time hardly depends on the angle
// (0.52 - 0.66 ms); same results (the fused kernels round the remapped rows to float32 too).
static bool rotated_warp_in_two_launches(const ipa_ctx* ctx, const double* m, int src_dtype,
                                         int dst_dtype, int interp, int dh, int dw, int n_frames) {
  if (!ctx->tune.tile_warp || src_dtype != IPA_F32 || dst_dtype != IPA_F32) return false;
  if ((interp & 0xff) != IPA_INTER_LINEAR) return false;
  if (n_frames < 8 || (double)n_frames * dh * dw < 64e6) return false;
  const double drift = homography_row_drift(m, dh, dw);
  return drift < 1e6 && drift >= (ctx->tune.tile_warp > 1 ? 0.0 : 0.2);   // (not finite: never)
}

// The lens model through its cached float32 map (knob lens_cache): the model's coordinates are the same for every frame
// and every call with these parameters - evaluated once (bit for bit what the per-pixel evaluation gives), and the call
// runs the map-based kernels, 9x9 / 11x11 in one kernel included.  (The map has dh x dw entries, pitch dw, and is there
// when ipa_lens_map_cached returns 0: the map checks of the exports hold for it.)
static int lens_through_cache(ipa_ctx* ctx, const ChainArgs& a, ChainCoords& c) {
  if (c.kind != 1 || !ctx->tune.lens_cache) return IPA_OK;
  float *mx = nullptr, *my = nullptr;
  int rc = ipa_lens_map_cached(ctx, c.K, c.dist5, c.newK, a.dh, a.dw, &mx, &my);
  if (rc) return rc;
  c = ChainCoords{0, mx, my, a.dw};
  ctx->chain_path |= IPA_CHAIN_PATH_LENS_MAP;
  return IPA_OK;
}

// what the three separable exports do once their coordinates are checked
static int sep_chain(ipa_ctx* ctx, const ChainArgs& a, ChainCoords c, const double* ky, int nky, const double* kx,
                     int nkx) {
  int rc = lens_through_cache(ctx, a, c);
  if (rc) return rc;
  bool rotated = false;
  if (c.kind == 2) {
    rotated = a.dh > 0 && a.dw > 0 &&
              rotated_warp_in_two_launches(ctx, c.M, a.src_dtype, a.dst_dtype, a.interp, a.dh, a.dw, a.n_frames);
    if (rotated) ctx->chain_path |= IPA_CHAIN_PATH_ROTATED;
#if IPA_WITH_TILE_CHAIN
    if ((rc = tile_chain_try(ctx, a, c.M, ky, nky, kx, nkx, rotated)) <= 0) return rc;   // (1: not taken)
#endif
  }
  return fused_sep_common(ctx, a, c, ky, nky, kx, nkx, rotated);
}

// Dense K x K kernels that are an outer product ky (x) kx - the bench's 5x5 is outer(g, g), and the reference itself
// obtains its Gaussians separably (scipy.ndimage.gaussian_filter: filters/standardDeviation.py:23,
// filters/fastFilter.py:42) - run on the separable K + K chain when that chain is ONE kernel for the call.  64 x 4K maps
// + 5x5: K + K = 10 instead of K * K = 25 multiply-adds per pixel on the same strips.  Knob rank1_sep bit 0; the two
// loops differ by the order of a float32 sum only (both within 1e-5 of the oracle's double sum).
static int dense_chain(ipa_ctx* ctx, const ChainArgs& a, ChainCoords c, const double* kernel, int kh, int kw) {
  double ky[9], kx[9];
  const int kind = c.kind == 1 && ctx->tune.lens_cache ? 0 : c.kind;
  if ((ctx->tune.rank1_sep & 1) && kernel && kh == kw && kh != 1 &&
      chain_one_kernel(ctx, a.src_dtype, a.dst_dtype, kind, a.interp, kh) && ipa_rank1_factor(kernel, kh, kw, ky, kx)) {
    ctx->rank1_routed++;
    ctx->chain_path |= IPA_CHAIN_PATH_RANK1;
    return sep_chain(ctx, a, c, ky, kh, kx, kw);
  }
  int rc = lens_through_cache(ctx, a, c);
  if (rc) return rc;
  const bool rotated = c.kind == 2 && kernel && a.dh > 0 && a.dw > 0 &&
                       rotated_warp_in_two_launches(ctx, c.M, a.src_dtype, a.dst_dtype, a.interp, a.dh, a.dw, a.n_frames);
  if (rotated) ctx->chain_path |= IPA_CHAIN_PATH_ROTATED;
  return fused_common(ctx, a, c, kernel, kh, kw, rotated);
}

// The strip remap of integer frames INTO their own type (remap.hip::ipa_remap_dev): cv2.remap's bilinear as it computes
// it on 16U (float32 product weights at 1/32-px coordinates) and 8U (15-bit fixed point) images - what
// LensDistortion.correct returns for camera frames - on the shared-record loop.  Returns 1 when the call is not one the
// loop covers on EVERY strip (the caller then takes the gather kernel), 0 when launched.
int ipa_strip_remap_int(ipa_ctx* ctx, int dtype, const void* d_src, int sh, int sw, long src_pitch, const float* d_mapx,
                        const float* d_mapy, long map_pitch, void* d_dst, int dh, int dw, long dst_pitch, int n_frames,
                        long src_frame_stride, long dst_frame_stride, int interp, int border_mode,
                        double border_value) {
  if (!ctx->tune.strip_remap || !ctx->tune.sep_u16) return 1;
  // uint16: cv2's arithmetic is what 'linear_cv_q5' names ('linear' = exact coordinates in double: the gather kernel);
  // uint8: every bilinear remap is cv2's fixed point
  if (dtype == IPA_U16 ? interp != (IPA_INTER_LINEAR | IPA_INTER_Q5)
                       : (dtype != IPA_U8 || (interp & 0xff) != IPA_INTER_LINEAR || (interp & ~(0xff | IPA_INTER_Q5)) != 0))
    return 1;
  // (the frame count and the grid: the shared-loop plan in fused_sep_c.hip)
  if (n_frames < 1 || n_frames > 65535) return 1;
  if (!d_src || !d_dst || !d_mapx || !d_mapy || sh <= 0 || sw <= 0 || dh <= 0 || dw <= 0 || (dw & 3) != 0) return 1;
  if (src_pitch < sw || dst_pitch < dw || map_pitch < dw || src_pitch >= (1l << 23)) return 1;
  if (((size_t)(sh - 1) * src_pitch + sw) * ipa_dtype_size(dtype) >= (1ull << 31)) return 1;
  const ChainArgs a{d_src, dtype, sh, sw, src_pitch, d_dst, dtype, dh, dw, dst_pitch, n_frames, src_frame_stride,
                    dst_frame_stride, interp, border_mode, border_value, IPA_BORDER_REFLECT, IPA_BORDER_REFLECT};
  FusedCall f;
  f.coord_kind = 0;
  f.map = MapCoord{d_mapx, d_mapy, map_pitch};
  int rc = fused_fill(ctx, f, a);
  if (rc) return rc;
  if (!f.p.vec_out || !f.map_vec) return 1;   // (rows of the result / of the maps that are no whole 16-byte vectors)
  // the border value as cv2 casts it: saturate_cast
  const double r = rint(border_value), top = dtype == IPA_U16 ? 65535.0 : 255.0;
  f.cval = r > 0 ? (r < top ? r : top) : 0;
  IPA_HIP(ctx, hipSetDevice(ctx->device));
  rc = dtype == IPA_U16 ? ipa_fused_sep_launch_c16(ctx, f) : ipa_fused_sep_launch_c8(ctx, f);
  if (rc) return rc;   // (1: not covered, or the status of a launch)
  ctx->strip_remaps++;
  ctx->remap_path |= IPA_REMAP_PATH_STRIP_INT;
  return IPA_OK;
}

extern "C" {

// (each export: its own checks, its arguments into a ChainArgs - mind the order of the two filter borders -, the chain)

int ipa_remap_sepconv2d_dev(ipa_ctx* ctx, const void* d_src, int src_dtype, int sh, int sw,
                            long src_pitch, const float* d_mapx, const float* d_mapy,
                            long map_pitch, const double* ky, int nky, const double* kx, int nkx,
                            void* d_dst, int dst_dtype, int dh, int dw, long dst_pitch, int n_frames,
                            long src_frame_stride, long dst_frame_stride, int interp,
                            int border_mode, double border_value, int conv_border_y,
                            int conv_border_x) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  ctx->chain_path = 0;
  IPA_REQUIRE(ctx, d_mapx && d_mapy && map_pitch >= dw, "bad map arguments");
  const ChainArgs a{d_src, src_dtype, sh, sw, src_pitch, d_dst, dst_dtype, dh, dw, dst_pitch, n_frames, src_frame_stride,
                    dst_frame_stride, interp, border_mode, border_value, conv_border_x, conv_border_y};
  return sep_chain(ctx, a, ChainCoords{0, d_mapx, d_mapy, map_pitch}, ky, nky, kx, nkx);
}

int ipa_undistort_sepconv2d_dev(ipa_ctx* ctx, const void* d_src, int src_dtype, int sh, int sw,
                                long src_pitch, const double* K, const double* dist5,
                                const double* newK, const double* ky, int nky, const double* kx,
                                int nkx, void* d_dst, int dst_dtype, int dh, int dw, long dst_pitch,
                                int n_frames, long src_frame_stride, long dst_frame_stride,
                                int interp, int border_mode, double border_value, int conv_border_y,
                                int conv_border_x) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  ctx->chain_path = 0;
  IPA_REQUIRE(ctx, K && dist5 && newK, "K, dist5 and newK must be given");
  const ChainArgs a{d_src, src_dtype, sh, sw, src_pitch, d_dst, dst_dtype, dh, dw, dst_pitch, n_frames, src_frame_stride,
                    dst_frame_stride, interp, border_mode, border_value, conv_border_x, conv_border_y};
  return sep_chain(ctx, a, ChainCoords{1, nullptr, nullptr, 0, K, dist5, newK}, ky, nky, kx, nkx);
}

int ipa_warp_perspective_sepconv2d_dev(ipa_ctx* ctx, const void* d_src, int src_dtype, int sh,
                                       int sw, long src_pitch, const double* M, const double* ky,
                                       int nky, const double* kx, int nkx, void* d_dst,
                                       int dst_dtype, int dh, int dw, long dst_pitch, int n_frames,
                                       long src_frame_stride, long dst_frame_stride, int interp,
                                       int border_mode, double border_value, int conv_border_y,
                                       int conv_border_x) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  ctx->chain_path = 0;
  IPA_REQUIRE(ctx, M, "null matrix");
  const ChainArgs a{d_src, src_dtype, sh, sw, src_pitch, d_dst, dst_dtype, dh, dw, dst_pitch, n_frames, src_frame_stride,
                    dst_frame_stride, interp, border_mode, border_value, conv_border_x, conv_border_y};
  return sep_chain(ctx, a, ChainCoords{2, nullptr, nullptr, 0, nullptr, nullptr, nullptr, M}, ky, nky, kx, nkx);
}

int ipa_remap_conv2d_dev(ipa_ctx* ctx, const void* d_src, int src_dtype, int sh, int sw,
                         long src_pitch, const float* d_mapx, const float* d_mapy, long map_pitch,
                         const double* kernel, int kh, int kw, void* d_dst, int dst_dtype, int dh,
                         int dw, long dst_pitch, int n_frames, long src_frame_stride,
                         long dst_frame_stride, int interp, int border_mode, double border_value,
                         int conv_border_x, int conv_border_y) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  ctx->chain_path = 0;
  IPA_REQUIRE(ctx, d_mapx && d_mapy && map_pitch >= dw, "bad map arguments");
  const ChainArgs a{d_src, src_dtype, sh, sw, src_pitch, d_dst, dst_dtype, dh, dw, dst_pitch, n_frames, src_frame_stride,
                    dst_frame_stride, interp, border_mode, border_value, conv_border_x, conv_border_y};
  return dense_chain(ctx, a, ChainCoords{0, d_mapx, d_mapy, map_pitch}, kernel, kh, kw);
}

int ipa_undistort_conv2d_dev(ipa_ctx* ctx, const void* d_src, int src_dtype, int sh, int sw,
                             long src_pitch, const double* K, const double* dist5,
                             const double* newK, const double* kernel, int kh, int kw, void* d_dst,
                             int dst_dtype, int dh, int dw, long dst_pitch, int n_frames,
                             long src_frame_stride, long dst_frame_stride, int interp,
                             int border_mode, double border_value, int conv_border_x,
                             int conv_border_y) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  ctx->chain_path = 0;
  IPA_REQUIRE(ctx, K && dist5 && newK, "K, dist5 and newK must be given");
  const ChainArgs a{d_src, src_dtype, sh, sw, src_pitch, d_dst, dst_dtype, dh, dw, dst_pitch, n_frames, src_frame_stride,
                    dst_frame_stride, interp, border_mode, border_value, conv_border_x, conv_border_y};
  return dense_chain(ctx, a, ChainCoords{1, nullptr, nullptr, 0, K, dist5, newK}, kernel, kh, kw);
}

int ipa_warp_perspective_conv2d_dev(ipa_ctx* ctx, const void* d_src, int src_dtype, int sh, int sw,
                                    long src_pitch, const double* M, const double* kernel, int kh,
                                    int kw, void* d_dst, int dst_dtype, int dh, int dw,
                                    long dst_pitch, int n_frames, long src_frame_stride,
                                    long dst_frame_stride, int interp, int border_mode,
                                    double border_value, int conv_border_x, int conv_border_y) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  ctx->chain_path = 0;
  IPA_REQUIRE(ctx, M, "null matrix");
  const ChainArgs a{d_src, src_dtype, sh, sw, src_pitch, d_dst, dst_dtype, dh, dw, dst_pitch, n_frames, src_frame_stride,
                    dst_frame_stride, interp, border_mode, border_value, conv_border_x, conv_border_y};
  return dense_chain(ctx, a, ChainCoords{2, nullptr, nullptr, 0, nullptr, nullptr, nullptr, M}, kernel, kh, kw);
}

}  // extern "C"
