// fused_impl.hpp — remap -> K x K filter in ONE kernel (the headline chain:
// LensDistortion.correct / PerspectiveCorrection.correct followed by a dense
// filter; in-tree archetype camera/lens/estimateSystematicErrorLensCorrection.py:199-207).
//
// The kernel is the wave-marching stencil of wave_stencil.hpp with a row
// source that samples the remapped image on the fly (positions outside the
// remapped image are resolved with the FILTER's border mode first, i.e.
// exactly what filtering the materialised remap result would see).  The
// intermediate image never exists in HBM: 16 B/px map-based, 8 B/px analytic,
// instead of 24 / 16 for two launches.
//
// This header is compiled once per K (fused_k*.hip define IPA_FUSED_K) so the
// translation units build in parallel.
#pragma once

#include "common.hpp"
#include "wave_stencil.hpp"
#include "stored_coords.hpp"

namespace ipa {

// host-side description of one fused call (coordinate source by kind)
struct FusedCall {
  WaveParams p;
  // remap source
  const char* src;
  long src_frame_bytes;
  unsigned src_bytes;
  int sh, sw, spitch;
  int border, q5;
  float cubic_a;
  double cval, conv_cval;
  int coord_kind;  // 0 map, 1 undistort, 2 homography
  int map_vec;
  MapCoord map;
  UndistortCoord und;
  HomographyCoord hom;
  int src_dt, dst_dt, interp_base, n_frames;
  const double* kernel;
};

// a launcher's answer to a call it has no kernel for (types, coordinates, interpolation): nothing launched.  fused.hip's
// dense_route sends the launchers only calls they cover; should the two ever disagree, the caller refuses the call.
constexpr int kNotCovered = 1;

// what every chain entry point receives, by name: fused.hip fills one from each export's own argument order and hands it
// on by reference (the coordinates and the filter travel beside it)
struct ChainArgs {
  const void* src;
  int src_dtype, sh, sw;
  long src_pitch;
  void* dst;
  int dst_dtype, dh, dw;
  long dst_pitch;
  int n_frames;
  long src_frame_stride, dst_frame_stride;   // elements
  int interp, border_mode;                   // of the remap
  double border_value;
  int conv_border_x, conv_border_y;          // the filter's border mode along a row / down a column
};

// the sampling row source of a fused call: everything but the members the kernel itself sets per frame
template <typename ST, int INTERP, typename Coord>
static inline void fused_source(SampleRowSrc<ST, INTERP, Coord>& s, const FusedCall& f, const Coord& c) {
  s.coord = c;
  s.src = f.src; s.src_frame_bytes = f.src_frame_bytes; s.src_bytes = f.src_bytes;
  s.sh = f.sh; s.sw = f.sw; s.spitch = f.spitch;
  s.border = f.border; s.q5 = f.q5; s.cubic_a = f.cubic_a; s.lanczos = nullptr;
  s.cval = (float)f.cval; s.ccval = (float)f.conv_cval; s.map_vec = f.map_vec;
}

// The shared-loop plan of a fused call (wave_stencil.hpp::shared_loop_plan, with its source and result byte ranges) and,
// when it is split, the two launches: part[0] the first n - n % IPA_WPB frames, part[1] the last IPA_WPB frames.
static inline SharedPlan fused_plan(const ipa_ctx* ctx, bool capable, const FusedCall& f, FusedCall (&part)[2]) {
  const long ds = (long)ipa_dtype_size(f.dst_dt);
  const char* s0 = f.src;
  const char* s1 = f.src + (long)f.n_frames * f.src_frame_bytes;
  const char* d0 = f.p.dst;
  const char* d1 = f.p.dst + (long)f.n_frames * f.p.dst_frame_elems * ds;
  const SharedPlan plan = shared_loop_plan(ctx, capable, f.n_frames, s1 <= d0 || d1 <= s0);
  if (plan == kSharedSplit) {
    part[0] = part[1] = f;
    part[0].n_frames = f.n_frames - f.n_frames % IPA_WPB;
    part[1].n_frames = IPA_WPB;
    part[1].src += (long)(f.n_frames - IPA_WPB) * f.src_frame_bytes;
    part[1].p.dst += (long)(f.n_frames - IPA_WPB) * f.p.dst_frame_elems * ds;
  }
  return plan;
}

// What every batch of a chain goes through before its launch (Capable: the kernel's trait, shared_capable / sep_shared):
// the plan; a homography's coordinates stored once; a split plan's head and tail.  launch(call, coordinates, plan) then
// launches ONE kernel over the frames of `call` and returns its status, which is what this returns.
// Homography batches on the shared-record loop (knob stored_coords: from that many frames): its double coordinates (two
// fused-multiply-add chains and a division per pixel) are evaluated ONCE per (matrix, geometry) into the plan buffer
// (stored_coords.hpp) and the record producers read them as a table - the C3 chain spent a third of its time evaluating
// them once per four frames.
template <typename ST, int INTERP, int K, template <typename, int> class Capable, typename Coord, typename Launch>
static int fused_batch(ipa_ctx* ctx, const FusedCall& f, const Coord& c, const Launch& launch) {
  constexpr bool capable = Capable<SampleRowSrc<ST, INTERP, Coord>, K>::value;
  FusedCall part[2];
  const SharedPlan plan = fused_plan(ctx, capable, f, part);
  if constexpr (std::is_same<Coord, HomographyCoord>::value && capable) {
    if (ctx->tune.stored_coords > 0 && f.n_frames >= ctx->tune.stored_coords && plan != kPerFrameLoop) {
      StoredCoord<double> sc;
      if (stored_coords_prepare<Coord>(ctx, c, f.p.dh, f.p.dw, &sc) == 0) {
        ctx->chain_path |= IPA_CHAIN_PATH_STORED;
        return fused_batch<ST, INTERP, K, Capable>(ctx, f, sc, launch);
      }
    }
  }
  if (plan == kSharedSplit) {
    ctx->chain_path |= IPA_CHAIN_PATH_SPLIT;
    const int rc = fused_batch<ST, INTERP, K, Capable>(ctx, part[0], c, launch);
    return rc ? rc : fused_batch<ST, INTERP, K, Capable>(ctx, part[1], c, launch);
  }
  return launch(f, c, plan);
}

template <typename ST, int INTERP, typename Coord, int K>
static void fused_launch_one(ipa_ctx* ctx, const FusedCall& call, const Coord& coord) {
  // (the dense chain is as it was: fused.hip checks hipGetLastError after its launchers)
  (void)fused_batch<ST, INTERP, K, shared_capable>(ctx, call, coord, [ctx](const FusedCall& f, const auto& c, SharedPlan plan) {
    using Src = SampleRowSrc<ST, INTERP, std::decay_t<decltype(c)>>;
    Weights<float, K * K> w;
    for (int i = 0; i < K * K; i++) w.w[i] = (float)f.kernel[i];
    Src s;
    fused_source(s, f, c);
    WaveParams p = f.p;
    // the tall strips of the shared-record loop only where that loop runs; the per-frame loop, whose rim strips are on
    // the chunked path, keeps the short ones (64 x 4K with frames_wg = 0: 1.53 ms on 144-row strips)
    wave_strips(ctx, p, wave_geom<K, geom_halo<Src, K, false>::value>::OW, f.n_frames, K, false,
                plan == kSharedLoop ? 2 : 0);
    // frames of one strip block run together: map-based remaps share their map rows between
    // frames (L2 fetch traffic -62 % on 16 x 4K), and even without shared rows the order measured
    // ~5 % faster than frame-after-frame
    dim3 grid = wave_grid(ctx, p, f.n_frames, IPA_WPB, true,
                          coord_is_table<typename Src::coord_type>::value || shared_capable<Src, K>::value, false, K);
    dim3 block(64 * IPA_WPB);
    hipLaunchKernelGGL((wave_stencil_kernel<Src, K>), grid, block, 0, ctx->stream, p, s, w);
    chain_launched(ctx, IPA_CHAIN_PATH_RESIDENT, p);
    return IPA_OK;
  });
}

template <typename ST, typename Coord, int K>
static int fused_launch_interp(ipa_ctx* ctx, const FusedCall& f, const Coord& c) {
  switch (f.interp_base) {
    case IPA_INTER_LINEAR: fused_launch_one<ST, kLinear, Coord, K>(ctx, f, c); break;
    case IPA_INTER_CUBIC_CV:
    case IPA_INTER_CUBIC_KEYS: fused_launch_one<ST, kCubic, Coord, K>(ctx, f, c); break;
    default: return kNotCovered;
  }
  return IPA_OK;
}

template <typename ST, int K> static int fused_launch_coord(ipa_ctx* ctx, const FusedCall& f) {
  switch (f.coord_kind) {
    case 0: return fused_launch_interp<ST, MapCoord, K>(ctx, f, f.map);
    case 1: return fused_launch_interp<ST, UndistortCoord, K>(ctx, f, f.und);
    default: return fused_launch_interp<ST, HomographyCoord, K>(ctx, f, f.hom);
  }
}

// float32 frames: any coordinates, bilinear and bicubic; camera frames (toFloatArray ingest), bilinear: uint16 with maps
// or the analytic lens model, uint8 (round 6) with maps
template <int K> static int fused_launch_k(ipa_ctx* ctx, const FusedCall& f) {
  if (f.dst_dt != IPA_F32) return kNotCovered;
  if (f.src_dt == IPA_F32) return fused_launch_coord<float, K>(ctx, f);
  if (f.interp_base != IPA_INTER_LINEAR) return kNotCovered;
  if (f.src_dt == IPA_U16 && f.coord_kind == 0) fused_launch_one<uint16_t, kLinear, MapCoord, K>(ctx, f, f.map);
  else if (f.src_dt == IPA_U16 && f.coord_kind == 1) fused_launch_one<uint16_t, kLinear, UndistortCoord, K>(ctx, f, f.und);
  else if (f.src_dt == IPA_U8 && f.coord_kind == 0) fused_launch_one<uint8_t, kLinear, MapCoord, K>(ctx, f, f.map);
  else return kNotCovered;
  return IPA_OK;
}

}  // namespace ipa

#ifdef IPA_FUSED_K
#define IPA_CAT2(a, b) a##b
#define IPA_CAT(a, b) IPA_CAT2(a, b)
int IPA_CAT(ipa_fused_launch_k, IPA_FUSED_K)(ipa_ctx* ctx, const ipa::FusedCall& f) {
  return ipa::fused_launch_k<IPA_FUSED_K>(ctx, f);
}
// the plain float32 filter on the same skeleton (rows straight from memory; declared in wave_stencil.hpp)
int IPA_CAT(ipa_wave_conv_launch_k, IPA_FUSED_K)(ipa_ctx* ctx, const ipa::WaveParams& p0,
                                                 const ipa::LoadRowSrc& src, const double* kernel,
                                                 int n_frames) {
  using namespace ipa;
  constexpr int K = IPA_FUSED_K;
  Weights<float, K * K> w;
  for (int i = 0; i < K * K; i++) w.w[i] = (float)kernel[i];
  WaveParams p = p0;
  wave_strips(ctx, p, wave_geom<K, geom_halo<LoadRowSrc, K, false>::value>::OW, n_frames, K, false,
              pipe_capable<LoadRowSrc, K>::value && IPA_PIPE ? 1 : 0);
  dim3 grid = wave_grid(ctx, p, n_frames, IPA_WPB, true, false, true), block(64 * IPA_WPB);
  hipLaunchKernelGGL((wave_stencil_kernel<LoadRowSrc, K>), grid, block, 0, ctx->stream, p, src, w);
  IPA_HIP(ctx, hipGetLastError());
  return IPA_OK;
}
#endif
