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

// Homography batches on the shared-record loop (knob stored_coords: from that many frames): its double coordinates (two
// fused-multiply-add chains and a division per pixel) are evaluated ONCE per (matrix, geometry) into the plan buffer
// (stored_coords.hpp) and the record producers read them as a table - the C3 chain spent a third of its time evaluating
// them once per four frames.
template <typename ST, int INTERP, typename Coord, int K>
static void fused_launch_one(ipa_ctx* ctx, const FusedCall& f, const Coord& c) {
  using Src = SampleRowSrc<ST, INTERP, Coord>;
  FusedCall part[2];
  const SharedPlan plan = fused_plan(ctx, shared_capable<Src, K>::value, f, part);
  if constexpr (std::is_same<Coord, HomographyCoord>::value && shared_capable<Src, K>::value) {
    if (ctx->tune.stored_coords > 0 && f.n_frames >= ctx->tune.stored_coords && plan != kPerFrameLoop) {
      StoredCoord<double> sc;
      if (stored_coords_prepare<Coord>(ctx, c, f.p.dh, f.p.dw, &sc) == 0) {
        fused_launch_one<ST, INTERP, StoredCoord<double>, K>(ctx, f, sc);
        return;
      }
    }
  }
  if (plan == kSharedSplit) {
    fused_launch_one<ST, INTERP, Coord, K>(ctx, part[0], c);
    fused_launch_one<ST, INTERP, Coord, K>(ctx, part[1], c);
    return;
  }
  Weights<float, K * K> w;
  for (int i = 0; i < K * K; i++) w.w[i] = (float)f.kernel[i];
  Src s;
  s.coord = c;
  s.src = f.src; s.src_frame_bytes = f.src_frame_bytes; s.src_bytes = f.src_bytes;
  s.sh = f.sh; s.sw = f.sw; s.spitch = f.spitch;
  s.border = f.border; s.q5 = f.q5; s.cubic_a = f.cubic_a; s.lanczos = nullptr;
  s.cval = (float)f.cval; s.ccval = (float)f.conv_cval; s.map_vec = f.map_vec;
  WaveParams p = f.p;
  using G = wave_geom<K, geom_halo<Src, K, false>::value>;
  p.strips_x = (p.dw + G::OW - 1) / G::OW;
  // the tall strips of the shared-record loop only where that loop runs; the per-frame loop, whose rim strips are on the
  // chunked path, keeps the short ones (64 x 4K with frames_wg = 0: 1.53 ms on 144-row strips)
  p.strip_h = wave_strip_height(ctx, p.dh, p.dw, f.n_frames, K, false, plan == kSharedLoop ? 2 : 0, p.strips_x);
  p.strips = (unsigned)p.strips_x * (unsigned)((p.dh + p.strip_h - 1) / p.strip_h);
  // frames of one strip block run together: map-based remaps share their map rows between
  // frames (L2 fetch traffic -62 % on 16 x 4K), and even without shared rows the order measured
  // ~5 % faster than frame-after-frame
  dim3 grid = wave_grid(ctx, p, f.n_frames, IPA_WPB, true,
                        coord_is_table<Coord>::value || shared_capable<Src, K>::value, false, K);
  dim3 block(64 * IPA_WPB);
  hipLaunchKernelGGL((wave_stencil_kernel<Src, K>), grid, block, 0, ctx->stream, p, s, w);
}

template <typename ST, typename Coord, int K>
static int fused_launch_interp(ipa_ctx* ctx, const FusedCall& f, const Coord& c) {
  switch (f.interp_base) {
    case IPA_INTER_LINEAR: fused_launch_one<ST, kLinear, Coord, K>(ctx, f, c); break;
    case IPA_INTER_CUBIC_CV:
    case IPA_INTER_CUBIC_KEYS: fused_launch_one<ST, kCubic, Coord, K>(ctx, f, c); break;
    default:
      IPA_UNSUPPORTED(ctx, "fused remap+filter supports INTER_LINEAR and the two bicubics");
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

template <int K> static int fused_launch_k(ipa_ctx* ctx, const FusedCall& f) {
  if (f.src_dt == IPA_F32 && f.dst_dt == IPA_F32) return fused_launch_coord<float, K>(ctx, f);
  if (f.src_dt == IPA_U16 && f.dst_dt == IPA_F32) {
    // camera frames (toFloatArray ingest): bilinear undistort, map-based or analytic
    if (f.interp_base == IPA_INTER_LINEAR && f.coord_kind == 0) {
      fused_launch_one<uint16_t, kLinear, MapCoord, K>(ctx, f, f.map);
      return IPA_OK;
    }
    if (f.interp_base == IPA_INTER_LINEAR && f.coord_kind == 1) {
      fused_launch_one<uint16_t, kLinear, UndistortCoord, K>(ctx, f, f.und);
      return IPA_OK;
    }
    IPA_UNSUPPORTED(ctx, "fused remap+filter on uint16 frames is built for INTER_LINEAR with "
                         "maps or the analytic lens model; use ipa_remap_dev + ipa_conv2d_dev");
  }
  if (f.src_dt == IPA_U8 && f.dst_dt == IPA_F32 && f.interp_base == IPA_INTER_LINEAR && f.coord_kind == 0) {
    // 8-bit camera frames (round 6): bilinear, map-based
    fused_launch_one<uint8_t, kLinear, MapCoord, K>(ctx, f, f.map);
    return IPA_OK;
  }
  IPA_UNSUPPORTED(ctx, "fused remap+filter: src dtype %d -> dst dtype %d not supported "
                       "(float32->float32 and uint16->float32 are)", f.src_dt, f.dst_dt);
}

}  // namespace ipa

#ifdef IPA_FUSED_K
#define IPA_CAT2(a, b) a##b
#define IPA_CAT(a, b) IPA_CAT2(a, b)
int IPA_CAT(ipa_fused_launch_k, IPA_FUSED_K)(ipa_ctx* ctx, const ipa::FusedCall& f) {
  return ipa::fused_launch_k<IPA_FUSED_K>(ctx, f);
}
// the plain float32 filter on the same skeleton (rows straight from memory)
int IPA_CAT(ipa_wave_conv_launch_k, IPA_FUSED_K)(ipa_ctx* ctx, const ipa::WaveParams& p0,
                                                 const ipa::LoadRowSrc& src, const double* kernel,
                                                 int n_frames) {
  using namespace ipa;
  constexpr int K = IPA_FUSED_K;
  Weights<float, K * K> w;
  for (int i = 0; i < K * K; i++) w.w[i] = (float)kernel[i];
  WaveParams p = p0;
  using G = wave_geom<K, geom_halo<LoadRowSrc, K, false>::value>;
  p.strips_x = (p.dw + G::OW - 1) / G::OW;
  p.strip_h = wave_strip_height(ctx, p.dh, p.dw, n_frames, K, false,
                                pipe_capable<LoadRowSrc, K>::value && IPA_PIPE ? 1 : 0, p.strips_x);
  p.strips = (unsigned)p.strips_x * (unsigned)((p.dh + p.strip_h - 1) / p.strip_h);
  dim3 grid = wave_grid(ctx, p, n_frames, IPA_WPB, true, false, true), block(64 * IPA_WPB);
  hipLaunchKernelGGL((wave_stencil_kernel<LoadRowSrc, K>), grid, block, 0, ctx->stream, p, src, w);
  return IPA_OK;
}
#endif
