// fused_sep_c.hip - the remap ALONE on the marching strips: wave_sep_kernel with K = 1 (no filter, no halo;
// fused_sep_impl.hpp, wave_sep.hpp::sep_geom<1>) - the standalone bilinear remap of frame batches (knob strip_remap)
#include "fused_sep_impl.hpp"

int ipa_fused_sep_launch_c(ipa_ctx* ctx, const ipa::FusedCall& f, const ipa::FusedSep& q) {
  return ipa::fused_sep_k<1>(ctx, f, q);
}

// integer frames into their own type with cv2's arithmetic (wave_pipe.hpp CV16: 16U float weights / 8U fixed point): maps.
// The kernel writes such results on the shared-record loop alone, rim strips included: returns 1 - nothing launched - unless
// the plan and wave_grid put every strip of every launch (the whole batch, or its head and tail) on that loop; else the
// status of the launches.
template <typename T> static int strip_remap_int_launch(ipa_ctx* ctx, const ipa::FusedCall& f) {
  using namespace ipa;
  using Src = SampleRowSrc<T, kLinear, MapCoord>;
  FusedCall part[2];
  const SharedPlan plan = fused_plan(ctx, sep_shared<Src, 1>::value && IPA_PIPE_EDGE, f, part);
  if (plan == kPerFrameLoop) return 1;
  if (plan == kSharedLoop) part[0] = f;
  const int parts = plan == kSharedSplit ? 2 : 1;
  for (int i = 0; i < parts; i++) {
    WaveParams p = part[i].p;
    sep_grid<Src, 1>(ctx, p, part[i].n_frames);
    if (!p.frames_wg) return 1;
  }
  Src s;
  fused_source(s, f, f.map);
  s.q5 = 1;       // cv2's 1/32-px coordinates, whatever the flag
  s.ccval = 0.f;  // no filter
  const double one = 1.0;
  for (int i = 0; i < parts; i++) {
    s.src = part[i].src;   // (per part)
    const int rc = launch_sep<Src, 1, T>(ctx, part[i].p, s, &one, &one, part[i].n_frames, 0.f);
    if (rc) return rc;
  }
  return IPA_OK;
}
int ipa_fused_sep_launch_c16(ipa_ctx* ctx, const ipa::FusedCall& f) { return strip_remap_int_launch<uint16_t>(ctx, f); }
int ipa_fused_sep_launch_c8(ipa_ctx* ctx, const ipa::FusedCall& f) { return strip_remap_int_launch<uint8_t>(ctx, f); }
