// wave_sep.hip - the plain separable filter on the wave-marching skeleton (wave_sep.hpp)
#include "launch.hpp"
#include "wave_sep.hpp"

int ipa_wave_sep_launch(ipa_ctx* ctx, const ipa::WaveParams& p, const ipa::LoadRowSrc& src, const double* ky,
                        const double* kx, int taps, int n_frames) {
  using namespace ipa;
  // (src.cval: the constant x border of the intermediate is the filter's own border value)
  const int rc = pick<3, 5, 7, 9>(taps, [&](auto K) {
    return launch_sep<LoadRowSrc, decltype(K)::value>(ctx, p, src, ky, kx, n_frames, src.cval);
  });
  IPA_REQUIRE(ctx, rc != kNotCovered, "internal error: no separable wave kernel for %d taps", taps);
  return rc;
}
