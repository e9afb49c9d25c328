#!/usr/bin/env python3
"""Generate tests/golden/nlf.npz: noise level functions and signal-to-noise maps as the reference
computes them (camera/NoiseLevelFunction.py, measure/SNR/SNR.py).  Runs only where the reference
source exists.

The reference runs unchanged under the throw-away stand-ins of gen_ste_golden.py (numba shim,
constants-only cv2); in this generator only, ``np.asfarray`` - which numpy 2 dropped and the
reference calls - is put back as ``np.asarray(a, dtype=float64)``.

The inputs are the seeded scenes of tests/nlf_cases.py: the fixture holds what the reference made
of them (x, y, weights; fitted function values on a grid; SNR maps of small frames) and one sum
per input that catches a drifting scene.  Arrays only.

Bins the reference leaves uninitialised (np.empty: fewer than min_len pixels) are stored as NaN
in x and y; their weight is 0.

    python tests/golden/gen_nlf_golden.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden import install_shim  # noqa: E402
from gen_ste_golden import install_standins  # noqa: E402
import nlf_cases as nc  # noqa: E402

warnings.filterwarnings('ignore')


def _in_sum(*arrs):
    return np.array([np.asarray(a, dtype=np.float64).sum() for a in arrs if a is not None])


def main():
    if not hasattr(np, 'asfarray'):
        np.asfarray = lambda a, dtype=np.float64: np.asarray(a, dtype=dtype)
    install_shim()
    install_standins()
    from imgProcessor.camera import NoiseLevelFunction as N
    from imgProcessor.measure.SNR.SNR import SNR, getBackgroundLevel

    out = {}
    for name in nc.GOLDEN_NLF:
        img, img2, kw = nc.nlf_inputs(name)
        x, y, weights, signal = N.calcNLF(img, img2, **kw)
        empty = weights == 0
        if 'mn_mx_nbins' not in kw:
            x, y = np.where(empty, np.nan, x), np.where(empty, np.nan, y)
        p = 'nlf_%s_' % name
        out[p + 'x'], out[p + 'y'], out[p + 'weights'] = x, y, weights
        out[p + 'in_sum'] = _in_sum(img, img2)
        out[p + 'signal_sum'] = np.array(signal.sum())
    # a caller's signal: the reference's own median, handed back in
    img, img2, _ = nc.nlf_inputs('pair_uint16')
    sig = N.calcNLF(img)[3]
    x, y, weights, _ = N.calcNLF(img, img2, signal=sig)
    out['nlf_signal_x'], out['nlf_signal_y'], out['nlf_signal_weights'] = \
        np.where(weights == 0, np.nan, x), np.where(weights == 0, np.nan, y), weights

    # the fit: function values over the fitted range, never parameters
    f = nc.fit_frame()
    x, y, weights, _ = N.calcNLF(f)
    params, fn, i = N._evaluate(x, y, weights)
    assert params is not None, 'the fit scene fell back to the polynomial'
    grid = np.linspace(x[i][0], x[i][-1], 50)
    out['fit_in_sum'] = _in_sum(f)
    out['fit_x'], out['fit_y'], out['fit_weights'] = \
        np.where(weights == 0, np.nan, x), np.where(weights == 0, np.nan, y), weights
    out['fit_valid'] = i
    out['fit_grid'], out['fit_values'] = grid, fn(grid)
    out['fit_params'] = np.asarray(params)

    imgs1, imgs2 = nc.estimate_pairs()
    x, fn, y_avg, y_vals, w_vals, params, i = N.estimateFromImages(imgs1, imgs2)
    assert params is not None
    grid = np.linspace(x[i][0], x[i][-1], 50)
    out['est_in_sum'] = _in_sum(*(imgs1 + imgs2))
    out['est_x'], out['est_y_avg'], out['est_y_vals'], out['est_w_vals'] = x, y_avg, y_vals, w_vals
    out['est_grid'], out['est_values'] = grid, fn(grid)

    # SNR maps
    f1, f2 = nc.snr_frames(nc.SNR_SHAPE)
    out['snr_in_sum'] = _in_sum(f1, f2)
    tri = lambda s: N.boundedFunction(s, *nc.SNR_TRIPLE)   # noqa: E731
    for form in nc.SNR_FORMS:
        pair, kw = nc.snr_kwargs(form, tri)
        out['snr_' + form] = SNR(f1, f2 if pair else None, **kw)
    g1, g2 = nc.snr_frames(nc.SNR_NLF_SHAPE, seed=84)
    out['snr_nlf_in_sum'] = _in_sum(g1, g2)
    out['snr_nlf_one'] = SNR(g1)[::nc.SNR_NLF_STEP, ::nc.SNR_NLF_STEP]
    out['snr_nlf_pair'] = SNR(g1, g2, bg=100.0)[::nc.SNR_NLF_STEP, ::nc.SNR_NLF_STEP]
    out['bg_level'] = np.array([getBackgroundLevel(np.asarray(a, dtype=np.float64))
                                for a in (f1, g1, g2)])
    path = os.path.join(HERE, 'nlf.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes, %d arrays)' % (path, os.path.getsize(path), len(out)))


if __name__ == '__main__':
    main()
