#!/usr/bin/env python3
"""Generate tests/golden/nlm.npz: skimage.restoration.denoise_nl_means (fast_mode=True) next to
the numpy restatement tests/nlm_ref.py.  Runs only where scikit-image 0.18.x is installed.

Per case the file holds the input (float32, exact), skimage's output (rounded to float32), the
float64 exact-exp restatement and the per-pixel margins min_t |D - 5| (float32), plus the
parameters and the measured gap between the two outputs (skimage 0.18 evaluates exp with its own fast_exp, +-3 %).  Before anything is written
the restatement with skimage's fast_exp substituted must match skimage to 1e-7 of the data range
for EVERY case (sigma > 0, the even patch size and the pad-larger-than-image cases included):
that pins the restatement to skimage.  Arrays only.

    python tests/golden/gen_nlm_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from nlm_ref import nlm_ref  # noqa: E402

import skimage  # noqa: E402
from skimage._shared.fast_exp import fast_exp  # noqa: E402
from skimage.restoration import denoise_nl_means  # noqa: E402

assert skimage.__version__.startswith('0.18'), 'the restatement is pinned to scikit-image 0.18.x'


def image(shape, seed):
    """unit-range content: two sinusoids, an edge and noise"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    img = 0.5 + 0.2 * np.sin(2 * np.pi * x / 23) + 0.2 * np.cos(2 * np.pi * y / 17)
    img += 0.15 * (x > 0.6 * shape[1])
    img += 0.05 * rng.standard_normal(shape)
    # multiples of 2**-12: exact in float32, which is how the file stores them
    return np.round(np.clip(img, 0, 1) * 4096) / 4096


fast_exp_v = np.vectorize(lambda v: fast_exp(float(v)), otypes=[np.float64])

# name, shape, seed, patch_size, patch_distance, h, sigma, scale
CASES = [
    ('s7d11', (40, 52), 1, 7, 11, 0.1, 0.0, 1.0),
    ('s7d5', (28, 36), 2, 7, 5, 0.1, 0.0, 1.0),
    ('s5d4', (28, 36), 3, 5, 4, 0.08, 0.0, 1.0),
    ('s6d3', (28, 36), 4, 6, 3, 0.1, 0.0, 1.0),
    ('s7d11h03', (28, 36), 5, 7, 11, 0.3, 0.0, 1.0),
    ('s7d6sig', (28, 36), 6, 7, 6, 0.1, 0.05, 1.0),
    ('wide9x50', (9, 50), 7, 7, 11, 0.1, 0.0, 1.0),
    ('tall50x3', (50, 3), 8, 7, 11, 0.1, 0.0, 1.0),
    ('counts', (28, 36), 9, 7, 5, 0.1, 0.0, 4095.0),
]


def main():
    out = {'names': np.array([c[0] for c in CASES])}
    for name, shape, seed, s, d, h, sigma, scale in CASES:
        img = image(shape, seed) * scale
        h, sigma = h * scale, sigma * scale
        sk = denoise_nl_means(img, patch_size=s, patch_distance=d, h=h, fast_mode=True, sigma=sigma)
        pinned, _ = nlm_ref(img, s, d, h, sigma, exp=fast_exp_v)
        pin = np.abs(pinned - sk).max() / scale
        assert pin <= 1e-7, '%s: restatement with fast_exp differs from skimage by %g' % (name, pin)
        ref, margin = nlm_ref(img, s, d, h, sigma)
        gap = np.abs(ref - sk).max()
        print('%-10s fast_exp restatement vs skimage %.2e, exact exp vs skimage %.2e (x %g)'
              % (name, pin, gap / scale, scale))
        assert np.array_equal(img.astype(np.float32).astype(np.float64), img)
        out[name + '_img'] = img.astype(np.float32)
        out[name + '_skimage'] = sk.astype(np.float32)   # compared to 1.5 x gap, ~1e-3 of the range
        out[name + '_ref'] = ref
        out[name + '_margin'] = margin.astype(np.float32)
        out[name + '_params'] = np.array([s, d, h, sigma], dtype=np.float64)
        out[name + '_gap'] = np.float64(gap)
        out[name + '_pin'] = np.float64(pin)
    np.savez_compressed(os.path.join(HERE, 'nlm.npz'), **out)


if __name__ == '__main__':
    main()
