"""Seeded scenes of the flat-field tests: the inputs of tests/golden/flat.npz (gen_flat_golden.py
stores what the reference made of them, and a sum per input that catches drift) and the boundary
scenes of test_gpu_flat.py.

Scene (a), `colour_scene`: five (24, 40, 3) colour frames of a vignetted, tinted field and three
background frames, in each of the four element types, for flatFieldFromCloseDistance.

Scene (b), `vignetting_scene`: six uint16 (60, 80) frames of a vignetted field of different
brightness under shot-like noise and three background frames, for flatFieldFromCloseDistance2.
Two frames carry a planted hit (of 2 and of 3 connected pixels), one frame an erroneously dark
block.  The frames are handed over in an order that is not the sorted one.
"""
import numpy as np

ALL_DTYPES = (np.uint8, np.uint16, np.float32, np.float64)

# ---------------------------------------------------------------- scene (a)
A_SHAPE = (24, 40, 3)
A_FRAMES, A_BG = 5, 3


def _top(dtype):
    return 200.0 if np.dtype(dtype) == np.uint8 else 3000.0


def _cast(a, dtype):
    if np.dtype(dtype).kind == 'f':
        return a.astype(dtype)
    return np.clip(np.round(a), 0, np.iinfo(dtype).max).astype(dtype)


def colour_scene(dtype):
    """-> (list of 5 (24, 40, 3) frames, list of 3 background frames)"""
    h, w, _ = A_SHAPE
    rng = np.random.default_rng(7100 + ALL_DTYPES.index(dtype))
    top = _top(dtype)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    r2 = ((x - 21.0) / w) ** 2 + ((y - 10.5) / h) ** 2
    field = (1.0 - 0.9 * r2)[:, :, None] * np.array([0.8, 1.0, 0.6])
    frames = [_cast(0.05 * top + 0.9 * top * field + 0.01 * top * rng.standard_normal(A_SHAPE), dtype)
              for _ in range(A_FRAMES)]
    bgs = [_cast(0.05 * top + 0.004 * top * rng.standard_normal(A_SHAPE), dtype) for _ in range(A_BG)]
    return frames, bgs


# ---------------------------------------------------------------- scene (b)
B_SHAPE = (60, 80)
B_BRIGHT = [0.988, 1.0, 0.994, 0.982, 0.997, 0.991]      # the order handed over: not sorted
B_HITS = ((2, ((20, 33), (20, 34))), (4, ((41, 52), (42, 52), (42, 53))))
B_DARK = (3, (slice(46, 54), slice(12, 22)))             # (frame, block): erroneously dark; the dimmest frame
# seeds of the six frames and of the backgrounds; searched once (gen_flat_golden.py asserts the
# conditions: the square-root fit succeeds, at most 1 % of any frame's decisions lie within 1e-5 of
# a threshold and none of them on the [::10, ::10] grid)
B_SEEDS = [7200, 7201, 7202, 7203, 7204, 7205]
B_BG_SEED = 7290
B_NSTD = 6


def vignetting_scene():
    """-> (list of 6 uint16 (60, 80) frames, list of 3 uint16 background frames)"""
    h, w = B_SHAPE
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    r2 = ((x - 41.0) / w) ** 2 + ((y - 28.0) / h) ** 2
    field = 200.0 + 30000.0 * (1.0 - 1.3 * r2)
    frames = []
    for k, b in enumerate(B_BRIGHT):
        rng = np.random.default_rng(B_SEEDS[k])
        sig = 400.0 + b * field
        f = sig + np.sqrt(sig) * 1.5 * rng.standard_normal((h, w))
        for kk, pts in B_HITS:
            if kk == k:
                for p in pts:
                    f[p] += 9000.0
        if B_DARK[0] == k:
            f[B_DARK[1]] *= 0.6
        frames.append(_cast(f, np.uint16))
    rng = np.random.default_rng(B_BG_SEED)
    bgs = [_cast(400.0 + 6.0 * rng.standard_normal((h, w)), np.uint16) for _ in range(3)]
    return frames, bgs


# ---------------------------------------------------------------- kernel scenes
MEAN_N = [1, 2, 5, 64, 65]


def frame(h, w, dtype, seed, special=True):
    """a frame of values between 0 and the type's top; float types with NaN, +inf and -inf"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0, _top(dtype), (h, w))
    if np.dtype(dtype).kind == 'f' and special and h * w > 8:
        a.ravel()[[1, 3, 4]] = [np.nan, np.inf, -np.inf]
    return _cast(a, dtype)


def stack(n, h, w, dtype, seed):
    rng = np.random.default_rng(seed)
    a = rng.uniform(0, _top(dtype), (n, h, w))
    if np.dtype(dtype).kind == 'f' and h * w > 8:
        a[0].ravel()[1] = np.nan
        a[n - 1].ravel()[3] = np.inf
        a[n // 2].ravel()[4] = -0.0
    return _cast(a, dtype)


def smooth_frame(h, w, dtype, seed):
    """a field that stays well above zero - the sensitivity divides by its local mean - with noise
    and single outliers for the median to remove"""
    rng = np.random.default_rng(seed)
    top = _top(dtype)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    a = top * (0.5 + 0.3 * np.sin(x / 7.0) * np.cos(y / 5.0)) + 0.02 * top * rng.standard_normal((h, w))
    a.ravel()[::17] += 0.15 * top
    return _cast(a, dtype)
