"""Seeded scenes of the dark-current tests: the inputs of tests/golden/dark.npz
(gen_dark_golden.py stores what the reference made of them, and a sum per input that catches
drift) and the boundary scenes of test_gpu_dark.py.

Scene (a), `dark_series`: 16 dark frames over 6 exposure times.  The frame counts per time are
1, 2, 3, 3, 3 and 4 - one single frame, one pair, and 16 - 3 = 13 frames over the other four, so
one of them has four (a second addImg).  Read noise of sigma 3 counts; two hits, of 2 and of 3
connected pixels, in different frames; a band of rows whose ascent is below MIN_ASCENT; a block
above MX_INTENSITY in the two longest exposures; one pixel above it in all exposures but one
(n = 1) and one in all (n = 0).

Scene (b), `fit_pair`: two exposures (and a third frame for addImg) of nlf_cases.fit_frame's
kind, on which the bounded square-root fit succeeds.
"""
import numpy as np

try:
    from .nlf_cases import gradient, FIT_SHAPE
except ImportError:   # the generator runs outside the package
    from nlf_cases import gradient, FIT_SHAPE

H, W = 24, 40
DTYPES = (np.uint16, np.float32, np.float64)
# exposure time of every frame, in the order the frames are handed over (not sorted, not grouped)
EXP_TIMES = [8.0, 1.0, 32.0, 2.0, 16.0, 4.0, 8.0, 32.0, 4.0, 16.0, 32.0, 8.0, 2.0, 16.0, 32.0, 4.0]
MX_INTENSITY = 260.0
MIN_ASCENT = 0.15
SATURATED = 300.0
BAND = slice(18, 21)                     # rows whose level falls with the exposure time
BLOCK = (slice(2, 4), slice(30, 32))     # saturated at t = 16 and t = 32
PX_N1 = (12, 5)                          # saturated unless t = 1
PX_N0 = (13, 20)                         # always saturated
# (frame index, pixels): hits of 2 and 3 connected pixels
HITS = ((6, ((8, 10), (8, 11))), (13, ((15, 25), (16, 25), (16, 26))))


# One seed per frame.  Whether scipy's curve_fit gives up on the square root - so that the noise
# level function of a group is the polynomial, the branch this scene is for - depends on the noise
# of the group's first two frames: about two in three pairs of flat dark frames take it.  The
# seeds were searched once for pairs that do; gen_dark_golden.py asserts the branch.
FRAME_SEEDS = [400, 401, 2902, 403, 1904, 405, 406, 407, 408, 409, 410, 411, 412, 413, 414, 415]


def dark_frame(k, seed=None):
    """frame k of the series in float64, integer-valued (every dtype stores the same numbers)"""
    rng = np.random.default_rng(FRAME_SEEDS[k] if seed is None else seed)
    t = EXP_TIMES[k]
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    offset = 200.0 + 0.1 * x + 0.05 * y
    ascent = 0.3 + 0.05 * np.sin(x / 5.0)
    ascent[BAND] = 0.0
    f = offset + ascent * t + 3.0 * rng.standard_normal((H, W))
    for kk, pts in HITS:
        if kk == k:
            for p in pts:
                f[p] += 80.0
    if t >= 16.0:
        f[BLOCK] = SATURATED
    if t != 1.0:
        f[PX_N1] = SATURATED
    f[PX_N0] = SATURATED
    return np.clip(np.round(f), 0, 65535)


def dark_series(dtype=np.uint16):
    """-> (exposure times, list of 16 (H, W) frames)"""
    return list(EXP_TIMES), [dark_frame(k).astype(dtype) for k in range(len(EXP_TIMES))]


def fit_pair():
    """-> three uint16 frames of the scene the square-root fit succeeds on"""
    return [gradient(FIT_SHAPE[0], FIT_SHAPE[1], 500 + i, np.uint16) for i in range(3)]


# ---------------------------------------------------------------- kernel scenes
SHAPES = [(1, 1), (3, 67), (33, 130)]
# the fit also where a row spans several tiles of lanes that own 4 (uint8, uint16) or 2 (float32) pixels
REGRESS_SHAPES = SHAPES + [(5, 520)]
# (both sides of every step of the fit's register count, stack_linregress_kernel<T, 4 | 8 | 16 | ...>:
# 4 | 5 and 8 | 9 as well as 16 | 17 - stacks of 5 to 8 frames are an instantiation of their own)
T_VALUES = [2, 3, 4, 5, 8, 9, 16, 17, 64]
ALL_DTYPES = (np.uint8, np.uint16, np.float32, np.float64)


def regress_stack(T, h, w, dtype, seed):
    """-> (times, (T, h, w) stack, mx_intensity): lines under noise with rising, flat and falling
    pixels; samples above mx_intensity so that pixels keep n = 0, 1, 2 and more samples; for float
    types NaN, +inf and -inf samples"""
    rng = np.random.default_rng(seed)
    top = 200.0 if np.dtype(dtype) == np.uint8 else 3000.0
    mx = 0.8 * top
    times = np.sort(rng.uniform(0.5, 40.0, T))
    rng.shuffle(times)
    offset = rng.uniform(0.05, 0.3, (h, w)) * top
    ascent = rng.uniform(-0.004, 0.008, (h, w)) * top
    ascent.ravel()[::5] = 0.0
    st = offset + ascent * times[:, None, None] + 0.002 * top * rng.standard_normal((T, h, w))
    st = np.clip(st, 0, mx)
    n_px = h * w
    flat = st.reshape(T, n_px)
    if n_px > 3:
        flat[rng.random((T, n_px)) < 0.05] = top * 0.9
        # pixels with exactly 0, 1 and 2 valid samples
        for j, keep in enumerate((0, 1, 2)):
            p = (7 * j + 3) % n_px
            flat[:, p] = np.minimum(flat[:, p], mx)
            flat[rng.permutation(T)[keep:], p] = top * 0.95
    if np.dtype(dtype).kind == 'f':
        if n_px > 8:
            for v in (np.nan, np.inf, -np.inf):
                flat[rng.integers(0, T), rng.integers(0, n_px)] = v
        return times, st.astype(dtype), mx
    return times, np.round(st).astype(dtype), mx
