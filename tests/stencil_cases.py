"""Frames, masks and windows shared by tests/test_cpu_stencil_refs.py (references against the C
oracle, no GPU) and tests/test_gpu_stencil_paths.py (kernels against both), and the path query
of the library (ipa_stencil_path: the launchers' own selection arithmetic, no device needed).
"""
import functools

import numpy as np

from .conftest import synth

SMALL = ((1, 1), (1, 70), (70, 1), (5, 63), (9, 64), (13, 65), (37, 130))
WIDE = ((50, 257), (50, 259))   # 256-px tiles; the odd width leaves the 16-byte stores
DTYPES = (np.float32, np.float64)

# paths of ipa_stencil_path (include/imgproc_hip.h)
REFUSED = 0
STD_WAVE, STD_TILE, STD_GENERIC = 1, 2, 3
MEAN_COLS, MEAN_WAVE = 1, 2
MEDIAN_WAVE = 1
NANMAX_SEP, NANMAX_GENERIC = 1, 2
CDD_TWO_PASS, CDD_DIRECT = 1, 2
PIU_SEP, PIU_GENERIC = 1, 2
MT_NETWORK, MT_COUNTING = 1, 2
VYG_TILED, VYG_EXPANDED_TILE, VYG_EXPANDED_GENERIC = 1, 2, 3


def path(op, dtype, kx, ky=0):
    """ipa_stencil_path for the op NAME ('local_std', 'masked_mean_fill', ...)"""
    from imgprocessor_amd import _lib
    from imgprocessor_amd.device import dtype_id
    return _lib.lib().ipa_stencil_path(getattr(_lib, 'STENCIL_' + op.upper()),
                                       dtype_id(np.dtype(dtype)), int(kx), int(ky))


def boundary(op, dtype, lo=2, hi=400, step=1, **kw):
    """-> (last window of the path `lo` takes, first window of the next path), found by walking
    the query upwards from lo"""
    first = path(op, dtype, lo, **kw)
    for k in range(lo + step, hi, step):
        if path(op, dtype, k, **kw) != first:
            return k - step, k
    raise AssertionError('%s %s: one path from %d to %d' % (op, dtype, lo, hi))


def var_y_boundary(dtype, kx):
    """-> (last ky the tiled kernel takes, first it does not); ky is odd"""
    first = path('var_y_gauss', dtype, kx, 1)
    assert first == VYG_TILED
    for ky in range(3, 400, 2):
        if path('var_y_gauss', dtype, kx, ky) != first:
            return ky - 2, ky
    raise AssertionError('var_y_gauss: tiled up to ky 399')


def stdy_for(ky):
    """an upper stdyrange for which filters/varYSizeGaussianFilter derives exactly ky taps"""
    return (ky + 0.5) / 2.5


# ------------------------------------------------------------------- frames ----
def signed(shape, seed, dtype=np.float64):
    """synth() moved to [-2, 2]: values of both signs"""
    return ((synth(shape, seed, np.float64) - 0.5) * 4).astype(dtype)


def quantised(shape, seed, dtype=np.float64):
    """8 levels, -0.75 ... 1.0 in steps of 0.25: nearly every window has ties, exact zeros of
    both signs included"""
    q = (np.minimum(np.floor(synth(shape, seed, np.float64) * 8), 7) - 3) / 4
    q = q.astype(dtype)
    z = np.flatnonzero(q == 0)
    q.flat[z[::2]] = -0.0
    return q


def special(shape, seed, dtype=np.float64):
    """quantised() with +-inf sprinkled in"""
    q = quantised(shape, seed, dtype)
    rng = np.random.default_rng(seed + 1000)
    r = rng.random(shape)
    q[r < 0.03] = np.inf
    q[r > 0.97] = -np.inf
    return q


def with_nans(shape, seed, dtype=np.float64):
    """signed() with isolated NaNs, two of them on the rim"""
    a = signed(shape, seed, dtype)
    a[np.random.default_rng(seed + 2000).random(shape) < 0.01] = np.nan
    a[0, 0] = a[-1, -1] = np.nan
    return a


FRAME_KINDS = {'signed': signed, 'quantised': quantised, 'special': special, 'nans': with_nans}


def frame(kind, shape, dtype, seed=7):
    return FRAME_KINDS[kind](shape, seed + shape[0] * 31 + shape[1], dtype)


# -------------------------------------------------------------------- masks ----
def mask_block(shape, k, seed=3):
    """30 % masked at random plus an all-masked band of columns wider than the window [j-k, j+k)
    (up to half the frame): windows with no unmasked pixel where the frame has room for one"""
    H, W = shape
    m = np.random.default_rng(seed + H * 31 + W).random(shape) < 0.3
    bw = min(2 * k + 3, W // 2)
    m[:, W // 4:W // 4 + bw] = True
    return m


def mask_single(shape, k):
    """everything masked but a lattice of single pixels 2k + 1 apart: a window [i-k, i+k) holds
    exactly one unmasked pixel, or none"""
    H, W = shape
    m = np.ones(shape, bool)
    m[min(k, H - 1)::2 * k + 1, min(k, W - 1) // 2::2 * k + 1] = False
    return m


def window_counts(m, k):
    """number of unmasked pixels in the clipped window [i-k, i+k) x [j-k, j+k) of every pixel"""
    H, W = m.shape
    S = np.pad((~m).astype(np.int64).cumsum(0).cumsum(1), ((1, 0), (1, 0)))
    i, j = np.arange(H)[:, None], np.arange(W)[None, :]
    r0, r1 = np.maximum(i - k, 0), np.minimum(i + k, H)
    c0, c1 = np.maximum(j - k, 0), np.minimum(j + k, W)
    return S[r1, c1] - S[r0, c1] - S[r1, c0] + S[r0, c0]


def mask(kind, shape, k):
    return mask_block(shape, k) if kind == 'block' else mask_single(shape, k)


# ------------------------------------------------- nan_max / closest / piu ----
def nan_max_frame(shape, k, dtype):
    """NaNs on the rim, an all-NaN block wider than the window, -inf as the only number of a
    region, isolated NaNs"""
    a = with_nans(shape, 11, dtype)
    H, W = shape
    a[0, :] = np.nan
    a[:, -1] = np.nan
    bw = min(2 * k + 3, W // 2)
    a[:, W // 4:W // 4 + bw] = np.nan
    if W >= 8:
        a[H // 2, W // 4 + bw // 2] = -np.inf   # alone in its neighbourhood
    return a


def closest_frames(shape):
    """-> {name: uint8 array}.  On (5, 600) two set pixels, (2, 10) and (0, 590), 580 columns
    apart: every distance 1 ... 300 along a row and every diagonal offset (4, d) occurs, none
    within reach of both pixels for ksize <= 300"""
    H, W = shape
    empty = np.zeros(shape, np.uint8)
    two = empty.copy()
    two[H // 2, min(10, W - 1)] = 1
    two[0, max(W - 10, 0)] = 1
    rnd = (np.random.default_rng(5).random(shape) > 0.99).astype(np.uint8)
    rnd[0, 0] = rnd[-1, -1] = 1
    return {'empty': empty, 'two': two, 'random': rnd}


def closest_cases():
    """-> [(shape, frame name, ksize, output dtype, oracle too)].  The oracle visits the whole
    +-ksize window of every pixel, (2 ksize + 1)**2 steps: it is asked where a path or the
    sentinel of the byte row distances is at stake, the plain reference everywhere."""
    out = []
    for shape in ((1, 1), (5, 600), (37, 130)):
        for name in ('empty', 'two', 'random'):
            for ks in (1, 253, 254, 255, 300):
                for dt in (np.uint16, np.float64):
                    orc = ks == 1 or (ks in (254, 255) and (
                        (shape == (5, 600) and name == 'two') or
                        (shape == (37, 130) and name == 'random' and dt == np.uint16) or
                        shape == (1, 1)))
                    out.append((shape, name, ks, dt, orc))
    return out


def piu_frame(shape, dtype):
    """signed frame with a NaN in the middle (a NaN centre for one pixel, a NaN neighbour for
    those around it)"""
    a = signed(shape, 13, dtype)
    a[shape[0] // 2, shape[1] // 2] = np.nan
    return a


def piu_sigma_maps(shape):
    y, x = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    return 0.8 + 0.05 * y + 0.01 * x, 1.5 + 0.02 * x


def median_threshold_frame(kind, shape, dtype):
    """'zeros': quantised (ties, medians that are exactly +-0); 'spiky': positive with outliers"""
    if kind == 'zeros':
        return quantised(shape, 17 + shape[1], dtype)
    a = 0.2 + synth(shape, 19 + shape[1], np.float64)
    a.flat[::7] *= 4
    return a.astype(dtype)


def var_y_frame(shape, dtype):
    a = signed(shape, 23, dtype)
    a[shape[0] // 3, shape[1] // 4:shape[1] // 4 + 20] = np.nan   # a NaN run
    a[-1, -3:] = np.nan
    return a


def cached(fn):
    """references are computed once per argument tuple and handed out read-only"""
    @functools.lru_cache(maxsize=None)
    def wrapped(*args):
        out = fn(*args)
        for o in (out if isinstance(out, tuple) else (out,)):
            o.setflags(write=False)
        return out
    return wrapped
