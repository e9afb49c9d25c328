"""Frames, kernels, masks and case lists shared by tests/test_cpu_conv_refs.py (tests/conv_ref.py
against scipy and the C oracle, no GPU) and tests/test_gpu_conv_paths.py (every kernel behind
ipa_conv2d_dev / ipa_sepconv2d_dev against conv_ref), and the path query of the library
(ipa_conv_path: the launchers' own selection arithmetic, no device needed).
"""
import numpy as np

from .stencil_cases import cached

F32, F64 = np.float32, np.float64
DTYPES = (F32, F64)
CVAL = 0.3   # never 0: a kernel that ignores cval must fail

# paths of ipa_conv_path (include/imgproc_hip.h)
REFUSED = 0
WAVE, TILE, GENERIC = 1, 2, 3
SEP_WAVE, SEP_LDS, SEP_LDS_BIG, SEP_TWO_GENERIC, SEP_ONE_GENERIC = 1, 2, 3, 4, 5
MASKED, BIG_WAVE_OFF = 1, 2   # flag bits of the CONV2D query

# ------------------------------------------------------------------- frames ----
TINY = ((1, 1), (1, 7), (2, 3), (5, 4))               # below the radius of most kernels
TILES = ((31, 127), (32, 128), (33, 129))             # one 128 x 32 tile exactly, and -+ 1
STRIP = ((37, 261),)                                  # crosses the 248 / 256 strip step
LONG = ((5, 140), (70, 150))                          # the first is shorter than a 63-tap radius
FRAMES = TINY + TILES + STRIP
BORDER_FRAMES = ((1, 7), (2, 3), (33, 129))

MODES = ('reflect', 'mirror', 'nearest', 'wrap', 'constant')
# (mode along x, mode along y): the five modes and two mixed pairs
BORDERS = tuple((m, None) for m in MODES) + (('wrap', 'reflect'), ('constant', 'nearest'))


def border_id(b):
    return b[0] if b[1] is None else '%s-y_%s' % b


def path(op, dtype, k0, k1, flags=0):
    """ipa_conv_path for the op NAME ('conv2d', 'sepconv2d', 'sepconv2d_lds')"""
    from imgprocessor_amd import _lib
    from imgprocessor_amd.device import dtype_id
    return _lib.lib().ipa_conv_path(getattr(_lib, 'CONV_' + op.upper()),
                                    dtype_id(np.dtype(dtype)), int(k0), int(k1), int(flags))


def sep_lds_bytes(dtype, nky, nkx):
    """dynamic LDS of the LDS-separable kernel, by the library's own formula"""
    return path('sepconv2d_lds', dtype, nky, nkx)


# --------------------------------------------------------------------- data ----
@cached
def frame(shape, dtype, seed=0):
    """standard_normal times a ramp over the frame (1 .. 4): both signs, sums that cancel"""
    H, W = shape
    rng = np.random.default_rng(1000 + 131 * H + W + seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    ramp = 1.0 + 2.0 * x / max(W - 1, 1) + 1.0 * y / max(H - 1, 1)
    return (rng.standard_normal(shape) * ramp).astype(dtype)


@cached
def batch(shape, dtype, n=3):
    return np.stack([frame(shape, dtype, 17 * (i + 1)) for i in range(n)])


@cached
def kernel2d(kh, kw):
    """signed, not normalised, one tap exactly 0.0 (the last of the first row, or the only
    off-centre corner there is)"""
    k = np.random.default_rng(50 + 17 * kh + kw).standard_normal((kh, kw))
    k[0, kw - 1] = 0.0
    if kh * kw == 1:
        k[0, 0] = -1.5
    return k


@cached
def taps(n, seed=0):
    """signed, not normalised, the second tap exactly 0.0"""
    k = np.random.default_rng(70 + n + seed).standard_normal(n)
    k[1] = 0.0
    return k


def sep_taps(nky, nkx):
    """-> (ky, kx), None for an axis of 0 taps"""
    return (taps(nky, 0) if nky else None, taps(nkx, 1) if nkx else None)


@cached
def rank1_kernel(K):
    """an exact outer product of two signed tap vectors (no zero tap: a zero row is no obstacle
    to the factorisation but says nothing about it either)"""
    rng = np.random.default_rng(90 + K)
    a, b = rng.standard_normal(K) + 2.0, rng.standard_normal(K) - 2.0
    return np.outer(a.astype(F32).astype(F64), b.astype(F32).astype(F64))


@cached
def mask(shape):
    """uint8, ~40 % zeros, the first pixel kept and the last one dropped"""
    H, W = shape
    m = (np.random.default_rng(7 + 31 * H + W).random(shape) > 0.4).astype(np.uint8)
    m.flat[0] = 1
    if m.size > 1:
        m.flat[-1] = 0
    return m


def nonfinite_frame(shape, dtype, window):
    """frame() with a NaN on an edge pixel, a NaN in the interior, one +inf and one -inf, their
    columns further apart than `window` (as many of the four as the width has room for: the edge
    NaN, +inf, -inf, interior NaN in that order)"""
    H, W = shape
    a = frame(shape, dtype, 5).copy()
    step = window + 3
    spots = [((0, 2), np.nan), ((H // 2, 2 + step), np.inf), ((H - 2, 2 + 2 * step), -np.inf),
             ((H // 3, 2 + 3 * step), np.nan)]
    n = 0
    for (r, c), v in spots:
        if c < W:
            a[r, c] = v
            n += 1
    assert n >= 3, (shape, window)
    return a


# -------------------------------------------------------------------- cases ----
# conv2d: (dtype, kh, kw, flags, path).  flags: MASKED, BIG_WAVE_OFF
CONV_F32 = tuple((F32, K, K, 0, WAVE) for K in (3, 5, 7, 9, 11)) + \
    tuple((F32, K, K, MASKED, TILE) for K in (3, 5, 7, 9, 11)) + \
    tuple((F32, K, K, BIG_WAVE_OFF, TILE) for K in (9, 11))
CONV_F64 = tuple((F64, K, K, f, TILE) for K in (3, 5, 7) for f in (0, MASKED)) + \
    tuple((F64, K, K, 0, GENERIC) for K in (9, 11))
GENERIC_SHAPES = ((13, 13), (12, 12), (1, 9), (9, 1), (6, 4), (3, 7))
CONV_GENERIC = tuple((dt, kh, kw, f, GENERIC) for dt in DTYPES for kh, kw in GENERIC_SHAPES
                     for f in (0, MASKED))
CONV_CASES = CONV_F32 + CONV_F64 + CONV_GENERIC

# every pair stands on two kernels: (case, case)
CONV_BOUNDARIES = (
    ((F32, 11, 11, 0), (F32, 13, 13, 0)),                 # wave | generic
    ((F32, 11, 11, 0), (F32, 12, 12, 0)),
    ((F32, 7, 7, 0), (F32, 7, 7, MASKED)),                # wave | tile: the mask
    ((F32, 9, 9, 0), (F32, 9, 9, BIG_WAVE_OFF)),          # wave | tile: the knob
    ((F32, 11, 11, 0), (F32, 11, 11, BIG_WAVE_OFF)),
    ((F32, 11, 11, MASKED), (F32, 13, 13, MASKED)),       # tile | generic
    ((F64, 7, 7, 0), (F64, 9, 9, 0)),                     # float64 tile | generic
    ((F64, 7, 7, MASKED), (F64, 9, 9, MASKED)),
    ((F32, 3, 3, 0), (F32, 3, 7, 0)),                     # square | not
)


def conv_id(c):
    dt, kh, kw, flags = c[:4]
    return '%s-%dx%d%s%s' % (np.dtype(dt).name, kh, kw, '-mask' if flags & MASKED else '',
                             '-big_wave0' if flags & BIG_WAVE_OFF else '')


# sepconv2d: (dtype, nky, nkx, path); 0 taps = axis skipped
SEP_F32 = tuple((F32, n, n, SEP_WAVE) for n in (3, 5, 7, 9)) + (
    (F32, 11, 11, SEP_LDS), (F32, 3, 9, SEP_LDS), (F32, 9, 3, SEP_LDS),
    (F32, 33, 33, SEP_LDS), (F32, 35, 35, SEP_LDS_BIG),
    (F32, 63, 63, SEP_LDS_BIG), (F32, 65, 65, SEP_TWO_GENERIC),
    (F32, 5, 0, SEP_LDS), (F32, 0, 5, SEP_LDS),
    (F32, 65, 0, SEP_ONE_GENERIC), (F32, 0, 65, SEP_ONE_GENERIC))
SEP_F64 = ((F64, 3, 3, SEP_LDS_BIG), (F64, 9, 9, SEP_LDS_BIG), (F64, 45, 45, SEP_LDS_BIG),
           (F64, 47, 47, SEP_TWO_GENERIC), (F64, 45, 3, SEP_LDS_BIG), (F64, 3, 45, SEP_LDS_BIG),
           (F64, 9, 0, SEP_LDS_BIG))
SEP_CASES = SEP_F32 + SEP_F64

SEP_BOUNDARIES = (
    ((F32, 9, 9), (F32, 11, 11)),      # wave | LDS
    ((F32, 9, 9), (F32, 9, 3)),        # wave | LDS: unequal taps
    ((F32, 33, 33), (F32, 35, 35)),    # 64 KiB
    ((F32, 63, 63), (F32, 65, 65)),    # kSepMaxTaps
    ((F64, 45, 45), (F64, 47, 47)),    # 150 KiB
    ((F32, 63, 0), (F32, 65, 0)),      # one axis: LDS | one generic launch
    ((F32, 0, 63), (F32, 0, 65)),
    ((F32, 65, 65), (F32, 65, 0)),     # two generic launches | one
)


def sep_id(c):
    return '%s-%dx%d' % (np.dtype(c[0]).name, c[1], c[2])


def sep_frames(nky, nkx):
    """short taps: every frame; long ones: the two LONG frames and one below every radius"""
    return FRAMES if max(nky, nkx) <= 11 else LONG + ((2, 3),)


def conv_inputs(case, shape):
    """-> (frame, kernel, mask or None) of a CONV_CASES entry on a frame shape"""
    dt, kh, kw, flags = case[:4]
    return frame(shape, dt), kernel2d(kh, kw), mask(shape) if flags & MASKED else None


def conv_runs(case):
    """-> [(shape, (mode, mode_y))]: every frame with 'reflect', the border frames with the
    other four modes and the two mixed pairs"""
    return [(s, BORDERS[0]) for s in FRAMES] + [(s, b) for b in BORDERS[1:] for s in BORDER_FRAMES]


def sep_runs(case):
    fr = sep_frames(case[1], case[2])
    bfr = BORDER_FRAMES if fr is FRAMES else fr
    return [(s, BORDERS[0]) for s in fr] + [(s, b) for b in BORDERS[1:] for s in bfr]


# --------------------------------------------------------------- comparison ----
def compare(got, want, bnd, what=''):
    """asserts the non-finite pattern of `got` equal to the float64 reference `want` and every
    finite pixel within its bound `bnd`; -> the worst err / bound (0 where both are 0)"""
    got = np.asarray(got, dtype=F64)
    assert got.shape == want.shape == bnd.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), '%s: NaN pattern differs (%d vs %d)' % (
        what, np.isnan(got).sum(), np.isnan(want).sum())
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]) and not np.isinf(got[~inf]).any(), \
        '%s: inf pattern differs' % what
    fin = np.isfinite(want)
    if not fin.any():
        return 0.0
    err = np.where(fin, np.abs(np.where(fin, got, 0.0) - np.where(fin, want, 0.0)), 0.0)
    b = np.where(fin, bnd, 1.0)
    assert np.isfinite(b).all(), '%s: a finite pixel with a non-finite bound' % what
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err == 0.0, 0.0, err / b)
    worst = float(ratio.max())
    if worst > 1.0:
        i = np.unravel_index(np.argmax(ratio), ratio.shape)
        raise AssertionError('%s: %d of %d pixels beyond the bound, worst at %s: got %r want %r, '
                             'err %.3g = %.3g x bound' % (what, (ratio > 1.0).sum(), ratio.size, i,
                                                         got[i], want[i], err[i], worst))
    return worst
