"""Seeded scenes of the noise-level-function and SNR tests: the inputs of tests/golden/nlf.npz
(gen_nlf_golden.py stores only what the reference made of them, and a sum per input that catches
drift) and the boundary scenes of test_cpu_nlf.py / test_gpu_nlf.py.
"""
import numpy as np

DTYPES = (np.uint8, np.uint16, np.float32, np.float64)
# intensity range per dtype: (lowest level, span)
RANGE = {np.uint8: (20.0, 200.0), np.uint16: (200.0, 3000.0), np.float32: (200.0, 3000.0),
         np.float64: (200.0, 3000.0)}


def _cast(a, dtype):
    if np.dtype(dtype).kind == 'f':
        return a.astype(dtype)
    return np.clip(np.round(a), 0, np.iinfo(dtype).max).astype(dtype)


def gradient(h, w, seed, dtype=np.uint16, k=0.8):
    """a diagonal intensity ramp under shot noise: std = k * sqrt(level)"""
    lo, span = RANGE[dtype]
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = lo + span * (x + y) / max(h + w - 2, 1)
    return _cast(base + np.sqrt(base) * k * rng.standard_normal((h, w)), dtype)


def flat(h, w, seed, dtype=np.uint16, level=1000.0, std=3.0):
    """one level under noise: the pixels fall into few bins"""
    rng = np.random.default_rng(seed)
    return _cast(level + std * rng.standard_normal((h, w)), dtype)


def uniform_int(h, w, seed, dtype=np.uint8, lo=50, hi=90):
    """integers spread evenly over [lo, hi]: mean +- 3 std lies outside, so the range is
    [min, max], the step is exactly 1.0 and every pixel sits on an edge (two bins)"""
    rng = np.random.default_rng(seed)
    return rng.integers(lo, hi + 1, (h, w)).astype(dtype)


# name -> (scene function, arguments, calcNLF keywords); 'pair' adds a second exposure (seed + 100)
GOLDEN_NLF = {}
for _i, _dt in enumerate(DTYPES):
    _n = np.dtype(_dt).name
    GOLDEN_NLF['one_' + _n] = (gradient, (64, 96, 10 + _i, _dt), {})
    GOLDEN_NLF['pair_' + _n] = (gradient, (64, 96, 20 + _i, _dt), {'pair': True})
GOLDEN_NLF['rms_uint16'] = (gradient, (64, 96, 30, np.uint16), {'averageFn': 'RMS'})
GOLDEN_NLF['rms_pair_float32'] = (gradient, (64, 96, 31, np.float32), {'averageFn': 'RMS', 'pair': True})
GOLDEN_NLF['multi_float64'] = (gradient, (64, 96, 32, np.float64), {'signalFromMultipleImages': True})
GOLDEN_NLF['given_uint16'] = (gradient, (64, 96, 33, np.uint16), {'mn_mx_nbins': (300.0, 2900.0, 40)})
GOLDEN_NLF['given_pair_uint8'] = (gradient, (64, 96, 34, np.uint8),
                                  {'mn_mx_nbins': (10.0, 250.0, 24), 'pair': True})
GOLDEN_NLF['step1_uint8'] = (uniform_int, (64, 96, 35, np.uint8), {})
GOLDEN_NLF['step1_pair_uint16'] = (uniform_int, (64, 96, 36, np.uint16, 400, 470), {'pair': True})
GOLDEN_NLF['flat_uint16'] = (flat, (64, 96, 37, np.uint16), {})
GOLDEN_NLF['flat_float64'] = (flat, (64, 96, 38, np.float64), {})
GOLDEN_NLF['odd_float32'] = (gradient, (37, 53, 39, np.float32), {})


def nlf_inputs(name):
    """-> (img, img2 or None, calcNLF keywords)"""
    fn, args, kw = GOLDEN_NLF[name]
    kw = dict(kw)
    img = fn(*args)
    img2 = None
    if kw.pop('pair', False):
        a = list(args)
        a[2] += 100
        img2 = fn(*a)
    return img, img2, kw


def estimates_mean_std(name):
    """does the scene's range come from the signal's moments (and not from mn_mx_nbins)?"""
    return 'mn_mx_nbins' not in GOLDEN_NLF[name][2]


# the frames of the fit: large enough that the density filter leaves ~50 bins
FIT_SHAPE = (150, 260)


def fit_frame(seed=50, dtype=np.uint16):
    return gradient(FIT_SHAPE[0], FIT_SHAPE[1], seed, dtype)


def estimate_pairs():
    """three pairs of exposures for estimateFromImages"""
    return ([gradient(96, 160, 60 + i, np.uint16) for i in range(3)],
            [gradient(96, 160, 70 + i, np.uint16) for i in range(3)])


SNR_TRIPLE = (5.0, 40.0, 0.8)
SNR_SHAPE = (25, 31)          # the fixture's maps
# The estimated-NLF map, stored every SNR_NLF_STEP-th pixel.  Parity of a fit is defined only where
# the reference's own fit is well-conditioned: on a 96 x 160 frame of this scene MINPACK's answer
# moved by 2.4e-6 under perturbations of y in the last bit (1e-15), on this one by 6e-8
# (test_cpu_nlf.py::test_fit_scenes_are_well_conditioned).
SNR_NLF_SHAPE = (150, 260)
SNR_NLF_STEP = 6


def snr_callable(s):
    """a noise level function that is not a square root"""
    return 2.0 + 0.01 * s


def snr_frames(shape, seed=80, dtype=np.uint16):
    return gradient(shape[0], shape[1], seed, dtype), gradient(shape[0], shape[1], seed + 1, dtype)


# name -> SNR keywords ('pair': img2 given)
SNR_FORMS = {
    'triple': {'noise_level_function': 'triple'},
    'callable': {'noise_level_function': 'callable'},
    'constant': {'constant_noise_level': True},
    'triple_bg': {'noise_level_function': 'triple', 'bg': 100.0},
    'pair_bg': {'pair': True, 'bg': 100.0, 'noise_level_function': 'triple'},
    'pair_const_avg': {'pair': True, 'bg': 100.0, 'constant_noise_level': True,
                       'imgs_to_be_averaged': True},
    'triple_avg': {'noise_level_function': 'triple', 'imgs_to_be_averaged': True},
}


def snr_kwargs(form, triple_fn, callable_fn=snr_callable):
    """the SNR keywords of a form; `triple_fn`: what stands for the triple (the reference takes a
    function, the package the triple itself)"""
    kw = dict(SNR_FORMS[form])
    pair = kw.pop('pair', False)
    f = kw.get('noise_level_function')
    if f == 'triple':
        kw['noise_level_function'] = triple_fn
    elif f == 'callable':
        kw['noise_level_function'] = callable_fn
    return pair, kw


# ---------------------------------------------------------------- boundary scenes
def edge_table(mn, step, nbins):
    e = np.empty(nbins + 1)
    m = mn
    for n in range(nbins + 1):
        e[n] = m
        m += step
    return e


def planted_edges(h=12, w=20, mn=100.0, mx=230.0, nbins=13, seed=90):
    """a float64 signal inside (mn, mx) with pixels planted exactly on e[0], on every interior
    edge, on e[nbins], and one ulp outside each end -> (img, signal, (mn, mx, nbins)).  The step
    0.1-like fraction makes the accumulated edges differ from mn + n * step."""
    rng = np.random.default_rng(seed)
    step = (mx - mn) / nbins
    e = edge_table(mn, step, nbins)
    sig = rng.uniform(mn + 0.01, mx - 0.01, (h, w))
    flat_ = sig.ravel()
    pos = rng.permutation(flat_.size)
    vals = list(e) + [np.nextafter(e[0], -np.inf), np.nextafter(e[-1], np.inf),
                      np.nextafter(e[3], -np.inf), np.nextafter(e[3], np.inf)]
    flat_[pos[:len(vals)]] = vals
    img = sig + rng.standard_normal((h, w))
    return img, sig, (mn, mx, nbins)


def accumulated_edges(h=16, w=24, seed=91):
    """mn = 0.1, step = 0.1: e[n] is n + 1 additions of 0.1, not 0.1 * (n + 1), and every pixel
    is planted on an edge of the table - floor((s - e[0]) / step) alone names the wrong bin for
    some of them"""
    nbins = 60
    mn, mx = 0.1, 0.1 + 0.1 * nbins
    step = (mx - mn) / nbins
    e = edge_table(mn, step, nbins)
    rng = np.random.default_rng(seed)
    sig = e[rng.integers(0, nbins + 1, (h, w))]
    img = sig + 0.01 * rng.standard_normal((h, w))
    return img, sig, (mn, mx, nbins)


def min_len_scene():
    """a 100 x 120 float64 frame (min_len = 12) whose caller-given signal has exactly 12 pixels in
    one bin and 11 in its neighbour -> (img, signal, the two levels)"""
    h, w = 100, 120
    rng = np.random.default_rng(92)
    sig = np.full((h, w), 500.0)
    sig[:, : w // 2] = 300.0
    sig[:, w // 2:] = 700.0
    lv_keep, lv_drop = 421.0, 581.0
    p = rng.permutation(h * w)
    sig.ravel()[p[:12]] = lv_keep
    sig.ravel()[p[12:23]] = lv_drop
    img = sig + rng.standard_normal((h, w))
    return img, sig, (lv_keep, lv_drop)


def moments_frame():
    """mean 60000, std 2: a plain sum of squares loses seven digits of the variance"""
    return 60000.0 + 2.0 * np.random.default_rng(93).standard_normal((64, 64))
