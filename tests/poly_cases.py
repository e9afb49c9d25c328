"""Seeded scenes of the 2-D polynomial fit tests (csrc/poly.hip, interpolate/polyfit2d.py,
camera/flatField/postprocessing/polynomial.py).  tests/golden/gen_poly_golden.py runs the reference on
the PINNED ones - shapes small enough that the reference's raw-monomial design matrix has a condition
number of at most COND_MAX, so that its own lstsq error stays near cond * 2.2e-16 ~ 1e-9 on values in
[0, 1] - and the CPU and GPU tests compare against what it recorded within PIN_TOL."""
import numpy as np

MAX_ORDER = 5
COND_MAX = 5e6
PIN_TOL = 1e-9          # against the fixture, and between the device and the restatement
MOMENT_RTOL = 1e-12     # of sum |terms|: the tolerance of the NLF moments
STABLE = 1e-9           # no decision of a pinned loop is closer to its threshold than this
LAP_THRESHOLD = 0.01
MAX_DEV = 1e-5


def field(h, w, seed, noise=0.001):
    """a vignetting-like field in (0, 1]: 1 - 0.6 r^2 about (0.45 w, 0.55 h) plus Gaussian noise"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    f = 1.0 - 0.6 * (((x - 0.45 * w) / w) ** 2 + ((y - 0.55 * h) / h) ** 2)
    return f + noise * rng.standard_normal((h, w))


def random_mask(h, w, seed, frac=0.3):
    return np.random.default_rng(seed + 1000).random((h, w)) < frac


# ---- the fits pinned to the reference: name -> (arr, mask, kwargs of polyfit2dGrid)
def fit_cases():
    c = {}
    a = field(5, 7, 1)
    m = np.zeros((5, 7), bool)
    m[1, 2] = m[3, 5] = m[0, 6] = True
    c['all_5x7_o2'] = (a, m, dict(order=2, replace_all=True))
    c['all_5x7_o3'] = (a, m, dict(order=3, replace_all=True))
    a = field(24, 40, 2)
    m = random_mask(24, 40, 2, 0.25)
    m[5:9, 10:17] = True
    a = a.copy()
    a[m] = np.nan                      # the reference's own example puts NaN under the mask
    c['repair_24x40_o2'] = (a, m, dict(order=2))
    a = field(6, 8, 3)
    yy, xx = np.mgrid[0:12, 0:16].astype(np.float64) * 0.5
    c['outgrid_6x8_o2'] = (a, None, dict(order=2, outgrid=(yy, xx)))
    c['nomask_5x7_o2'] = (field(5, 7, 4), None, dict(order=2))
    return c


# ---- the loops pinned to the reference: name -> (img, mask, kwargs of polynomial, the exit it takes)
def loop_cases():
    c = {}
    # ends on res < max_dev after several iterations
    a = field(24, 40, LOOP_SEEDS['res'])
    m = np.zeros((24, 40), bool)
    m[4:8, 6:13] = True
    m[15:20, 25:31] = True
    a[m] = 0.0
    a[11, 20] += 0.05
    c['loop_res'] = (a, m, dict(), 'res')
    # ends on m == img.size: noise above the Laplacian's threshold everywhere
    a = field(*LOOP_ALL_SHAPE, LOOP_SEEDS['all'], noise=LOOP_ALL_NOISE)
    m = np.zeros(LOOP_ALL_SHAPE, bool)
    m[3:6, 4:9] = True
    a[m] = 0.0
    c['loop_all'] = (a, m, dict(), 'all')
    # ends on m == lastm: a smooth field, nothing has a high gradient once the holes are filled
    a = field(24, 40, LOOP_SEEDS['same'], noise=1e-4)
    m = np.zeros((24, 40), bool)
    m[10:14, 18:25] = True
    a[m] = 0.0
    c['loop_same'] = (a, m, dict(), 'same')
    return c


LOOP_SEEDS = {'res': 5, 'all': 6, 'same': 7}
LOOP_ALL_SHAPE = (24, 40)
LOOP_ALL_NOISE = 0.02

# ---- shapes of the device tests against the restatement
#  1 x 1 (order 0 only), 3 x 3, 5 x 7, 24 x 40, 67 x 259 (a row longer than one stride of the lanes, with a
#  tail; more rows than one workgroup takes), 9 x 1100 (a lane has 8 pixels in flight: two such rounds and
#  a tail), 130 x 70 (dilation window 14), 80 x 90 (its cap, 15), 8200 x 3 (more row quads than the
#  moments launch has workgroups: a second pass per workgroup)
MOMENT_SHAPES = [(1, 1), (3, 3), (5, 7), (24, 40), (67, 259), (9, 1100), (8200, 3)]
GRAD_SHAPES = [(1, 1), (1, 9), (9, 1), (3, 3), (5, 7), (24, 40), (67, 259), (130, 70), (80, 90), (22, 30)]


def scene(shape, seed, dtype=np.float64, frac=0.3):
    """(frame, mask) of a shape; NaN under every third masked pixel"""
    h, w = shape
    a = field(h, w, seed, noise=0.004).astype(dtype)
    m = random_mask(h, w, seed, frac)
    a[m & (np.arange(h * w).reshape(h, w) % 3 == 0)] = np.nan
    return a, m


def grad_scene(shape, seed, dtype=np.float64):
    """a field whose Laplacian crosses the threshold in places: noise of 0.002 (a Laplacian of 0.009 rms)
    in the left third, 0.0003 elsewhere, and a few raised pixels whose dilated windows stay apart"""
    h, w = shape
    rng = np.random.default_rng(seed)
    a = field(h, w, seed, noise=0.0)
    a += np.where(np.arange(w) < w / 3.0, 0.002, 0.0003) * rng.standard_normal((h, w))
    for _ in range(1 + (h * w) // 2000):
        a[rng.integers(0, h), rng.integers(0, w)] += 0.05
    return a.astype(dtype)


def exact_mask(shape, order):
    """a mask that leaves exactly (order+1)^2 valid pixels on a tensor grid of distinct rows and columns"""
    h, w = shape
    k = order + 1
    ys = np.unique(np.round(np.linspace(0, h - 1, k)).astype(int))
    xs = np.unique(np.round(np.linspace(0, w - 1, k)).astype(int))
    assert len(ys) == k and len(xs) == k
    m = np.ones(shape, bool)
    m[np.ix_(ys, xs)] = False
    return m
