"""The case table of the structured IDW fills (csrc/idw.hip): which kernel and which branch of it
each case stands on, proven on the CPU by test_cpu_idw_refs.py from the replay of the reference's
walk (idw_ref.fast_idw_fill) and from the selection rule restated below.

Masks are built, not drawn: the probed pixel, the neighbours that come before a chosen index in
the walk's order (a ragged disc), blocks and corners.  Grids are 40 x 70 or smaller.
"""
import numpy as np

from . import idw_ref as ref

H, W = 40, 70
PITCH_PAD = 7


def grid_of(shape, seed=1):
    return np.random.default_rng(seed).uniform(-1.0, 2.0, shape)


# ------------------------------------------------------------------ fast IDW ----
def order_mask(shape, p, k, upto, keep=()):
    """the probe p and its neighbours before index `upto` of the walk masked, but those in `keep`"""
    offs, _ = ref.neighbours_of(k)
    m = np.zeros(shape, bool)
    m[p] = True
    for n in range(upto):
        y, x = p[0] + offs[n, 0], p[1] + offs[n, 1]
        if n not in keep and 0 <= y < shape[0] and 0 <= x < shape[1]:
            m[y, x] = True
    return m


def block_mask(shape, y0, y1, x0, x1, holes=()):
    m = np.zeros(shape, bool)
    m[y0:y1, x0:x1] = True
    for hy, hx in holes:
        m[hy, hx] = False
    return m


def disc_mask(shape, c, r):
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    return (y - c[0]) ** 2 + (x - c[1]) ** 2 <= r * r


C = (20, 35)     # a probe whose 33 x 33 window lies inside the 40 x 70 grid


def _fast_cases():
    s = (H, W)
    cases = []

    def add(name, k, m, mask, shape=s):
        cases.append(dict(name=name, k=k, minnvals=m, mask=mask, shape=shape))
    for t in (63, 64, 65):        # two hits before, the third - the stop - at t
        add('hit %d' % t, 8, 2, order_mask(s, C, 8, t, keep=(5, t - 1)))
    for t in (127, 128):
        add('hit %d' % t, 8, 2, order_mask(s, C, 8, t, keep=(5, 70)))
    add('hit 200', 8, 3, order_mask(s, C, 8, 200, keep=(5, 70, 140)))
    add('hit 700', 16, 4, order_mask(s, C, 16, 700, keep=(5, 70, 300, 650)))
    # corners: far-outside neighbours (beyond -1 in both axes)
    add('corner, many hits', 4, 50, block_mask(s, 0, 1, 0, 1))            # far stop in batch 0
    add('corner, 13 hits', 4, 12, block_mask(s, 0, 1, 0, 1))              # far before hit stop
    add('corner, 2 hits', 4, 1, block_mask(s, 0, 1, 0, 1))                # hit stop before far
    add('corner block', 8, 200, block_mask(s, 0, 6, 0, 6))                # far with no hit yet
    add('in from the corner', 8, 200, block_mask(s, 0, 12, 0, 12, holes=[(3, 5), (9, 2)]))
    add('in from the far corner', 6, 200, block_mask(s, H - 11, H, W - 11, W, holes=[(H - 4, W - 6)]))
    # walks to the end of the list
    add('end 80', 4, 100, block_mask(s, C[0], C[0] + 1, C[1], C[1] + 1))
    add('end 288', 8, 1000, disc_mask(s, C, 2))
    add('end 1088', 16, 2000, block_mask(s, C[0], C[0] + 1, C[1], C[1] + 2))
    add('first hit', 4, 0, disc_mask(s, C, 3) | block_mask(s, 0, 2, W - 2, W))
    add('nothing in reach', 4, 4, block_mask(s, 5, 30, 10, 50))
    add('two segments', 4, 4, block_mask((9, 70), 2, 5, 61, 68), shape=(9, 70))
    return cases


FAST = _fast_cases()
FAST_CLASSES = ('hit 63', 'hit 64', 'hit 65', 'hit 127', 'hit 128', 'hit batch >= 2', 'far batch 0',
                'far batch >= 1', 'far unlit', 'hit<far', 'far<hit', 'end 80', 'end 288', 'end 1088',
                'first hit', 'minnvals beyond window', 'nothing in reach')


def fast_args(case, power=2):
    offs, wts = ref.neighbours_of(case['k'], power)
    return offs, wts


_cache = {}


def _once(key, make):
    """a reference is computed once, shared by the tests and left unchanged"""
    if key not in _cache:
        _cache[key] = make()
        for a in _cache[key]:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _cache[key]


def fast_ref(case, dtype, defect=None, pitch=None):
    def make():
        g = grid_of(case['shape']).astype(dtype)
        offs, wts = fast_args(case)
        return g, ref.fast_idw_fill(g, case['mask'], offs, wts, case['minnvals'], defect, pitch)
    return _once(('fast', case['name'], np.dtype(dtype).name, defect, pitch), make)


def fast_classes(case, res):
    """the classes of FAST_CLASSES that the masked pixels of a case hit"""
    m = case['mask']
    n = len(ref.neighbours_of(case['k'])[0])
    out = set()
    for i, j in zip(*np.nonzero(m)):
        stop, why, hits = res['stop'][i, j], res['reason'][i, j], res['hits'][i, j]
        if why == ref.HIT:
            if stop in (63, 64, 65, 127, 128):
                out.add('hit %d' % stop)
            if stop >= 128:
                out.add('hit batch >= 2')
            if case['minnvals'] == 0:
                out.add('first hit')
        elif why == ref.FAR:
            out.add('far batch 0' if stop < 64 else 'far batch >= 1')
        else:
            if res['filled'][i, j] and hits == res['n'][i, j]:
                out.add('end %d' % n)
                if case['minnvals'] >= n:
                    out.add('minnvals beyond window')
            if not res['filled'][i, j]:
                out.add('nothing in reach')
        if res['far_unlit'][i, j]:
            out.add('far unlit')
        if res['both'][i, j]:
            out.add(res['both'][i, j])
    return out


# ------------------------------------------------------------------ IDW fill ----
def idw_kernel(k):
    """-> (kernel, window rows per pass): idw_path of csrc/stencil_paths.hpp restated - a window
    of 17 ... 64 columns runs with the lanes over the columns of a window row, two rows per pass
    up to 32 columns; any other with the lanes over the taps"""
    kw = 2 * k + 1
    if 16 < kw <= 64:
        return 'rows', 2 if kw <= 32 else 1
    return 'taps', 0


def corners_mask(shape, extra=()):
    m = np.zeros(shape, bool)
    h, w = shape
    for y, x in [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)] + list(extra):
        if 0 <= y < h and 0 <= x < w:
            m[y, x] = True
    return m


def _idw_cases():
    cases = []

    def add(name, k, shape, mask, nan=None, centre_weight=0.0):
        cases.append(dict(name=name, k=k, shape=shape, mask=mask, nan=nan, centre_weight=centre_weight,
                          kernel=idw_kernel(k)))
    for k in (1, 7, 8, 15, 16, 31, 32):
        s = (H, W)
        m = corners_mask(s, [(20, 35), (20, 36), (7, 63), (7, 64), (33, 1)])
        add('k%d main' % k, k, s, m, nan=(19, 34) if k in (1, 8, 16) else None,
            centre_weight=7.0 if k in (7, 15, 32) else 0.0)
    add('k1 masked window', 1, (H, W), block_mask((H, W), 10, 15, 20, 25))
    add('k7 masked window', 7, (H, W), block_mask((H, W), 2, 19, 30, 47))
    for k in (8, 16, 31):
        add('k%d 7x9' % k, k, (7, 9), corners_mask((7, 9), [(3, 4)]))
        add('k%d 3x70' % k, k, (3, 70), corners_mask((3, 70), [(1, 35), (1, 63), (1, 64)]))
    for k in (1, 8, 16):
        for w in (64, 65, 128, 129):
            add('k%d 6x%d' % (k, w), k, (6, w), corners_mask((6, w), [(2, 63), (3, 64), (2, 127), (3, 128)]))
    return cases


IDW = _idw_cases()


def idw_ref_of(case, dtype, defect=None, pitch=None):
    return _once(('idw', case['name'], np.dtype(dtype).name, defect, pitch),
                 lambda: _idw_ref_of(case, dtype, defect, pitch))


def _idw_ref_of(case, dtype, defect, pitch):
    g = grid_of(case['shape'], 2)
    if case['nan']:
        g[case['nan']] = np.nan
    g[case['mask']] = np.nan            # what a caller has at the pixels to be filled
    g = g.astype(dtype)
    wts = ref.weights_of(case['k'])
    wts[case['k'], case['k']] = case['centre_weight']   # the reference leaves this entry unset
    return g, wts, ref.idw_fill(g, case['mask'], case['k'], wts, defect, pitch)


def pitched(g, pad=PITCH_PAD, fill=1e30):
    """the grid in a buffer of pitch w + pad; the padding holds a value that ruins any mean"""
    big = np.full((g.shape[0], g.shape[1] + pad), fill, g.dtype)
    big[:, :g.shape[1]] = g
    return big
