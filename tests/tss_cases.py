"""Scenes and the case table for the signal-stability kernels (csrc/tss.hip), shared by
test_cpu_tss.py (which proves on the CPU what each kind of scene is sensitive to),
test_gpu_tss.py (which runs them on the device) and tests/golden/gen_tss_golden.py.

A scene is (stack, times, offset, ascent, error): the kernel takes the fit as an argument, so a
scene may prescribe it.

lattice     offset = ascent = 0, integer frames, error in {2, 3, 4}: thresholds c of 1, 1.5 and 2
            on the half-integer lattice.  Many samples equal c (and, for the float types, -c), and
            with the per-block bias about half of a window's samples lie beyond c: many windows sit
            at a count of exactly 62 or 63.
planes      spatially constant frames, each above c or not after a prescribed pattern along the
            frames.  A window holds 25 samples of each of its five (reflected) planes: three
            planes above give 75 and an event, two give 50 and none.  The patterns hold runs and
            gaps of every length the frame count allows.
borders     the same along x or y: columns (rows) above c or not, constant along the other two
            axes.  In the interior they alternate, so a pixel is an event exactly when the two
            OUTERMOST samples of its window are above c: at the first and last output pixel of a
            tile they lie in the neighbouring tile.  The first three are 0 1 1 and the last three
            1 1 0: the corner pixels are events only because -2 reflects to 1 (the edge repeated
            gives two of five).  Two phases, so that both pixels at a tile border are probed.
continuous  a seeded smooth scene with noise and two fluctuating blocks, fitted by the restatement.
demo, demo16  the scenes of tests/golden/tss.npz: a scene after the description of the reference's
            demo (a device area with a decaying signal, two blocks fluctuating at different
            frequencies, Gaussian noise, 15 frames) and an integer-valued uint16 series.
"""
import numpy as np

TILE_W, TILE_H = 64, 16          # kTssTileW, kTssTileH of csrc/tss.hip
FIN_TILE_W, FIN_TILE_H = 32, 8   # kFinW, kFinH
MAX_FRAMES = 64

ALL_DTYPES = (np.uint8, np.uint16, np.float32, np.float64)
MULTI = (TILE_H + 3, 2 * TILE_W + 5)
SHAPES = ((1, 1), (3, 4), (5, 7), MULTI)
# the kernel has one strategy for every T; 2 .. 4 reflect into planes the window already holds
T_VALUES = (2, 3, 4, 5, 6, 9, 16, 17, 64)


def shapes_for(T):
    """64 frames at the smallest multi-tile shape only"""
    return (MULTI,) if T == MAX_FRAMES else SHAPES


def times_for(T, seed=0):
    """ascending, unevenly spaced"""
    rng = np.random.default_rng(900 + seed)
    return np.cumsum(rng.uniform(0.5, 1.5, T))


def _signed(dtype):
    return np.dtype(dtype).kind == 'f'


def lattice(T, h, w, dtype, seed):
    rng = np.random.default_rng(seed)
    by, bx = np.mgrid[0:h, 0:w]
    bias = ((by // 5 + bx // 7) % 3).astype(np.int64)               # 0, 1, 2 in blocks
    lo = -2 if _signed(dtype) else 0
    v = rng.integers(lo, lo + 4, (T, h, w)) + bias[None]
    if _signed(dtype):
        v = v * np.where((by // 5) % 2, -1, 1)[None]                  # blocks that lean below -c
    error = rng.choice([2.0, 3.0, 3.0, 4.0], (h, w))
    zero = np.zeros((h, w))
    return v.astype(dtype), times_for(T, seed), zero, zero.copy(), error


# 1011001 and 0100110 are the planes that leave one clean frame between two events and one event
# frame between two clean ones (the majority of five smooths everything shorter away); then runs
# and gaps of every length
# It starts 1 0 0: frame 0 sees planes 1 0 0 1 2 by reflection (two above, no event) and 0 0 0 1 2
# with the edge repeated (three above); variant 1 is the pattern reversed, so that the last frame
# is decided the same way.
_PATTERN = '100' + '10110010100110' + '0011110000' + '1101000111100101100000111110100110001110111100001011111101000000111'


def z_pattern(T, variant):
    hot = np.array([ch == '1' for ch in _PATTERN[:T]])
    return hot[::-1].copy() if variant else hot


def planes(T, h, w, dtype, variant):
    hot = z_pattern(T, variant)
    st = np.where(hot[:, None, None], 2, 0) * np.ones((T, h, w), np.int64)
    zero = np.zeros((h, w))
    return st.astype(dtype), times_for(T, variant), zero, zero.copy(), np.full((h, w), 2.0)


def edge_pattern(n, phase, tail=True):
    p = (np.arange(n) + phase) % 2 == 0
    if n >= 6:
        p[:3] = (False, True, True)
        if tail:
            p[-3:] = (True, True, False)
    return p


def borders(T, h, w, dtype, axis, phase):
    """axis 'x' or 'y'"""
    # the multi-tile height leaves three rows below its tile border: in phase 1 they alternate on, so
    # that the last row of the first tile is decided by its outermost sample
    hot = (edge_pattern(w, phase)[None, None, :] if axis == 'x' else
           edge_pattern(h, phase, tail=phase == 0)[None, :, None])
    st = np.where(hot, 2, 0) * np.ones((T, h, w), np.int64)
    zero = np.zeros((h, w))
    return st.astype(dtype), times_for(T, phase), zero, zero.copy(), np.full((h, w), 2.0)


def continuous_stack(T, h, w, dtype, seed):
    rng = np.random.default_rng(seed)
    top = 200.0 if np.dtype(dtype) == np.uint8 else 3000.0
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    k = np.arange(T, dtype=np.float64)[:, None, None]
    f = top * (0.5 + 0.2 * np.sin(x / 9.0) * np.cos(y / 5.0)) - 0.004 * top * k
    f = f + 0.02 * top * rng.standard_normal((T, h, w))
    f = f + 0.05 * top * np.sin(1.3 * k) * ((x // 8 + y // 4) % 3 == 0)    # blocks that fluctuate
    f = f + 0.05 * top * np.sin(0.4 * k + 1.0) * ((x // 8 + y // 4) % 3 == 1)
    if np.dtype(dtype).kind == 'f':
        return times_for(T, seed), f.astype(dtype)
    return times_for(T, seed), np.clip(np.round(f), 0, np.iinfo(dtype).max).astype(dtype)


def continuous(T, h, w, dtype, seed):
    from . import tss_ref
    times, st = continuous_stack(T, h, w, dtype, seed)
    offset, ascent, error = tss_ref.fit(times, st)
    return st, times, offset, ascent, error


# ------------------------------------------------------------------ the fixture's scenes ----
DEMO_HW, DEMO_T = (100, 100), 15
DEMO16_HW, DEMO16_T = (96, 104), 9


# the demo scene: a square device area whose signal decays linearly over the series, two square
# blocks inside it whose signal swings between 0 and an amplitude as (sin(phase) + 1) / 2 with the
# phase running from 0 to `sweep` over the series, Gaussian noise everywhere
DEMO_AREA = (20, 80)                  # rows and columns [20, 80) of the 100 x 100 frame
DEMO_SIGNAL = (100.0, 60.0)           # first and last frame
DEMO_NOISE = 5.0
DEMO_BLOCKS = (dict(at=(30, 40), amplitude=20.0, sweep=10.0),    # slow
               dict(at=(60, 70), amplitude=30.0, sweep=50.0))    # fast
DEMO_SPAN = 100.0                     # the measurement times run from 0 to here


def demo():
    """-> (times, (15, 100, 100) float64 frames), seeded"""
    (h, w), n = DEMO_HW, DEMO_T
    rng = np.random.default_rng(5143)
    frames = DEMO_NOISE * rng.standard_normal((n, h, w))
    lo, hi = DEMO_AREA
    frames[:, lo:hi, lo:hi] += np.linspace(DEMO_SIGNAL[0], DEMO_SIGNAL[1], n)[:, None, None]
    for blk in DEMO_BLOCKS:
        lo, hi = blk['at']
        swing = 0.5 * blk['amplitude'] * (1.0 + np.sin(np.linspace(0.0, blk['sweep'], n)))
        frames[:, lo:hi, lo:hi] += swing[:, None, None]
    return np.linspace(0.0, DEMO_SPAN, n), frames


def demo16():
    """integer-valued uint16 frames: a gradient that decays, blocks that fluctuate, noise"""
    times, st = continuous_stack(DEMO16_T, DEMO16_HW[0], DEMO16_HW[1], np.uint16, 77)
    return times, st


# ------------------------------------------------------------------ the case table ----
_cache = {}


def _once(key, make):
    if key not in _cache:
        out = make()
        for a in out if isinstance(out, tuple) else out.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def case_ids(T):
    """[(kind, (h, w), dtype, variant)] of one frame count: continuous scenes in all four types at
    every shape, lattice scenes likewise where the image has more than one pixel (one pixel
    quantises the counts to multiples of 25: no window can sit at 62 or 63), the pattern scenes in
    one type each (rotating) - the border scenes along an axis of six samples or more, which the
    designed ends of edge_pattern need"""
    out = []
    for si, (h, w) in enumerate(shapes_for(T)):
        for di, dt in enumerate(ALL_DTYPES):
            if h * w > 1:
                out.append(('lattice', (h, w), dt, 0))
            out.append(('continuous', (h, w), dt, 0))
        for v in range(2):
            out.append(('planes', (h, w), ALL_DTYPES[(si + v) % 4], v))
            if w >= 6:
                out.append(('borders_x', (h, w), ALL_DTYPES[(si + v + 1) % 4], v))
            if h >= 6:
                out.append(('borders_y', (h, w), ALL_DTYPES[(si + v + 2) % 4], v))
    return out


def scene(kind, T, shape, dtype, variant):
    """-> (stack, times, offset, ascent, error), made once, read-only"""
    h, w = shape
    key = (kind, T, shape, np.dtype(dtype).name, variant)
    seed = 3000 + 17 * T + 5 * h + w + 1000 * ALL_DTYPES.index(dtype)

    def make():
        if kind == 'lattice':
            return lattice(T, h, w, dtype, seed)
        if kind == 'continuous':
            return continuous(T, h, w, dtype, seed)
        if kind == 'planes':
            return planes(T, h, w, dtype, variant)
        return borders(T, h, w, dtype, kind[-1], variant)
    return _once(key, make)


def reference(kind, T, shape, dtype, variant):
    """-> (events, raw event length) of a scene, the reference's way (median form), made once"""
    from . import tss_ref
    key = ('ref', kind, T, shape, np.dtype(dtype).name, variant)

    def make():
        evt = tss_ref.events_median(*scene(kind, T, shape, dtype, variant))
        return evt, tss_ref.run_lengths(evt)
    return _once(key, make)


def probes(T, h, w):
    """voxels a tile algorithm decides from beyond its tile or beyond the image: the first and
    last output pixel of every tile in x and y, the image corners, in the first, a middle and
    the last frame"""
    ys = sorted({0, h - 1} | {y for y in range(0, h, TILE_H)} | {y - 1 for y in range(TILE_H, h, TILE_H)})
    xs = sorted({0, w - 1} | {x for x in range(0, w, TILE_W)} | {x - 1 for x in range(TILE_W, w, TILE_W)})
    return [(k, y, x) for k in sorted({0, T // 2, T - 1}) for y in ys for x in xs]
