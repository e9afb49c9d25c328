"""Seeded inputs of the spot tests (tests/test_cpu_spot.py, tests/test_gpu_spot.py) and of the
generator of their fixture (tests/golden/gen_spot_golden.py): the scenes of
camera/flatField/vignettingFromSpotAverage.py and the masks of the labelling tests.  numpy only."""
import numpy as np

ALL_DTYPES = (np.uint8, np.uint16, np.float32, np.float64)
TILE_H, TILE_W = 16, 64        # kTH, kTW of csrc/spot.hip
BLOCK = 1024                   # linear indices per block of the numbering passes
SPOT = 9                       # side of a planted spot; 7 after the erosion


def _cast(a, dtype):
    if np.issubdtype(dtype, np.integer):
        return np.clip(np.round(a), 0, np.iinfo(dtype).max).astype(dtype)
    return a.astype(dtype)


def spot_frame(rng, shape, dtype, spots, level, noise):
    """background level + noise with bright squares: spots = [(row, column, value)] of the top left
    corners; the values are far above the noise, so a planted square survives the threshold whole"""
    a = level + noise * rng.standard_normal(shape)
    for r, c, v in spots:
        a[r:r + SPOT, c:c + SPOT] += v
    return _cast(a, dtype)


def scenes():
    """name -> dict(images, bg, averageSpot, thresh, raises): every kind the routine distinguishes"""
    out = {}
    # (a) uint16, averaged background frames, Otsu, the spot's pixels; frame 2 holds two spots of
    # exactly the same size (the first in raster order wins), frame 4 a spot touching the corner
    rng = np.random.default_rng(41)
    shape = (48, 70)
    pos = [(5, 8, 900.), (30, 50, 700.), (20, 30, 1100.), (12, 55, 800.), (0, 0, 600.)]
    imgs = [spot_frame(rng, shape, np.uint16, [p], 120., 4.) for p in pos]
    imgs[2] = spot_frame(rng, shape, np.uint16, [(20, 30, 1100.), (4, 50, 1000.)], 120., 4.)
    bgs = [spot_frame(rng, shape, np.uint16, [], 100., 4.) for _ in range(3)]
    out['a_u16_bgframes_otsu_spot'] = dict(images=imgs, bg=bgs, averageSpot=False, thresh=None, raises=None)
    # (b) float32, scalar background, a given threshold, the spot's pixels; frame 1 is constant
    rng = np.random.default_rng(42)
    shape = (40, 56)
    imgs = [spot_frame(rng, shape, np.float32, [p], 10., 0.5) for p in ((3, 4, 50.), (0, 0, 0.), (25, 40, 80.))]
    imgs[1] = np.full(shape, 10., np.float32)
    out['b_f32_scalar_thresh_spot'] = dict(images=imgs, bg=3.5, averageSpot=False, thresh=30., raises=None)
    # (c) uint8, scalar background, Otsu, the reference's two rows; spots left of column h; frame 2 constant
    rng = np.random.default_rng(43)
    imgs = [spot_frame(rng, shape, np.uint8, [p], 20., 1.5) for p in ((6, 10, 150.), (28, 22, 200.), (0, 0, 0.),
                                                                       (15, 3, 100.))]
    imgs[2] = np.full(shape, 20, np.uint8)
    out['c_u8_scalar_otsu_rows'] = dict(images=imgs, bg=2, averageSpot=True, thresh=None, raises=None)
    # (d) float64, w > h, the second spot near the right edge: its column is no row
    rng = np.random.default_rng(44)
    imgs = [spot_frame(rng, shape, np.float64, [p], 5., 0.2) for p in ((10, 10, 30.), (20, 45, 40.))]
    out['d_f64_rows_index_error'] = dict(images=imgs, bg=0, averageSpot=True, thresh=None, raises=IndexError)
    # (e) no spot anywhere: mx stays 0
    imgs = [np.full((20, 30), v, np.uint8) for v in (7, 9)]
    out['e_u8_no_spot'] = dict(images=imgs, bg=1.0, averageSpot=False, thresh=None, raises=None)
    return out


# ---------------------------------------------------------------- labelling masks
def checkerboard(shape):
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    return ((x + y) % 2 == 0).astype(np.uint8)


def spiral(shape):
    """a one-pixel-wide path that winds from the top left corner inwards, one free pixel between its
    turns: a single component at either connectivity whose parent chains cross every tile seam"""
    h, w = shape
    m = np.zeros(shape, np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = 1

    def free(yy, xx):
        return 0 <= yy < h and 0 <= xx < w and not m[yy, xx]

    def filled(yy, xx):
        return 0 <= yy < h and 0 <= xx < w and m[yy, xx]

    while True:
        for _ in range(2):   # straight on, else one turn to the right
            if free(y + dy, x + dx) and not filled(y + 2 * dy, x + 2 * dx):
                break
            dy, dx = dx, -dy
        else:
            return m
        y, x = y + dy, x + dx
        m[y, x] = 1


def u_shape(shape):
    """two arms that meet only in the last row: the root is the first pixel of the left arm"""
    h, w = shape
    m = np.zeros(shape, np.uint8)
    m[:, 1 if w > 2 else 0] = 1
    m[:, w - 2 if w > 2 else w - 1] = 1
    m[h - 1, :] = 1
    m[h - 1, 0] = 0 if w > 2 else m[h - 1, 0]
    return m


def diagonal_pair(shape, corner, anti):
    """two pixels that touch only across the tile corner at (row, column) = corner"""
    m = np.zeros(shape, np.uint8)
    r, c = corner
    if anti:
        m[r - 1, c], m[r, c - 1] = 1, 1
    else:
        m[r - 1, c - 1], m[r, c] = 1, 1
    return m


def random_field(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def golden_patterns():
    """name -> mask: the small patterns whose skimage / scipy labels the fixture stores"""
    s = (2 * TILE_H + 1, 2 * TILE_W + 2)    # 33 x 130: 3 x 3 tiles, the last ones one and two pixels wide
    out = {
        'one': np.ones((1, 1), np.uint8),
        'row': random_field((1, 2 * TILE_W + 3), 0.6, 1),
        'column': random_field((2 * TILE_H + 5, 1), 0.6, 2),
        'false': np.zeros(s, np.uint8),
        'true': np.ones(s, np.uint8),
        'checker': checkerboard(s),
        'spiral': spiral(s),
        'u': u_shape(s),
    }
    for k, (corner, anti) in enumerate((((TILE_H, TILE_W), False), ((TILE_H, TILE_W), True),
                                        ((2 * TILE_H, 2 * TILE_W), False), ((2 * TILE_H, 2 * TILE_W), True))):
        out['diag%d' % k] = diagonal_pair(s, corner, anti)
    for d in (0.3, 0.5, 0.62):
        out['random%02d' % int(100 * d)] = random_field((TILE_H + 4, TILE_W + 6), d, int(100 * d))
    return out


# shapes around one tile (16 x 64) and one numbering block (1024 pixels), up to 3 x 3 tiles
LABEL_SHAPES = [(1, 1), (1, 130), (40, 1), (TILE_H, TILE_W), (TILE_H - 1, TILE_W), (TILE_H + 1, TILE_W),
                (TILE_H, TILE_W - 1), (TILE_H, TILE_W + 1), (3 * TILE_H, 3 * TILE_W), (2 * TILE_H + 1, 2 * TILE_W + 2)]
