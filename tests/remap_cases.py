"""The plain remap (csrc/remap.hip, csrc/remap_impl.hpp) walked path by path: one table of calls, each
with the kernels it must launch WRITTEN DOWN BY HAND from the rules of remap_dispatch - never computed
from the library.  tests/test_gpu_remap_paths.py runs every case and reads the evidence
(ctx.get_tuning('remap_path')); tests/test_cpu_remap_cases.py checks the table itself.  Inputs and
oracle calls live here so that both files build exactly the same arrays.

The bits below are restated, not imported: the CPU test holds them against imgprocessor_amd/_lib.py
and include/imgproc_hip.h."""
from collections import namedtuple

import numpy as np

from . import grid_ref

GATHER, REST, RING, TILE, TILE_MAP, STORED, U8_LZ_LDS, STRIP, STRIP_INT, LENS_MAP, FRAMES_INNER = (
    1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024)
BIT_NAMES = ('GATHER', 'REST', 'RING', 'TILE', 'TILE_MAP', 'STORED', 'U8_LZ_LDS', 'STRIP', 'STRIP_INT',
             'LENS_MAP', 'FRAMES_INNER')
G, INNER = GATHER, FRAMES_INNER

# every alternative off: what the second run of a case uses, and group A throughout
GATHER_ONLY = dict(ring_remap=0, tile_warp=0, stored_coords=0, strip_remap=0, u8_lz_lds=0, lens_cache=0)
RING_ALWAYS = dict(ring_remap=2, ring_min=1, tile_warp=0)
RING_RULE = dict(ring_remap=1, tile_warp=0)
STORED_ONLY = dict(ring_remap=0, tile_warp=0)
TILE_ALWAYS = dict(tile_warp=2, ring_remap=0, stored_coords=0)
TILE_RULE = dict(tile_warp=1, ring_remap=0, stored_coords=0)
EAGER = dict(ring_remap=2, ring_min=1, tile_warp=2, stored_coords=1)

F32, F64, U8, U16 = 'float32', 'float64', 'uint8', 'uint16'
DTYPE_PAIRS = ((F32, F32), (F64, F64), (U16, F32), (U16, U16), (U8, F32), (U8, U8), (F32, U8), (F32, U16))
BORDERS = ('constant', 'replicate', 'reflect', 'wrap', 'reflect101')

# group: A gather, B uint8 Lanczos4 from LDS, C ring + rest, D stored coordinates, E tile kernels,
# F strips / cached lens map, G grid.  edge: the boundary a case stands at, as (name, side) - the CPU test
# requires both sides of every name (a case may stand at several).  coords: (kind, variant).  pad: result pitch - dw.  oracle_frames:
# None = every frame.  inner0: run once more under frames_inner=0, expect GATHER and equal bits.
Case = namedtuple('Case', 'id group edge sdt ddt interp border cval coords n src_hw dst_hw knobs expect '
                          'pad oracle_frames inner0')

CASES = []


def _add(group, edge, sdt, ddt, interp, border, cval, coords, n, src_hw, dst_hw, knobs, expect, pad=0,
         oracle_frames=None, inner0=False, tag=''):
    cid = '%s-%s_%s-%s-%s-%s-%s-n%d-%dx%d%s' % (
        group, sdt[0] + sdt[-2:], ddt[0] + ddt[-2:], interp, border, coords[0], coords[1], n, dst_hw[0],
        dst_hw[1], tag)
    assert cid not in {c.id for c in CASES}, cid
    edge = () if edge is None else ((edge,) if isinstance(edge[0], str) else tuple(edge))
    CASES.append(Case(cid, group, edge, sdt, ddt, interp, border, cval, coords, n, tuple(src_hw),
                      tuple(dst_hw), dict(knobs), expect, pad, oracle_frames, inner0))


# ------------------------------------------------------------------ A: the gather kernel alone --
# the 256 x 4 tile: one row group / one tile column short of, at and past the tile, and two tiles
for k, dst in enumerate(((3, 255), (4, 256), (5, 257), (9, 513))):
    side = ('below', 'at', 'above', 'above')[k]
    for n in (1, 3):
        for interp in ('nearest', 'linear'):
            _add('A', ('tile256x4', side), F32, F32, interp, 'constant', 0.25, ('maps', 'wavy'), n, (13, 97),
                 dst, GATHER_ONLY, G | INNER if n == 3 else G, inner0=(n == 3))
        _add('A', ('tile256x4', side), F32, F32, 'cubic', 'constant', 0.25, ('maps', 'wavy'), n, (13, 97), dst,
             GATHER_ONLY, G)
# the instantiation matrix: 37 x 70 into 41 x 77, every dtype pair with every coordinate source
for sdt, ddt in DTYPE_PAIRS:
    for kind, var in (('maps', 'wavy'), ('lens', 'plain'), ('hom', 'mild')):
        for interp in ('linear', 'lanczos4'):
            for border in (BORDERS if (sdt, ddt) == (F32, F32) else ('constant', 'reflect')):
                # (a border value within the data's range: it must not widen the tolerance)
                _add('A', None, sdt, ddt, interp, border, 0.25 if ddt in (F32, F64) and sdt == ddt else 17.5,
                     (kind, var), 1, (37, 70), (41, 77), GATHER_ONLY, G)
for sdt in (F32, U8, F64):
    for interp in ('linear', 'lanczos4'):
        for border in ('constant', 'reflect'):
            _add('A', None, sdt, sdt, interp, border, 17.0 if sdt == U8 else 0.25, ('grid', 'four'), 1, (37, 70),
                 (41, 77), GATHER_ONLY, G)
for kind, var in (('maps', 'wavy'), ('lens', 'plain'), ('hom', 'mild')):
    for interp in ('linear_cv_q5', 'cubic_cv_q5'):          # uint16 in cv2's arithmetic: the FIXED forms
        for border in ('constant', 'reflect'):
            _add('A', None, U16, U16, interp, border, 17.5, (kind, var), 1, (37, 70), (41, 77), GATHER_ONLY, G)
# uint8 bicubic with the table in LDS: 16 row groups = 64 rows per workgroup
for k, rows in enumerate((63, 64, 65)):
    for interp in ('cubic_cv', 'cubic_cv_q5'):
        _add('A', ('u8cubic64rows', ('below', 'at', 'above')[k]), U8, U8, interp, 'reflect', 0.0,
             ('maps', 'wavy'), 2, (37, 71), (rows, 257), GATHER_ONLY, G)
# odd h x w uint8 sources, three frames: frame 1 starts off a dword
for interp, m in (('linear', G | INNER), ('cubic_cv', G), ('lanczos4', G)):
    _add('A', None, U8, U8, interp, 'constant', 9.0, ('maps', 'wavy'), 3, (37, 71), (41, 77), GATHER_ONLY, m,
         tag='-oddsrc')

# ------------------------------------------------------------ B: uint8 Lanczos4 from LDS --
# one band = 8 passes of 16 rows; `whole` 256-px segments; the result pitch dw + 1 stores bytes
_B_SHAPES = (((127, 255), 'below'), ((128, 256), 'at'), ((129, 257), 'above'))
for kind, var in (('maps', 'wavy'), ('lens', 'plain'), ('hom', 'mild')):
    for k, (dst, side) in enumerate(_B_SHAPES):
        for n in (1, 3):           # (both border modes meet both frame counts over the three shapes)
            _add('B', ('u8lz128x256', side), U8, U8, 'lanczos4', ('constant', 'reflect')[(k + (n == 3)) & 1], 9.0,
                 (kind, var), n, (37, 71), dst, {}, U8_LZ_LDS)
for kind, var in (('maps', 'wavy'), ('hom', 'mild')):
    _add('B', None, U8, U8, 'lanczos4', 'constant', 9.0, (kind, var), 3, (37, 71), (128, 256), {}, U8_LZ_LDS,
         pad=1, tag='-pitch')
_add('B', None, U8, U8, 'lanczos4', 'constant', 9.0, ('grid', 'four'), 3, (37, 71), (41, 77), {}, G)

# ------------------------------------------------------------------- C: ring + rest --
# strip_h = 32, strips of 128 px in pairs of 256, RingRemapKernel::kWaves frames per workgroup (2 for
# Lanczos4, else 4).  ring_remap = 2 launches whenever the planning pass ran; a new key always plans, and
# the test puts a ring call with a key of its own before every case, so no hint decides.
# The mask only says that the ring kernel was LAUNCHED: it writes the pixels of CLEAN strip pairs alone -
# whole 128-px strips (both of a pair, or the only one) with every footprint inside the source
# (ring_clean_pairs() below restates ring_plan_kernel's rule; the CPU test pins it).  So the picture is
# inset: result pixel (u, v) looks at about (u + 20, v + 12) of a source of (dh + 24) x (dw + 40), every
# footprint of a whole strip inside.  Only 128 and 257 of the columns below have a pair of whole strips
# (129 and 255 pair a whole strip with a partial one, 127 has none: all of those go to the rest launch, the
# other side of that rule); the row counts and the frame counts each meet a clean pair on every side.  The
# rim: the partial last strip / strip row, and for 65 rows a source cut off at 60 rows, so that the second
# strip row's footprints leave the source.
RING_INSET = (12, 20)          # (rows, columns) the result is inset into the source


def _ring_src(dst, cut=False):
    return (60 if cut else dst[0] + 2 * RING_INSET[0], dst[1] + 2 * RING_INSET[1])


_C_SHAPES = ((31, 128), (32, 257), (33, 128), (65, 257), (32, 127), (33, 129), (65, 255), (31, 257))
_ROW_SIDE = {31: 'below', 32: 'at', 33: 'above', 65: 'above'}
_COL_SIDE = {127: 'below', 128: 'at', 129: 'above', 255: 'below', 257: 'above'}
RING_WHOLE_PAIR_COLS = (128, 257)
for interp in ('linear', 'cubic', 'lanczos4'):
    kw = 2 if interp == 'lanczos4' else 4
    for kind in ('maps', 'lens', 'hom'):
        for k, dst in enumerate(_C_SHAPES):
            n = (kw - 1, kw, kw + 1)[k % 3]
            m = RING | REST | (INNER if kind == 'maps' and interp == 'linear' and n > 1 else 0)
            _add('C', (('ring_rows32', _ROW_SIDE[dst[0]]), ('ring_cols128', _COL_SIDE[dst[1]]),
                       ('ring_waves_' + interp, ('below', 'at', 'above')[k % 3])),
                 F32, F32, interp, ('constant', 'reflect')[k & 1], 0.25, (kind, 'inset'), n,
                 _ring_src(dst, cut=dst[0] == 65), dst, RING_ALWAYS, m)
# the default rule on a 64 x 256 result: ring_from by taps and coordinate source, ring_min = 2
# (the source cut off at 56 rows: the first strip row is clean, the second leaves the source)
for kind, interp, lo, hi in (('maps', 'linear', 15, 16), ('maps', 'cubic', 7, 8), ('maps', 'lanczos4', 2, 3),
                             ('lens', 'linear', 3, 4), ('lens', 'cubic', 3, 4), ('hom', 'cubic', 3, 4),
                             ('lens', 'lanczos4', 1, 2), ('hom', 'lanczos4', 1, 2)):
    inner = INNER if kind == 'maps' and interp == 'linear' else 0
    name = 'ring_from_%s_%s' % (kind, interp)
    _add('C', (name, 'below'), F32, F32, interp, 'constant', 0.25, (kind, 'inset'), lo, (56, 296), (64, 256),
         RING_RULE, G | (inner if lo > 1 else 0), oracle_frames=(0, lo - 1), tag='-rule')
    _add('C', (name, 'at'), F32, F32, interp, 'constant', 0.25, (kind, 'inset'), hi, (56, 296), (64, 256),
         RING_RULE, RING | REST | inner, oracle_frames=(0, hi - 1), tag='-rule')
_add('C', None, F32, F32, 'linear', 'constant', 0.25, ('hom', 'inset'), 16, (56, 296), (64, 256), RING_RULE, G,
     oracle_frames=(0, 15), tag='-rule')        # a bilinear homography never takes the ring by the rule

# ------------------------------------------------------------- D: stored coordinates --
for kind, var in (('lens', 'plain'), ('hom', 'mild')):
    for interp in ('cubic', 'cubic_cv', 'lanczos4'):
        _add('D', ('stored4_%s_%s' % (kind, interp), 'below'), F32, F32, interp, 'constant', 0.25, (kind, var),
             3, (37, 70), (41, 77), STORED_ONLY, G)
        _add('D', ('stored4_%s_%s' % (kind, interp), 'at'), F32, F32, interp, 'reflect', 0.25, (kind, var), 4,
             (37, 70), (41, 77), STORED_ONLY, STORED)
    _add('D', None, F32, F32, 'linear', 'constant', 0.25, (kind, var), 4, (37, 70), (41, 77), STORED_ONLY, G)
_add('D', None, F32, F32, 'linear', 'constant', 0.25, ('maps', 'wavy'), 4, (37, 70), (41, 77), STORED_ONLY, G | INNER)
_add('D', None, F32, F32, 'cubic', 'constant', 0.25, ('maps', 'wavy'), 4, (37, 70), (41, 77), STORED_ONLY, G)

# -------------------------------------------------------------------- E: tile kernels --
# homographies, forced: 64 x 32 output tiles, up to 8 frames per workgroup
_E_SHAPES = (((31, 63), 'below'), ((32, 64), 'at'), ((33, 65), 'above'))
for sdt, interp in ((F32, 'linear'), (F32, 'cubic'), (F32, 'lanczos4'), (U16, 'cubic_cv_q5'), (U16, 'lanczos4')):
    for dst, side in _E_SHAPES:
        _add('E', ('tile64x32', side), sdt, sdt, interp, 'constant', 0.25 if sdt == F32 else 17.5,
             ('hom', 'rot'), 5, (37, 70), dst, TILE_ALWAYS, TILE)
    for n, side in ((1, 'below'), (8, 'at'), (9, 'above')):
        _add('E', ('tile_frames8', side), sdt, sdt, interp, 'reflect', 0.25, ('hom', 'rot'), n, (37, 70),
             (33, 65), TILE_ALWAYS, TILE)
# no tile shape holds the boxes of a picture shrunk 8 times (the narrowest tile, 32 px, spans 256 source
# columns: a box has at most 128) - the call falls through, here to the gather kernel; shrunk 3 times the
# boxes (96 columns and the taps) fit
_add('E', ('tile_box_fits', 'above'), F32, F32, 'lanczos4', 'constant', 0.25, ('hom', 'shrink8'), 2, (300, 600),
     (33, 65), TILE_ALWAYS, G)
_add('E', ('tile_box_fits', 'below'), F32, F32, 'lanczos4', 'constant', 0.25, ('hom', 'shrink3'), 2, (300, 600),
     (33, 65), TILE_ALWAYS, TILE)
# what the tile kernel is not instantiated for
_add('E', None, F32, F32, 'nearest', 'constant', 0.25, ('hom', 'rot'), 5, (37, 70), (33, 65), TILE_ALWAYS, G)
for sdt, ddt in DTYPE_PAIRS:
    if (sdt, ddt) not in ((F32, F32), (U16, U16)):      # (uint8 Lanczos4 has its own kernel, u8_lz_lds = 1)
        _add('E', None, sdt, ddt, 'lanczos4', 'constant', 17.5, ('hom', 'rot'), 5, (37, 70), (33, 65),
             TILE_ALWAYS, U8_LZ_LDS if (sdt, ddt) == (U8, U8) else G)
_add('E', None, U16, U16, 'linear_cv_q5', 'constant', 17.5, ('hom', 'rot'), 5, (37, 70), (33, 65), TILE_ALWAYS, G)
_add('E', None, U16, U16, 'cubic', 'constant', 17.5, ('hom', 'rot'), 5, (37, 70), (33, 65), TILE_ALWAYS, G)
# the default rule where it is a product of counts
_add('E', None, F32, F32, 'lanczos4', 'constant', 0.25, ('hom', 'rot'), 1, (37, 70), (33, 65), TILE_RULE, TILE,
     tag='-rule')                                                    # Lanczos4: whenever the homography fits
_add('E', ('tile_u16_2e6', 'below'), U16, U16, 'lanczos4', 'constant', 17.5, ('hom', 'zoom4'), 1, (250, 500),
     (1000, 1999), TILE_RULE, G, oracle_frames=(0,), tag='-rule')
_add('E', ('tile_u16_2e6', 'at'), U16, U16, 'lanczos4', 'constant', 17.5, ('hom', 'zoom4'), 1, (250, 500),
     (1000, 2000), TILE_RULE, TILE, oracle_frames=(0,), tag='-rule')
_add('E', ('tile_cubic_16e6', 'below'), F32, F32, 'cubic', 'constant', 0.25, ('hom', 'near_identity'), 4,
     (2000, 2000), (1999, 2000), TILE_RULE, G, oracle_frames=(3,), tag='-rule')
_add('E', ('tile_cubic_16e6', 'at'), F32, F32, 'cubic', 'constant', 0.25, ('hom', 'near_identity'), 4,
     (2000, 2000), (2000, 2000), TILE_RULE, TILE, oracle_frames=(3,), tag='-rule')
# maps, forced
for interp in ('linear', 'cubic', 'lanczos4'):
    for dst, side in (((31, 63), 'below'), ((32, 64), 'at'), ((33, 65), 'above')):
        _add('E', ('tilemap64x32', side), F32, F32, interp, 'constant', 0.25, ('maps', 'wavy'), 5, (37, 70), dst,
             TILE_ALWAYS, TILE_MAP)
    for n, side in ((1, 'below'), (8, 'at'), (9, 'above')):
        _add('E', ('tilemap_frames8', side), F32, F32, interp, 'reflect', 0.25, ('maps', 'wavy'), n, (37, 70),
             (33, 65), TILE_ALWAYS, TILE_MAP)
    # a map that shrinks the picture 6 times: a 64 x 32 tile spans 384 x 192 source pixels, past every
    # LDS reserve (at most 128 columns x 72 rows) - those pixels go tap by tap
    _add('E', None, F32, F32, interp, 'constant', 0.25, ('maps', 'shrink6'), 2, (300, 600), (40, 90), TILE_ALWAYS,
         TILE_MAP, tag='-slow')
_add('E', ('tilemap_lz_8e6', 'below'), F32, F32, 'lanczos4', 'constant', 0.25, ('maps', 'zoom'), 1, (200, 400),
     (2000, 3999), TILE_RULE, G, oracle_frames=(0,), tag='-rule')
_add('E', ('tilemap_lz_8e6', 'at'), F32, F32, 'lanczos4', 'constant', 0.25, ('maps', 'zoom'), 1, (200, 400),
     (2000, 4000), TILE_RULE, TILE_MAP, oracle_frames=(0,), tag='-rule')

# ------------------------------------------------ F: strips and the cached lens map --
# ipa_undistort_dev sends integer batches of 4+ frames through its cached map into ipa_remap_dev
_add('F', ('lens_map4_u8_f32', 'below'), U8, F32, 'linear', 'constant', 9.0, ('lens', 'plain'), 3, (37, 72),
     (37, 72), {}, G)
_add('F', ('lens_map4_u8_f32', 'at'), U8, F32, 'linear', 'constant', 9.0, ('lens', 'plain'), 4, (37, 72),
     (37, 72), {}, LENS_MAP | STRIP)
_add('F', None, U16, F32, 'linear', 'constant', 9.0, ('lens', 'plain'), 1, (37, 72), (37, 72), {}, STRIP)
_add('F', ('lens_map4_u8_u8', 'below'), U8, U8, 'linear', 'constant', 9.0, ('lens', 'plain'), 3, (37, 72),
     (37, 72), {}, G)
_add('F', ('lens_map4_u8_u8', 'at'), U8, U8, 'linear', 'constant', 9.0, ('lens', 'plain'), 4, (37, 72),
     (37, 72), {}, LENS_MAP | STRIP_INT)
_add('F', None, U8, U8, 'linear', 'constant', 9.0, ('lens', 'plain'), 4, (37, 610), (37, 610), {},
     LENS_MAP | G | INNER)       # a width that is no multiple of 4: the strips decline, the maps stay

# ---------------------------------------------------------------------- G: the grid --
for sdt, interp, n in ((F32, 'lanczos4', 4), (F32, 'cubic', 4), (F32, 'linear', 16), (U8, 'lanczos4', 3),
                       (U16, 'lanczos4', 1)):
    _add('G', None, sdt, sdt, interp, 'constant', 0.25 if sdt == F32 else 17.0, ('grid', 'four'), n, (37, 70),
         (41, 77), EAGER, G)

BY_ID = {c.id: c for c in CASES}


# ------------------------------------------------------------------------------ inputs --
def _source(case):
    n, (h, w) = case.n, case.src_hw
    rng = np.random.default_rng(1000 + 7 * h + w)
    if case.sdt == U8:
        return rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    if case.sdt == U16:
        return rng.integers(0, 65536, (n, h, w), dtype=np.uint16)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = 0.5 + 0.25 * np.sin(2 * np.pi * x / 23) + 0.25 * np.cos(2 * np.pi * y / 17)
    out = np.clip(img[None] + 0.05 * rng.standard_normal((n, h, w)), 0, 1)
    if case.ddt in (U8, U16):     # values over the destination's range
        out = out * (255.0 if case.ddt == U8 else 65535.0)
    return out.astype(case.sdt)


def _lens(variant, dh, dw):
    """the lens model of tests/gpu_helpers.radial_maps"""
    K = np.array([[float(dw), 0, (dw - 1) / 2.0], [0, float(dw), (dh - 1) / 2.0], [0, 0, 1.0]])
    dist = np.array([-0.12, 0.03, 1e-3, -5e-4, 0.0])
    newK = K.copy()
    if variant == 'inset':      # group C: the model of the (dh + 24) x (dw + 40) source, the result inset into it
        K[0, 2] += RING_INSET[1]
        K[1, 2] += RING_INSET[0]
    return K, dist, newK


def _hom(variant, src_hw, dst_hw):
    (sh, sw), (dh, dw) = src_hw, dst_hw
    fx, fy = sw / float(dw), sh / float(dh)
    if variant == 'mild':         # the source stretched over the result, a little shear and perspective
        return np.array([[0.98 * fx, 0.03, 1.5], [-0.02, 1.01 * fy, 0.75], [1e-5, -2e-5, 1.0]])
    if variant == 'rot':          # 17 degrees about the middle, with perspective
        a = np.deg2rad(17.0)
        cx, cy, ux, uy = (sw - 1) / 2.0, (sh - 1) / 2.0, (dw - 1) / 2.0, (dh - 1) / 2.0
        R = np.array([[fx * np.cos(a), -fy * np.sin(a), 0], [fx * np.sin(a), fy * np.cos(a), 0], [0, 0, 1.0]])
        R[0, 2] = cx - (R[0, 0] * ux + R[0, 1] * uy)
        R[1, 2] = cy - (R[1, 0] * ux + R[1, 1] * uy)
        return np.array([[1, 0, 0], [0, 1, 0], [1e-4, 5e-5, 1.0]]) @ R
    if variant == 'inset':        # group C: (u, v) -> about (u + 20, v + 12), a little shear and perspective
        return np.array([[0.99, 0.02, RING_INSET[1] + 0.3], [-0.01, 1.01, RING_INSET[0] + 2.6], [1e-5, -2e-5, 1.0]])
    if variant == 'shrink8':
        return np.array([[8.0, 0, 20.0], [0, 8.0, 10.0], [0, 0, 1.0]])
    if variant == 'shrink3':
        return np.array([[3.0, 0, 20.0], [0, 3.0, 10.0], [0, 0, 1.0]])
    if variant == 'zoom4':
        return np.array([[0.25, 0.001, 0.5], [-0.001, 0.25, 0.25], [0, 0, 1.0]])
    if variant == 'near_identity':
        return np.array([[1.0, 1e-4, 0.25], [-1e-4, 1.0, 0.5], [1e-8, -1e-8, 1.0]])
    raise KeyError(variant)


def _maps(variant, src_hw, dst_hw, oracle):
    (sh, sw), (dh, dw) = src_hw, dst_hw
    y, x = np.mgrid[0:dh, 0:dw].astype(np.float32)
    fx, fy = sw / float(dw), sh / float(dh)
    if variant == 'wavy':         # tests/test_gpu_parity.py::test_remap_all_modes_vs_oracle, scaled to the shapes
        mx = (x * (0.93 * fx) - 2.2 + 3 * np.sin(y / 9)).astype(np.float32)
        my = (y * (0.9 * fy) - 3.1 + 2 * np.cos(x / 7)).astype(np.float32)
        mx[min(5, dh - 1), 7] = np.nan
        my[min(9, dh - 1), 3] = np.inf
        mx[min(11, dh - 1), 11] = 1e7
        return mx, my
    if variant == 'inset':
        return oracle.build_undistort_map(*_lens('inset', dh, dw), dh, dw)
    if variant == 'shrink6':
        return (x * 6.0 + 3.3).astype(np.float32), (y * 6.0 + 1.7).astype(np.float32)
    if variant == 'zoom':
        return (x * fx + 0.3 * np.sin(y / 50)).astype(np.float32), (y * fy - 0.25).astype(np.float32)
    raise KeyError(variant)


# four cells over the 41 x 77 result: they meet inside 4-px groups, the last two columns belong to none
GRID_RECTS = np.array([[0, 0, 38, 20], [38, 0, 37, 20], [0, 20, 38, 21], [38, 20, 37, 21]], dtype=np.int32)


def _grid(src_hw):
    sh, sw = src_hw
    Ms = []
    for k, (x0, y0, w, h) in enumerate(GRID_RECTS):
        Ms.append([[0.9 + 0.02 * k, 0.03, x0 * sw / 77.0 + 1.25], [-0.02, 0.85 + 0.03 * k, y0 * sh / 41.0 + 0.5],
                   [1e-4 * (k - 1), -5e-5, 1.0]])
    return GRID_RECTS, np.array(Ms, dtype=np.float64)


def inputs(case, oracle):
    """-> dict: src (n, h, w) and the coordinate source's arrays"""
    kind, var = case.coords
    inp = {'src': _source(case)}
    if kind == 'maps':
        inp['mx'], inp['my'] = _maps(var, case.src_hw, case.dst_hw, oracle)
    elif kind == 'lens':
        inp['K'], inp['dist'], inp['newK'] = _lens(var, *case.dst_hw)
    elif kind == 'hom':
        inp['M'] = _hom(var, case.src_hw, case.dst_hw)
    else:
        inp['rects'], inp['Ms'] = _grid(case.src_hw)
    return inp


ORC_INTERP = {'nearest': ('NEAREST', 0), 'linear': ('LINEAR', 0), 'cubic': ('CUBIC_KEYS', 0),
              'cubic_cv': ('CUBIC_CV', 0), 'linear_cv_q5': ('LINEAR', 1), 'cubic_cv_q5': ('CUBIC_CV', 1),
              'lanczos4': ('LANCZOS4', 0)}


def hole_value(case):
    """what a pixel no grid cell covers receives: the border value as the result type holds it"""
    if case.ddt in (U8, U16):
        top = 255 if case.ddt == U8 else 65535
        return np.dtype(case.ddt).type(min(max(np.rint(case.cval), 0), top))
    return np.dtype(case.ddt).type(case.cval)


def oracle_frame(case, inp, oracle, f):
    """the oracle's result for frame f"""
    name, q5 = ORC_INTERP[case.interp]
    oi = getattr(oracle, name) | (oracle.Q5 if q5 else 0)
    src, odt, kind = inp['src'][f], np.dtype(case.ddt), case.coords[0]
    if kind == 'maps':
        return oracle.remap(src, inp['mx'], inp['my'], oi, case.border, case.cval, out_dtype=odt)
    if kind == 'lens':
        return oracle.undistort(src, inp['K'], inp['dist'], inp['newK'], oi, case.border, case.cval,
                                out_dtype=odt, out_shape=case.dst_hw)
    if kind == 'hom':
        return oracle.warp_perspective(src, inp['M'], case.dst_hw, oi, case.border, case.cval, out_dtype=odt)
    out = np.full(case.dst_hw, hole_value(case), odt)       # the grid: every cell's own warp, in paint order
    for (x0, y0, w, h), M in zip(inp['rects'], inp['Ms']):
        out[y0:y0 + h, x0:x0 + w] = oracle.warp_perspective(src, M, (int(h), int(w)), oi, case.border, case.cval,
                                                            out_dtype=odt)
    assert ((grid_ref.paint_rects(inp['rects'], case.dst_hw) == -1) == (np.arange(case.dst_hw[1]) >= 75)).all()
    return out


def tolerance(case, src):
    """(rtol, atol) of tests/test_gpu_parity.py for the result type, the value range taken from the
    source frame (not from the result, which a border value could widen); None: equal"""
    if case.ddt == F32:
        return 1e-5, 1e-5 * float(np.abs(src.astype(np.float64)).max())
    if case.ddt == F64:
        return 1e-12, 1e-12
    return None


# ------------------------------------------------- which pixels the ring kernel writes --
def coordinates(case, inp, oracle):
    """(sx, sy) of every result pixel, float64 arrays of the result's shape"""
    kind = case.coords[0]
    dh, dw = case.dst_hw
    if kind == 'maps':
        return inp['mx'].astype(np.float64), inp['my'].astype(np.float64)
    if kind == 'lens':
        mx, my = oracle.build_undistort_map(inp['K'], inp['dist'], inp['newK'], dh, dw)
        return mx.astype(np.float64), my.astype(np.float64)
    v, u = np.mgrid[0:dh, 0:dw].astype(np.float64)
    M = inp['M']
    w = M[2, 0] * u + M[2, 1] * v + M[2, 2]
    return (M[0, 0] * u + M[0, 1] * v + M[0, 2]) / w, (M[1, 0] * u + M[1, 1] * v + M[1, 2]) / w


def ring_clean_pairs(case, inp, oracle):
    """ring_plan_kernel's rule (csrc/ring_stencil.hpp, K = 1) restated in numpy: -> bool array (strip rows,
    strip pairs), True where ring_remap_kernel writes the pair's pixels.  A strip of 128 columns x up to 32
    rows is clean when it is whole, every footprint lies inside the source, the footprints of every two-row
    step span no more rows than the ring holds, source rows only move forward by at most 4 per step, and
    the strip's footprints span at most 160 columns; a pair is clean when both its strips are, or its only
    one."""
    nt = {'linear': 2, 'linear_cv_q5': 2, 'lanczos4': 8}.get(case.interp, 4)
    rr = 16 if nt == 8 else 8
    back = nt // 2 - 1
    q5 = nt == 8 or case.interp.endswith('_q5')
    (sh, sw), (dh, dw) = case.src_hw, case.dst_hw
    sx, sy = coordinates(case, inp, oracle)
    if q5:
        sx, sy = np.rint(sx * 32) / 32, np.rint(sy * 32) / 32
    fin = (np.abs(sx) < 1e6) & (np.abs(sy) < 1e6)
    ix = np.where(fin, np.floor(np.where(fin, sx, 0)), 0).astype(np.int64) - back
    iy = np.where(fin, np.floor(np.where(fin, sy, 0)), 0).astype(np.int64) - back
    inside = fin & (ix >= 0) & (iy >= 0) & (ix + nt <= sw) & (iy + nt <= sh)
    strips_x, rows = (dw + 127) // 128, (dh + 31) // 32
    clean = np.zeros((rows, strips_x), bool)
    for r in range(rows):
        y0, y1 = 32 * r, min(32 * r + 32, dh)
        for c in range(strips_x):
            xs = 128 * c
            if xs + 128 > dw or not inside[y0:y1, xs:xs + 128].all():
                continue
            ok, ybase, hrun = True, 0, 0
            for v0 in range(y0, y1, 2):
                blk = iy[v0:min(v0 + 2, y1), xs:xs + 128]
                ymn, ymx = int(blk.min()), int(blk.max())
                need = ymx + nt
                if ymx - ymn + nt > rr:
                    ok = False
                if v0 == y0:
                    ybase, hrun, cnt = ymn, need, 0
                else:
                    cnt, hrun = max(need - hrun, 0), max(need, hrun)
                if cnt > 4 or ymn < max(ybase, hrun - rr):
                    ok = False
            blk = ix[y0:y1, xs:xs + 128]
            if int(blk.max()) + nt > (int(blk.min()) & ~3) - 4 + 160:
                ok = False
            clean[r, c] = ok
    pairs = np.zeros((rows, (strips_x + 1) // 2), bool)
    for c in range(pairs.shape[1]):
        pairs[:, c] = clean[:, 2 * c] & (clean[:, 2 * c + 1] if 2 * c + 1 < strips_x else True)
    return pairs
