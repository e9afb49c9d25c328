"""The remap -> filter chains (csrc/fused.hip, fused_impl.hpp, fused_sep_impl.hpp, fused_big.hip) walked route by
route: one table of calls, each with the launch record it must leave WRITTEN DOWN BY HAND from the rules of
dense_route, chain_one_kernel, dense_chain, lens_through_cache, fused_plan / shared_loop_plan, fused_batch and
wave_grid - never computed from the library, nor from a restatement of those rules.
tests/test_gpu_chain_paths.py runs every case and reads the evidence (ctx.get_tuning('chain_path'));
tests/test_cpu_chain_cases.py checks the table itself.  Inputs and references live here so that both files build
exactly the same arrays.

The bits below are restated, not imported: the CPU test holds them against imgprocessor_amd/_lib.py and
include/imgproc_hip.h.

Geometry.  Every case runs under strip_h = 16 on a 52 x 760 result ('main'): four strips per row at the 240-px
step (3, 5, 9, 11 taps; first columns -8, 232, 472, 712) and at the 248-px step (7 x 7; -4, 244, 492, 740) - strip
columns 1 and 2 lie inside the picture, 0 and 3 are rim - and four strip rows, of which row 1 is interior for
every K up to 11 (row 2 too up to 9 taps; rows 0 and 3 never).  Two twins, for one case per kernel family:
'odd', 52 x 757 - the same strips, rows that are no whole 16-byte vectors, so the rim strips of a batch leave the
shared-record loop ((dw & 3) != 0) - and 'ragged', 52 x 485, where NO strip is interior in x: every strip runs
with its columns resolved.  (Rows of float32 results are always 4-byte aligned, so vec_out holds at any width:
only a picture without an interior strip column keeps every strip off the fast loops.)  fast_strips() restates
the kernels' predicates; the CPU test asserts all of this.

The coordinates stretch the 64 x 780 source by 1.13 along the rows (no rotation, and ROTATED needs 64e6 pixels: no
case here can turn it - tests/test_gpu_tile_warp.py asserts that bit) and leave it along its left and right edges:
columns 0 .. 8 (a rim strip) and from about column 698 on, which for the main and the odd geometry begins inside
interior strip column 2: constant-border footprints occur in rim and in interior strips."""
from collections import namedtuple

import numpy as np

from .conftest import synth
from .conv_ref import bound, ref_conv2d, ref_sepconv2d

(RESIDENT, STREAMED, SEP, TWO_LAUNCHES, RANK1, LENS_MAP, ROTATED, STORED, SPLIT, FRAMES_WG, PER_FRAME) = (
    1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024)
BIT_NAMES = ('RESIDENT', 'STREAMED', 'SEP', 'TWO_LAUNCHES', 'RANK1', 'LENS_MAP', 'ROTATED', 'STORED', 'SPLIT',
             'FRAMES_WG', 'PER_FRAME')
RES, STR, TWO, R1, LM, STO, SPL, FWG, PF = (RESIDENT, STREAMED, TWO_LAUNCHES, RANK1, LENS_MAP, STORED, SPLIT,
                                            FRAMES_WG, PER_FRAME)

F32, U8, U16 = 'float32', 'uint8', 'uint16'
VALUE_RANGE = {F32: 1.0, U16: 4095.0, U8: 255.0}
BORDER_VALUE = {F32: 0.25, U16: 1000.0, U8: 60.0}      # of the remap, within the data's range
STRIP_H = 16
SRC_HW = (64, 780)
SHAPES = {'main': (52, 760), 'odd': (52, 757), 'ragged': (52, 485)}
NMAX = 9

# the knobs whose bits a second run takes away (every case also runs under strip_h = 16)
PLAIN = dict(frames_wg=0, stored_coords=0, lens_cache=0)

# filt: ('dense', kh, kw) a full-rank kernel; ('sep', nky, nkx); ('rank1', K) np.outer(ky, kx);
# ('near1', K) the same with entry [0, 0] times 1 + 1e-9.  edge: (name, side) pairs, as in remap_cases.py.
# overlap: source and result in one allocation, the result inside the slack after the last source frame.
Case = namedtuple('Case', 'id group edge sdt interp coords n shape filt knobs expect overlap')

CASES = []


def _add(group, edge, sdt, interp, coords, n, filt, knobs, expect, shape='main', overlap=False, tag=''):
    cid = '%s-%s-%s-%s-%s-n%d-%s%s%s' % (group, sdt[0] + sdt[-2:], interp, coords, '_'.join(str(v) for v in filt), n,
                                        shape, ''.join('-%s=%d' % kv for kv in sorted(knobs.items())),
                                        '-overlap' if overlap else tag)
    assert cid not in {c.id for c in CASES}, cid
    assert 1 <= n <= NMAX
    edge = () if edge is None else ((edge,) if isinstance(edge[0], str) else tuple(edge))
    CASES.append(Case(cid, group, edge, sdt, interp, coords, n, shape, tuple(filt), dict(knobs), expect, overlap))


# ------------------------------------------------------------------------ D: the dense route --
# float32 frames, maps, bilinear, one frame (n = 1: frames_wg stays 0 in every launch)
_add('D', ('dense_k7_streams', 'below'), F32, 'linear', 'maps', 1, ('dense', 3, 3), {}, RES | PF)
_add('D', ('dense_k7_streams', 'below'), F32, 'linear', 'maps', 1, ('dense', 5, 5), {}, RES | PF)
_add('D', ('dense_k7_streams', 'at'), F32, 'linear', 'maps', 1, ('dense', 7, 7), {}, STR | PF)
_add('D', ('dense_k11_last', 'below'), F32, 'linear', 'maps', 1, ('dense', 9, 9), {}, STR | PF)
_add('D', ('dense_k11_last', 'at'), F32, 'linear', 'maps', 1, ('dense', 11, 11), {}, STR | PF)
_add('D', ('dense_k11_last', 'above'), F32, 'linear', 'maps', 1, ('dense', 13, 13), {}, TWO)
_add('D', ('dense_square_odd', 'above'), F32, 'linear', 'maps', 1, ('dense', 3, 5), {}, TWO)
_add('D', ('dense_square_odd', 'above'), F32, 'linear', 'maps', 1, ('dense', 8, 8), {}, TWO)   # stream-shaped, even
_add('D', ('dense_square_odd', 'below'), F32, 'linear', 'maps', 4, ('dense', 9, 9), {}, STR | FWG)
# the knobs of dense_route
_add('D', ('stream_k', 'above'), F32, 'linear', 'maps', 1, ('dense', 7, 7), dict(stream_k=9), RES | PF)
_add('D', ('stream_k', 'below'), F32, 'linear', 'maps', 1, ('dense', 9, 9), dict(stream_k=9), STR | PF)
_add('D', ('big_fused', 'above'), F32, 'linear', 'maps', 1, ('dense', 9, 9), dict(big_fused=0), TWO)
_add('D', ('big_fused', 'above'), F32, 'linear', 'maps', 1, ('dense', 7, 7), dict(big_fused=0), RES | PF)
_add('D', ('big_fused', 'below'), F32, 'linear', 'maps', 1, ('dense', 11, 11), dict(big_fused=1), STR | PF)
# the interpolation (bicubic maps are a table the frames share: frames_wg at n = 4, with no shared-record loop)
_add('D', ('dense_cubic_k7', 'below'), F32, 'cubic', 'maps', 1, ('dense', 5, 5), {}, RES | PF)
_add('D', ('dense_cubic_k7', 'at'), F32, 'cubic', 'maps', 4, ('dense', 7, 7), {}, RES | FWG)
_add('D', ('dense_cubic_k7', 'above'), F32, 'cubic_cv', 'maps', 1, ('dense', 9, 9), {}, TWO)
_add('D', ('dense_taps', 'below'), F32, 'cubic_cv', 'hom', 4, ('dense', 5, 5), {}, RES | PF)   # no table, no shared loop
_add('D', ('dense_taps', 'above'), F32, 'lanczos4', 'maps', 1, ('dense', 5, 5), {}, TWO)
# coordinates by value: 9 x 9 streams from maps only - the lens model reaches it through its cached map
_add('D', ('dense_k9_by_value', 'below'), F32, 'linear', 'hom', 1, ('dense', 5, 5), {}, RES | PF)
_add('D', ('dense_k9_by_value', 'above'), F32, 'linear', 'hom', 1, ('dense', 9, 9), {}, TWO)
_add('D', ('lens_cache_dense', 'below'), F32, 'linear', 'lens', 1, ('dense', 5, 5), dict(lens_cache=0), RES | PF)
_add('D', ('lens_cache_dense', 'below'), F32, 'linear', 'lens', 1, ('dense', 9, 9), dict(lens_cache=0), TWO)
_add('D', ('lens_cache_dense', 'at'), F32, 'linear', 'lens', 1, ('dense', 9, 9), {}, STR | LM | PF)
_add('D', ('lens_cache_dense', 'at'), F32, 'linear', 'lens', 4, ('dense', 5, 5), {}, RES | LM | FWG)
_add('D', None, F32, 'linear', 'lens', 1, ('dense', 13, 13), {}, TWO | LM)

# --------------------------------------------------------------- C: the dense route, camera frames --
# uint16, 7 x 7: the shared7 rule keeps whole workgroups of frames on the resident kernel's shared-record loop
_add('C', (('shared7_frames', 'at'), ('pipe7', 'at')), U16, 'linear', 'maps', 4, ('dense', 7, 7), {}, RES | FWG)
_add('C', ('shared7_frames', 'below'), U16, 'linear', 'maps', 3, ('dense', 7, 7), {}, STR | PF)
_add('C', ('shared7_frames', 'above'), U16, 'linear', 'maps', 5, ('dense', 7, 7), {}, STR | PF)
_add('C', ('shared7_frames', 'at'), U16, 'linear', 'maps', 8, ('dense', 7, 7), {}, RES | FWG)
_add('C', ('pipe7', 'below'), U16, 'linear', 'maps', 4, ('dense', 7, 7), dict(pipe7=0), STR | FWG)
_add('C', None, F32, 'linear', 'maps', 4, ('dense', 7, 7), {}, STR | FWG)        # float32 frames: never shared7
_add('C', ('u16_k7_last', 'at'), U16, 'linear', 'maps', 1, ('dense', 7, 7), {}, STR | PF)
_add('C', ('u16_k7_last', 'above'), U16, 'linear', 'maps', 1, ('dense', 9, 9), {}, TWO)
_add('C', ('u16_k7_last', 'below'), U16, 'linear', 'maps', 4, ('dense', 5, 5), {}, RES | FWG)
_add('C', ('u16_coords', 'above'), U16, 'linear', 'hom', 1, ('dense', 5, 5), {}, TWO)
_add('C', ('u16_coords', 'below'), U16, 'linear', 'lens', 1, ('dense', 5, 5), dict(lens_cache=0), RES | PF)
_add('C', ('u16_coords', 'below'), U16, 'linear', 'lens', 4, ('dense', 5, 5), dict(lens_cache=0), RES | FWG)
_add('C', None, U16, 'cubic', 'maps', 1, ('dense', 5, 5), {}, TWO)
for K in (3, 5, 7):
    _add('C', ('u8_coords', 'below'), U8, 'linear', 'maps', 1, ('dense', K, K), {}, RES | PF)
_add('C', ('u8_coords', 'below'), U8, 'linear', 'maps', 4, ('dense', 7, 7), {}, RES | FWG)
_add('C', ('u8_coords', 'above'), U8, 'linear', 'lens', 1, ('dense', 5, 5), dict(lens_cache=0), TWO)
_add('C', ('u8_coords', 'above'), U8, 'linear', 'hom', 1, ('dense', 5, 5), {}, TWO)
_add('C', ('u8_coords', 'below'), U8, 'linear', 'lens', 1, ('dense', 5, 5), {}, RES | LM | PF)
_add('C', None, U8, 'linear', 'maps', 1, ('dense', 9, 9), {}, TWO)

# --------------------------------------------------------------------- S: the separable route --
# whole workgroups of float32 frames: the shared-record loop with two different, non-symmetric factors
for K in (3, 5, 7, 9):
    _add('S', ('sep_taps9', 'below' if K < 9 else 'at'), F32, 'linear', 'maps', 4, ('sep', K, K), {}, SEP | FWG)
    _add('S', None, F32, 'linear', 'maps', 1, ('sep', K, K), {}, SEP | PF)
_add('S', ('sep_taps9', 'above'), F32, 'linear', 'maps', 4, ('sep', 11, 11), {}, TWO)
_add('S', ('sep_equal_taps', 'above'), F32, 'linear', 'maps', 4, ('sep', 3, 5), {}, TWO)
_add('S', ('sep_equal_taps', 'above'), F32, 'linear', 'maps', 1, ('sep', 7, 5), {}, TWO)
_add('S', ('sep_equal_taps', 'below'), F32, 'linear', 'hom', 1, ('sep', 5, 5), {}, SEP | PF)
_add('S', ('sep_taps', 'above'), F32, 'cubic', 'maps', 4, ('sep', 5, 5), {}, TWO)
_add('S', ('sep_taps', 'below'), F32, 'linear', 'lens', 1, ('sep', 5, 5), dict(lens_cache=0), SEP | PF)
_add('S', None, F32, 'linear', 'lens', 4, ('sep', 7, 7), {}, SEP | LM | FWG)
# camera frames: fused_sep_interp has no uint16 source for the lens model by value - only chain_one_kernel's
# coord_kind != 1 keeps such a call from running the float32 source on uint16 bytes
_add('S', ('sep_u16_coords', 'below'), U16, 'linear', 'maps', 4, ('sep', 5, 5), {}, SEP | FWG)
_add('S', ('sep_u16_coords', 'below'), U16, 'linear', 'maps', 1, ('sep', 9, 9), {}, SEP | PF)
_add('S', ('sep_u16_coords', 'below'), U16, 'linear', 'hom', 1, ('sep', 5, 5), {}, SEP | PF)
_add('S', ('sep_u16_coords', 'above'), U16, 'linear', 'lens', 1, ('sep', 5, 5), dict(lens_cache=0), TWO)
_add('S', ('sep_u16_coords', 'above'), U16, 'linear', 'lens', 4, ('sep', 7, 7), dict(lens_cache=0), TWO)
_add('S', ('sep_u16_coords', 'below'), U16, 'linear', 'lens', 4, ('sep', 7, 7), {}, SEP | LM | FWG)
_add('S', ('sep_u8_coords', 'below'), U8, 'linear', 'maps', 4, ('sep', 5, 5), {}, SEP | FWG)
_add('S', ('sep_u8_coords', 'below'), U8, 'linear', 'maps', 1, ('sep', 7, 7), {}, SEP | PF)
_add('S', ('sep_u8_coords', 'above'), U8, 'linear', 'hom', 1, ('sep', 5, 5), {}, TWO)
_add('S', ('sep_u8_coords', 'above'), U8, 'linear', 'lens', 1, ('sep', 5, 5), dict(lens_cache=0), TWO)
_add('S', ('sep_u16', 'below'), U16, 'linear', 'maps', 4, ('sep', 5, 5), dict(sep_u16=0), TWO)
_add('S', ('sep_u16', 'below'), U8, 'linear', 'maps', 4, ('sep', 5, 5), dict(sep_u16=0), TWO)
_add('S', ('sep_u16', 'at'), U16, 'linear', 'maps', 1, ('sep', 3, 3), dict(sep_u16=1), SEP | PF)
_add('S', None, F32, 'linear', 'maps', 4, ('sep', 5, 5), dict(sep_u16=0), SEP | FWG)   # float32: always

# ----------------------------------------------------------------------------- R: rank-1 --
for K in (3, 5, 7, 9):
    _add('R', (('rank1_exact', 'at'), ('rank1_taps9', 'below' if K < 9 else 'at'), ('rank1_sep', 'at')),
         F32, 'linear', 'maps', 4, ('rank1', K), {}, R1 | SEP | FWG)
_add('R', None, F32, 'linear', 'maps', 1, ('rank1', 5), {}, R1 | SEP | PF)
_add('R', ('rank1_exact', 'above'), F32, 'linear', 'maps', 4, ('near1', 3), {}, RES | FWG)
_add('R', ('rank1_exact', 'above'), F32, 'linear', 'maps', 4, ('near1', 5), {}, RES | FWG)
_add('R', ('rank1_exact', 'above'), F32, 'linear', 'maps', 4, ('near1', 7), {}, STR | FWG)
_add('R', ('rank1_exact', 'above'), F32, 'linear', 'maps', 4, ('near1', 9), {}, STR | FWG)
_add('R', ('rank1_sep', 'below'), F32, 'linear', 'maps', 4, ('rank1', 5), dict(rank1_sep=0), RES | FWG)
_add('R', ('rank1_sep', 'below'), F32, 'linear', 'maps', 4, ('rank1', 9), dict(rank1_sep=2), STR | FWG)
_add('R', ('rank1_taps9', 'above'), F32, 'linear', 'maps', 4, ('rank1', 11), {}, STR | FWG)
_add('R', ('rank1_taps', 'above'), F32, 'cubic', 'maps', 1, ('rank1', 5), {}, RES | PF)
_add('R', ('rank1_taps', 'below'), F32, 'linear', 'hom', 1, ('rank1', 5), {}, R1 | SEP | PF)
_add('R', None, F32, 'linear', 'lens', 4, ('rank1', 5), {}, R1 | SEP | LM | FWG)
_add('R', ('rank1_u16_lens', 'below'), U16, 'linear', 'maps', 4, ('rank1', 5), {}, R1 | SEP | FWG)
_add('R', ('rank1_u16_lens', 'above'), U16, 'linear', 'lens', 4, ('rank1', 5), dict(lens_cache=0), RES | FWG)

# ------------------------------------------------------------------------- B: the batch plan --
# whole batch at a multiple of 4 frames, head + tail from 7 frames on, else every frame on its own; the streamed
# kernel has no shared-record loop and no plan: wave_grid alone orders its frames (frames_wg at multiples of 4)
for n, side in ((1, 'below'), (3, 'below'), (4, 'at'), (5, 'above'), (6, 'above'), (7, 'split'), (8, 'at'), (9, 'split')):
    own = SPL | FWG if side == 'split' else (FWG if side == 'at' else PF)
    e = (('plan_frames4', side if side != 'split' else 'above'), ('plan_split7', 'at' if side == 'split' else 'below'))
    _add('B', e, F32, 'linear', 'maps', n, ('dense', 5, 5), {}, RES | own)
    _add('B', e, F32, 'linear', 'maps', n, ('sep', 5, 5), {}, SEP | own, tag='')
    _add('B', ('streamed_frames4', 'at' if n % 4 == 0 else ('below' if n < 4 else 'above')), F32, 'linear', 'maps', n,
         ('dense', 9, 9), {}, STR | (FWG if n in (4, 8) else PF), tag='')
for knob in ('frames_wg', 'pipe', 'frames_inner'):
    _add('B', (knob, 'below'), F32, 'linear', 'maps', 4, ('dense', 5, 5), {knob: 0}, RES | PF)
    _add('B', (knob, 'below'), F32, 'linear', 'maps', 4, ('sep', 5, 5), {knob: 0}, SEP | PF)
    _add('B', (knob, 'below'), F32, 'linear', 'maps', 4, ('dense', 9, 9), {knob: 0}, STR | PF)
    _add('B', (knob, 'at'), F32, 'linear', 'maps', 8, ('dense', 3, 3), {knob: 1}, RES | FWG)
_add('B', None, F32, 'linear', 'maps', 7, ('dense', 5, 5), dict(frames_wg=0), RES | PF)
# source and result ranges that overlap by fused_plan's rule (whole strides) but in no byte read: no split
_add('B', ('plan_apart', 'below'), F32, 'linear', 'maps', 7, ('dense', 5, 5), {}, RES | PF, overlap=True)
_add('B', ('plan_apart', 'below'), F32, 'linear', 'maps', 7, ('sep', 5, 5), {}, SEP | PF, overlap=True)
_add('B', ('plan_apart', 'at'), F32, 'linear', 'maps', 7, ('dense', 3, 3), {}, RES | SPL | FWG)

# -------------------------------------------------------------------- T: stored coordinates --
# a homography's coordinates evaluated once, for batches on the shared plan from stored_coords (4) frames on
for filt, own in ((('dense', 5, 5), RES), (('sep', 5, 5), SEP), (('sep', 9, 9), SEP)):
    _add('T', (('stored4', 'at'), ('stored_coords', 'at')), F32, 'linear', 'hom', 4, filt, {}, own | STO | FWG)
    _add('T', ('stored4', 'below'), F32, 'linear', 'hom', 3, filt, {}, own | PF)
    _add('T', ('stored_coords', 'below'), F32, 'linear', 'hom', 4, filt, dict(stored_coords=0), own | FWG)
_add('T', ('stored4', 'above'), F32, 'linear', 'hom', 7, ('dense', 5, 5), {}, RES | STO | SPL | FWG)
_add('T', ('stored4', 'above'), F32, 'linear', 'hom', 5, ('sep', 5, 5), {}, SEP | PF)     # per frame: no table
_add('T', ('stored4', 'above'), U16, 'linear', 'hom', 8, ('sep', 5, 5), {}, SEP | STO | FWG)
_add('T', None, F32, 'linear', 'hom', 4, ('dense', 5, 5), dict(frames_wg=0), RES | PF)     # no shared plan: no table
_add('T', None, F32, 'linear', 'hom', 4, ('dense', 7, 7), {}, RES | STO | FWG)

# ---------------------------------------------------------------- G: the two other geometries --
for shape in ('odd', 'ragged'):
    _add('G', None, F32, 'linear', 'maps', 4, ('dense', 5, 5), {}, RES | FWG, shape=shape)
    _add('G', None, F32, 'linear', 'maps', 1, ('dense', 3, 3), {}, RES | PF, shape=shape)
    _add('G', None, U16, 'linear', 'maps', 4, ('dense', 7, 7), {}, RES | FWG, shape=shape)
    _add('G', None, F32, 'linear', 'maps', 4, ('dense', 9, 9), {}, STR | FWG, shape=shape)
    _add('G', None, F32, 'linear', 'maps', 1, ('dense', 7, 7), {}, STR | PF, shape=shape)
    _add('G', None, F32, 'linear', 'maps', 4, ('sep', 7, 7), {}, SEP | FWG, shape=shape)
    _add('G', None, F32, 'linear', 'hom', 1, ('sep', 5, 5), {}, SEP | PF, shape=shape)
    _add('G', None, F32, 'linear', 'maps', 4, ('rank1', 9), {}, R1 | SEP | FWG, shape=shape)
    _add('G', None, F32, 'cubic', 'maps', 1, ('dense', 5, 5), {}, RES | PF, shape=shape)
    _add('G', None, F32, 'linear', 'maps', 4, ('dense', 13, 13), {}, TWO, shape=shape)

BY_ID = {c.id: c for c in CASES}


# ------------------------------------------------------------------------------ inputs --
def _frames(sdt):
    """NMAX frames of SURVEY 8(d) content; every case uses the first n"""
    out = np.stack([synth(SRC_HW, 300 + i) for i in range(NMAX)])
    if sdt == F32:
        return out
    return np.round(out.astype(np.float64) * VALUE_RANGE[sdt]).astype(sdt)


_FRAMES = {}


def source(case):
    if case.sdt not in _FRAMES:
        _FRAMES[case.sdt] = _frames(case.sdt)
        _FRAMES[case.sdt].setflags(write=False)
    return _FRAMES[case.sdt][:case.n]


def _scale(dw):
    """the stretch along the rows: result column u looks at about a * u - 9.3"""
    return 1.13 * 760.0 / dw if dw < 700 else 1.13


def maps(shape):
    dh, dw = SHAPES[shape]
    y, x = np.mgrid[0:dh, 0:dw].astype(np.float64)
    return ((_scale(dw) * x - 9.3 + 0.004 * y).astype(np.float32),
            (y + 5.6 + 0.003 * x - 2e-6 * x * x).astype(np.float32))


def homography(shape):
    return np.array([[_scale(SHAPES[shape][1]), 0.004, -9.3], [0.003, 1.0, 5.6], [1e-6, -2e-6, 1.0]])


def lens(shape):
    """-> K, dist5, newK: the source's focal length along the rows 1.13 times the result's"""
    dh, dw = SHAPES[shape]
    a = _scale(dw)
    cxn, cyn = (dw - 1) / 2.0, (dh - 1) / 2.0
    newK = np.array([[300.0, 0, cxn], [0, 300.0, cyn], [0, 0, 1.0]])
    K = np.array([[300.0 * a, 0, a * cxn - 9.3], [0, 300.0, cyn + 5.6], [0, 0, 1.0]])
    return K, np.array([-0.002, 0.001, 1e-4, -1e-4, 0.0]), newK


def kernel(case):
    """the case's filter: a (kh, kw) array or a (ky, kx) pair.  Nothing symmetric: factors are random + 0.1,
    normalised, ky and kx drawn separately; dense kernels random + 0.1 (full rank)."""
    kind = case.filt[0]
    rng = np.random.default_rng(7000 + 31 * case.filt[1] + case.filt[-1] + {'dense': 0, 'sep': 1, 'rank1': 2, 'near1': 2}[kind])
    if kind == 'dense':
        k = rng.random(case.filt[1:]) + 0.1
        return k / k.sum()
    nky, nkx = (case.filt[1], case.filt[2]) if kind == 'sep' else (case.filt[1], case.filt[1])
    ky, kx = rng.random(nky) + 0.1, rng.random(nkx) + 0.1
    ky, kx = ky / ky.sum(), kx / kx.sum()
    if kind == 'sep':
        return ky, kx
    k = np.outer(ky, kx)
    if kind == 'near1':
        k[0, 0] *= 1 + 1e-9
    return k


def inputs(case, oracle):
    """-> dict: src (n, h, w), the filter, and the coordinate source's arrays"""
    inp = {'src': source(case), 'filt': kernel(case)}
    if case.coords == 'maps':
        inp['mx'], inp['my'] = maps(case.shape)
    elif case.coords == 'lens':
        inp['K'], inp['dist'], inp['newK'] = lens(case.shape)
    else:
        inp['M'] = homography(case.shape)
    return inp


ORC_INTERP = {'linear': 'LINEAR', 'cubic': 'CUBIC_KEYS', 'cubic_cv': 'CUBIC_CV', 'lanczos4': 'LANCZOS4'}
_MID = {}


def remapped(case, inp, oracle, f):
    """the oracle's remap of frame f, rounded to float32 as the kernels round the remapped rows; computed once
    per (frames, coordinates, interpolation, geometry, frame) and left unchanged"""
    key = (case.sdt, case.coords, case.interp, case.shape, f)
    if key not in _MID:
        oi = getattr(oracle, ORC_INTERP[case.interp])
        src, cval, hw = inp['src'][f], BORDER_VALUE[case.sdt], SHAPES[case.shape]
        if case.coords == 'maps':
            m = oracle.remap(src, inp['mx'], inp['my'], oi, 'constant', cval, out_dtype=np.float32)
        elif case.coords == 'lens':
            m = oracle.undistort(src, inp['K'], inp['dist'], inp['newK'], oi, 'constant', cval, out_dtype=np.float32,
                                 out_shape=hw)
        else:
            m = oracle.warp_perspective(src, inp['M'], hw, oi, 'constant', cval, out_dtype=np.float32)
        assert m.dtype == np.float32 and m.shape == hw
        m.setflags(write=False)
        _MID[key] = m
    return _MID[key]


def filtered(mid, filt):
    """tests/conv_ref.py in float64, the filter's border mode 'reflect' on both axes"""
    return ref_sepconv2d(mid, filt[0], filt[1]) if isinstance(filt, tuple) else ref_conv2d(mid, filt)


def expected(case, inp, oracle, f):
    return filtered(remapped(case, inp, oracle, f), inp['filt'])


def rounding_bound(case, inp, oracle, f):
    """conv_ref.bound() of the filter on the remapped frame: what the log shows the margin against"""
    return bound(remapped(case, inp, oracle, f), inp['filt'])


def tolerance(case):
    """(rtol, atol): what tests/test_gpu_fused_batches.py and test_gpu_rank1.py hold the chains to"""
    return 1e-5, 1e-5 * VALUE_RANGE[case.sdt]


def turned(filt):
    """the filter with its taps turned round: name -> filter"""
    if isinstance(filt, tuple):
        ky, kx = filt
        return {'ky reversed': (ky[::-1], kx), 'kx reversed': (ky, kx[::-1]), 'ky and kx exchanged': (kx, ky)}
    return {'flipped': filt[::-1, ::-1], 'flipped vertically': filt[::-1], 'transposed': filt.T}


# ---------------------------------------------------- which strips take the fast branch --
def strip_geometry(filt):
    """-> (K, separable, OW, HL) of the kernel a one-kernel case launches: wave_geom / sep_geom without the
    halo pass (no sampling source takes it)"""
    kind = filt[0]
    K = filt[1]
    if kind in ('sep', 'rank1'):
        hl = max((K // 2 + 3) // 4, 2)
    else:
        hl = max((K // 2 + 3) // 4, {3: 2, 5: 2, 7: 1, 9: 2}.get(K, 1))
    return K, kind in ('sep', 'rank1'), 256 - 8 * hl, hl


def fast_strips(K, ow, hl, dh, dw, depth, strip_h=STRIP_H, vec_out=True):
    """the `fast` predicate of wave_stencil_body and wave_sep_kernel (uniform strips, no halo pass) restated:
    -> (fast in x per strip column, fast in y per strip row, first column of every strip)"""
    H = K // 2
    xs = [sx * ow - 4 * hl for sx in range((dw + ow - 1) // ow)]
    fx = [vec_out and x >= 0 and x + 256 <= dw for x in xs]
    fy = []
    for y0 in range(0, dh, strip_h):
        nrows = min(strip_h, dh - y0)
        touched = ((nrows + K - 1 + depth - 1) // depth) * depth
        fy.append(y0 - H >= 0 and y0 - H + touched <= dh)
    return fx, fy, xs


def interior_mask(filt, shape, depth=2):
    """bool (dh, dw): the pixels fast strips WRITE (lanes HL .. 63 - HL of interior strip columns, interior strip
    rows); depth 2 is the deepest chunk of any sampling kernel, so what is interior here is interior at depth 1"""
    K, _, ow, hl = strip_geometry(filt)
    dh, dw = SHAPES[shape]
    fx, fy, xs = fast_strips(K, ow, hl, dh, dw, depth)
    m = np.zeros((dh, dw), bool)
    for r, okr in enumerate(fy):
        for c, okc in enumerate(fx):
            if okr and okc:
                m[r * STRIP_H:(r + 1) * STRIP_H, xs[c] + 4 * hl:min(xs[c] + 256 - 4 * hl, dw)] = True
    return m


def path_names(mask):
    return '|'.join(n for k, n in enumerate(BIT_NAMES) if mask >> k & 1) or '0'
