"""CPU-only: the numpy restatement of single-time-effect removal (features/
SingleTimeEffectDetection.py:13-75 with a given noise level function) equals the reference's own
outputs in tests/golden/ste.npz bit for bit, and the parts that are not on the GPU path refuse
before any device is touched.  The GPU tests (test_gpu_ste.py) compare the kernel with both.

The second half proves what the scenes of tests/ste_cases.py are sensitive to: SteTiles, a numpy
emulation of ste_kernel's tile algorithm, equals the restatement in its exact form and differs
from it on a new scene under every defect listed there - and does NOT differ on the older random
scenes when the halo is one ring short and a launch has more than one step.
"""
import numpy as np
import pytest

from .conftest import load_golden


def bounded_nlf(x, min_y, ax, ay):
    """NoiseLevelFunction.boundedFunction (camera/NoiseLevelFunction.py:94-107)"""
    with np.errstate(invalid='ignore'):
        y = ay * np.sqrt(x - ax)
    return np.maximum(np.nan_to_num(y), min_y)


def remove_single_pixels(s):
    """filters/removeSinglePixels.py:4-30 as one parallel pass (a cleared pixel has no set
    neighbour, so clearing it changes no other decision)"""
    h, w = s.shape
    p = np.zeros((h + 2, w + 2), dtype=bool)
    p[1:-1, 1:-1] = s
    nb = np.zeros((h, w), dtype=bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if dy == 1 and dx == 1:
                continue
            nb |= p[dy:dy + h, dx:dx + w]
    return s & nb


class SteNumpy(object):
    """the contract of the issue, step by step: float64 throughout, NaN-propagating min / max"""

    def __init__(self, frames, nlf, nstd, thr=None):
        f0 = np.asarray(frames[0]).astype(np.float64)
        f1 = np.asarray(frames[1])
        self.avg = np.min((f0, f1), axis=0)
        self.count = np.ones(self.avg.shape, dtype=np.int64)
        self.thr = bounded_nlf(self.avg, *nlf) * nstd if thr is None else thr
        self.mask_ste = np.zeros(self.avg.shape, dtype=bool)
        self.add(np.max((f0, f1), axis=0))
        for f in frames[2:]:
            self.add(f)

    def add(self, g, mask=None):
        d = g - self.avg
        with np.errstate(invalid='ignore'):
            s = remove_single_pixels(d > self.thr)
        self.mask_clean = ~s
        clean = self.mask_clean if mask is None else self.mask_clean & mask
        self.count[clean] += 1
        a = self.avg[clean]
        self.avg[clean] = a + (np.asarray(g, dtype=np.float64)[clean] - a) / self.count[clean]
        self.mask_ste |= s
        return self


def same_f64(a, b):
    """bit equality of float64 arrays, NaN positions equal"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na],
                                                          b.view(np.int64)[~nb]))


def test_restatement_equals_reference_golden():
    g = load_golden('ste.npz')
    n = int(g['n_cases'])
    assert n == 12 and str(g['mma_source'])
    for i in range(n):
        p = 'c%d_' % i
        s = SteNumpy(g[p + 'frames'], tuple(g[p + 'nlf']), float(g[p + 'nstd']))
        assert same_f64(s.thr, g[p + 'thr']), p + 'thr'
        assert same_f64(s.avg, g[p + 'noSTE']), p + 'noSTE'
        assert np.array_equal(s.mask_clean, g[p + 'mask_clean']), p + 'mask_clean'
        assert np.array_equal(s.mask_ste, g[p + 'mask_ste']), p + 'mask_ste'
        s.add(g[p + 'add'], g[p + 'add_mask'])
        assert same_f64(s.avg, g[p + 'noSTE2']), p + 'noSTE2'
        assert np.array_equal(s.mask_clean, g[p + 'mask_clean2']), p + 'mask_clean2'
        assert np.array_equal(s.mask_ste, g[p + 'mask_ste2']), p + 'mask_ste2'
    for j in range(int(g['n_rsp'])):
        assert np.array_equal(remove_single_pixels(g['rsp%d_in' % j]), g['rsp%d_out' % j])


def test_golden_covers_the_contract():
    g = load_golden('ste.npz')
    kinds = set()
    for i in range(int(g['n_cases'])):
        p = 'c%d_' % i
        f = g[p + 'frames']
        kinds.add((f.dtype.name, f.shape[0], float(g[p + 'nstd'])))
        if f.dtype.kind == 'f':
            assert np.isnan(f).any()
        assert g[p + 'mask_ste'].any()
    assert {k[0] for k in kinds} == {'uint8', 'uint16', 'float32', 'float64'}
    assert {k[1] for k in kinds} == {2, 3, 5} and {k[2] for k in kinds} == {4.0, 2.5}


def _ste():
    from imgprocessor_amd.features import SingleTimeEffectDetection
    return SingleTimeEffectDetection


def test_ste_refusals_need_no_device():
    S = _ste()
    stack = [np.zeros((4, 5)), np.zeros((4, 5))]
    with pytest.raises(NotImplementedError):
        S(stack)                                    # NLF estimation (oneImageNLF)
    with pytest.raises(NotImplementedError):
        S(stack, (1.0, 0.0, 1.0), calcVariance=True)
    with pytest.raises(NotImplementedError):
        S(stack, (1.0, 0.0, 1.0), dtype=np.float32)
    with pytest.raises(TypeError):
        S(['a.tif', 'b.tif'], (1.0, 0.0, 1.0))
    with pytest.raises(TypeError):
        S([np.zeros((4, 5, 3))] * 2, (1.0, 0.0, 1.0))   # colour frames
    with pytest.raises(TypeError):
        S(np.zeros((2, 4, 5, 3)), (1.0, 0.0, 1.0))
    with pytest.raises(TypeError):
        S(stack, (1.0, 0.0))                        # not a triple
    obj = object.__new__(S)
    with pytest.raises(NotImplementedError):
        obj.countSTE()
    with pytest.raises(NotImplementedError):
        obj.intensityDistributionSTE()


def test_ste_abi_declared():
    from imgprocessor_amd import _lib
    assert 'ipa_ste_dev' in _lib.PROTOTYPES and 'ipa_remove_single_pixels_dev' in _lib.PROTOTYPES
    lib = _lib.lib()
    assert hasattr(lib, 'ipa_ste_dev') and hasattr(lib, 'ipa_remove_single_pixels_dev')
    assert lib.ipa_ste_dev(None, None, 0, 2, 1, 1, 1, 1, 1, None, 4.0, None, None, None, 1, None,
                           None, None, 1) == _lib.ERR_BAD_ARG


def test_device_arrays_refuse_int32_outside_the_counts():
    from imgprocessor_amd import DeviceArray
    with pytest.raises(TypeError):
        DeviceArray(None, (2, 2), np.int32)   # refused before any allocation


# ------------------------------------------------- what the scenes of ste_cases.py can see ----
from . import ste_cases as sc   # noqa: E402

OLD_N = (2, 3, 4, 7, 8, 9, 16, 17)   # test_ste_frame_counts


def _old(n):
    return sc.random_scene(n, 150, 260, np.float32, 10 + n)


def _tiles_of(kind, key, defect=None):
    """SteTiles run over a case of the table the way the GPU test calls the library"""
    if kind == 'fuse':
        return sc.SteTiles(sc.fuse_case(key)[0], sc.NLF_CONST, sc.NSTD_CONST, defect)
    if kind == 'cont':
        fr, _, m = sc.cont_case(key)[:3]
        return sc.SteTiles(fr[:2], sc.NLF_CONST, sc.NSTD_CONST, defect).add(fr[2:], m)
    return sc.SteTiles(sc.adj_case(*key)[0], sc.NLF_CONST, sc.NSTD_CONST, defect)


def _ref_of(kind, key):
    return {'fuse': sc.fuse_case, 'cont': sc.cont_case}[kind](key)[-2 if kind == 'cont' else -1] \
        if kind != 'adj' else sc.adj_case(*key)[-1]


ALL_NEW = ([('fuse', s) for s in sc.FUSE_STEPS] + [('cont', m) for m in sc.CONT_MORE] +
           [('adj', (st, dt)) for st in sc.ADJ_STEPS for dt in sc.ADJ_DTYPES])


def test_tile_emulation_equals_the_restatement():
    """exact halo, all rows exchanged, carry across the seam, separate input and output state:
    the same bits as SteNumpy on every new scene and on the older random ones"""
    for kind, key in ALL_NEW:
        assert sc.same_state(_tiles_of(kind, key), _ref_of(kind, key)), (kind, key)
    for n in OLD_N:
        fr = _old(n)
        assert sc.same_state(sc.SteTiles(fr, sc.NLF, 2.5), SteNumpy(fr, sc.NLF, 2.5)), n
        assert sc.same_state(sc.SteTiles(fr, sc.NLF, 2.5, per_launch=1), SteNumpy(fr, sc.NLF, 2.5)), n


def test_fuses_burn_as_described():
    """P is an STE in the last step of its launch if and only if the fuse was lit; every launch
    has a lit fuse for every end and direction in its own tiling, one for every end in the tiling
    that a halo of st - 1 would give, and unlit and (from 3 steps) soft ones next to them"""
    for steps in sc.FUSE_STEPS:
        fr, fuses, ref = sc.fuse_case(steps)
        assert np.all(ref.thr == sc.THR_CONST)
        r = SteNumpy(fr[:2], sc.NLF_CONST, sc.NSTD_CONST)
        per = [~r.mask_clean]
        for f in fr[2:]:
            per.append(~r.add(f).mask_clean)
        have = set()
        for f in fuses:
            assert per[f['last_step']][f['P']] == (f['kind'] != 'unlit'), f
            assert len(f['px']) == f['S'] + 1
            have.add((f['launch'], f['tiling'], f['end'], f['u'], f['kind']))
        launches = sc.split_steps(steps)
        for li, st in enumerate(launches):
            for tiling in ('exact', 'short'):
                for end, dirs in sc.INBOUND.items():
                    lit = {k[3] for k in have if k[:3] == (li, tiling, end) and k[4] == 'lit'}
                    assert lit == set(dirs) if tiling == 'exact' else lit, (steps, li, tiling, end)
                    kinds = {k[4] for k in have if k[:3] == (li, tiling, end)}
                    assert 'unlit' in kinds and ('soft' in kinds or st < 3), (steps, li, tiling, end)
        dirs = {f['u'] for f in fuses}
        assert dirs == set(sc.DIRS8)
    assert {len(sc.split_steps(s)) for s in sc.FUSE_STEPS} == {1, 2, 3}
    assert {st for s in sc.FUSE_STEPS for st in sc.split_steps(s)} >= set(range(1, 9))
    # the continuing calls: one launch after a copy, two without, three with; the mask lights fuses
    assert [len(sc.split_steps(m)) for m in sc.CONT_MORE] == [1, 1, 2, 2, 3]
    for m in sc.CONT_MORE:
        fr, fuses, mask, ref, hit = sc.cont_case(m)
        assert hit and all(ref.mask_ste[f['P']] for f in hit)
        plain = SteNumpy(fr, sc.NLF_CONST, sc.NSTD_CONST)
        assert all(plain.avg[f['P']] > ref.avg[f['P']] for f in hit)   # unmasked, P absorbs its 1000


def test_adjacency_scenes_cover_their_classes():
    for st in sc.ADJ_STEPS:
        fr, pairs, ref = sc.adj_case(st, np.float64)
        for step in range(min(st, 2)):   # both slots of edge[] where the launch has two steps
            cls = {p[1] for p in pairs if p[0] == step}
            assert cls >= {'wave %d|%d' % (r, r + 1) for r in range(7, 56, 8)} | {
                'seam', 'tile x', 'tile y', 'top', 'bottom', 'left', 'right', 'corner'}
            for c in cls - {'top', 'bottom', 'left', 'right', 'corner'}:
                assert len({p[4] for p in pairs if p[0] == step and p[1] == c}) == 3, c
        us = {p[4] for p in pairs} | {(-p[4][0], -p[4][1]) for p in pairs}
        assert us == set(sc.DIRS8)
        for step, c, a, b, u in pairs:           # every pair survives, as a pair
            assert ref.mask_ste[a] and ref.mask_ste[b], (st, c)
        assert ref.mask_ste.sum() == len({p[2] for p in pairs} | {p[3] for p in pairs})
        for dt in sc.ADJ_DTYPES:
            assert sc.same_state(sc.adj_case(st, dt)[2], ref)


def test_every_defect_is_seen_by_a_new_scene():
    """each defect of the tile algorithm differs from SteNumpy on a new scene; the halo one ring
    short in any single launch of a call is seen by that call's fuse scene"""
    def differs(kind, key, defect):
        return not sc.same_state(_tiles_of(kind, key, defect), _ref_of(kind, key))
    for steps in sc.FUSE_STEPS:
        for li in range(len(sc.split_steps(steps))):
            assert differs('fuse', steps, ('halo', li)), (steps, li)
    for m in sc.CONT_MORE:                       # launch 0 is the first pair's
        for li in range(1, 1 + len(sc.split_steps(m))):
            assert differs('cont', m, ('halo', li)), (m, li)
        assert differs('cont', m, 'inplace'), m
    for steps in (12, 16, 17):
        assert differs('fuse', steps, 'inplace'), steps
    for st in sc.ADJ_STEPS:
        for dt in sc.ADJ_DTYPES:
            assert differs('adj', (st, dt), 'waves') and differs('adj', (st, dt), 'seam'), (st, dt)


def test_control_random_scenes_do_not_see_a_short_halo():
    """The control: on the random scenes of test_ste_frame_counts (1 % hits, no dependency chain
    longer than one pixel across a tile border) a halo one ring short is seen for n = 2 only -
    single-step launches - and for no n >= 3, in any launch or in all of them."""
    seen = {}
    for n in OLD_N:
        fr = _old(n)
        ref = SteNumpy(fr, sc.NLF, 2.5)
        which = ['all'] + list(range(len(sc.split_steps(n - 1))))
        seen[n] = any(not sc.same_state(sc.SteTiles(fr, sc.NLF, 2.5, ('halo', i)), ref) for i in which)
    print('short halo seen on the random scenes: %s' % seen)
    assert seen == {n: n == 2 for n in OLD_N}
