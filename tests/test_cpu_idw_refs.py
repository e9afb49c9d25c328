"""CPU: the float64 references of the structured IDW fills (tests/idw_ref.py) against the oracle
and the reference's own outputs in tests/golden/idw.npz; the case table of tests/idw_cases.py
proven to stand on every branch of fast_idw_kernel's batched walk and on both idw_kernel
variants; and wrong variants of the references shown to fail a case under the bound the GPU
tests use.

The control: replayed through the reference's sequential walk, no fast-IDW case that the suite
ran before this file - test_idw_edges_vs_oracle, test_idw_kernel_boundaries_vs_oracle and the
fidw_* / block entries of idw.npz - stops at a neighbour index of 64 or more (the largest is 49),
and the only pixels that walk to the end of the list have 48 neighbours: the carry of the hit
count from one batch of 64 to the next never ran.
"""
import numpy as np
import pytest

from . import idw_cases as ic
from . import idw_ref as ref
from .conftest import load_golden


def _close(got, res, dtype, what):
    r = ref.worst(got, res, dtype)
    assert r <= 1.0, '%s: err / bound %.3g' % (what, r)
    return r


def test_references_equal_the_fixture():
    g = load_golden('idw.npz')
    grid = g['grid']
    n = 0
    for key, want in g.items():
        p = key.split('_')
        if key.startswith('idw_k'):
            kern, power = int(p[1][1:]), int(p[2][1:])
            fx, fy = (2, 0.5) if len(p) > 3 else (1, 1)
            res = ref.idw_fill(grid, g['mask_k%d' % kern], kern, ref.weights_of(kern, power, fx, fy))
        elif key.startswith('fidw_k'):
            kern, power, minn = int(p[1][1:]), int(p[2][1:]), int(p[3][1:])
            offs, wts = ref.neighbours_of(kern, power)
            res = ref.fast_idw_fill(grid, g['mask_k%d' % kern], offs, wts, minn - 1)
        else:
            continue
        _close(want, res, np.float64, key)
        n += 1
    assert n == 21
    _close(g['idw32_k5_p2'], ref.idw_fill(grid.astype(np.float32), g['mask_k5'], 5, ref.weights_of(5)),
           np.float32, 'idw32')
    _close(g['idw_block_k3'], ref.idw_fill(grid, g['mask_block'], 3, ref.weights_of(3)), np.float64, 'block')
    offs, wts = ref.neighbours_of(3)
    _close(g['fidw_block_k3'], ref.fast_idw_fill(grid, g['mask_block'], offs, wts, 4), np.float64, 'fast block')


def test_references_equal_the_oracle_on_the_case_table(oracle):
    for dt in (np.float32, np.float64):
        for c in ic.FAST:
            g, res = ic.fast_ref(c, dt)
            got = oracle.interpolate2dStructuredFastIDW(g.copy(), c['mask'], c['k'], 2, c['minnvals'] + 1)
            _close(got, res, dt, 'fast ' + c['name'])
        for c in ic.IDW:
            if c['centre_weight']:
                continue   # the oracle builds its own weight table
            g, wts, res = ic.idw_ref_of(c, dt)
            got = oracle.interpolate2dStructuredIDW(g.copy(), c['mask'], c['k'], 2)
            _close(got, res, dt, 'idw ' + c['name'])


def _old_fast_cases():
    """every fast-IDW call of the suite before this file: (grid, mask, k, minnvals of the wrapper)"""
    g = load_golden('idw.npz')
    for key in g:
        if key.startswith('fidw_k'):
            p = key.split('_')
            yield key, g['grid'], g['mask_k%d' % int(p[1][1:])], int(p[1][1:]), int(p[3][1:])
    yield 'fidw_block_k3', g['grid'], g['mask_block'], 3, 5
    for seed, shapes in ((8, ((40, 150), (65, 64), (7, 9))), (9, ((40, 150), (65, 64)))):
        rng = np.random.default_rng(seed)
        for s in shapes:
            grid = rng.random(s)
            yield 'seed %d %s' % (seed, s), grid, rng.random(s) < 0.3, 4, 5


def test_control_no_older_case_leaves_the_first_batch():
    worst_stop, ends = -1, set()
    for name, grid, mask, k, minn in _old_fast_cases():
        offs, wts = ref.neighbours_of(k)
        res = ref.fast_idw_fill(grid, mask, offs, wts, minn - 1)
        # the hit count reset at every 64th neighbour passes every one of them
        reset = ref.fast_idw_fill(grid, mask, offs, wts, minn - 1, 'reset64')
        assert np.array_equal(res['out'], reset['out'], equal_nan=True), name
        m = np.asarray(mask, bool)
        stopped = m & (res['reason'] != ref.END)
        if stopped.any():
            worst_stop = max(worst_stop, int(res['stop'][stopped].max()))
        if (m & (res['reason'] == ref.END)).any():
            ends.add(len(offs))
    print('older fast-IDW cases: largest stop index %d, lists walked to the end: %s' % (worst_stop, sorted(ends)))
    assert worst_stop == 49 and ends == {48}


def test_fast_case_table_covers_every_class():
    seen = {}
    for c in ic.FAST:
        assert c['shape'][0] <= 40 and c['shape'][1] <= 70
        cls = ic.fast_classes(c, ic.fast_ref(c, np.float64)[1])
        for k in cls:
            seen.setdefault(k, []).append(c['name'])
    for k in ic.FAST_CLASSES:
        print('%-24s %s' % (k, ', '.join(seen.get(k, []))))
    assert set(ic.FAST_CLASSES) <= set(seen), set(ic.FAST_CLASSES) - set(seen)
    # 1088 neighbours are exactly 17 batches, 80 and 288 end on a partial one
    assert [len(ref.neighbours_of(k)[0]) for k in (4, 8, 16)] == [80, 288, 1088] and 1088 == 17 * 64


def test_idw_case_table_states_the_kernels():
    want = {1: ('taps', 0), 7: ('taps', 0), 8: ('rows', 2), 15: ('rows', 2), 16: ('rows', 1), 31: ('rows', 1),
            32: ('taps', 0)}
    have = {}
    for c in ic.IDW:
        have.setdefault(c['k'], set()).add(c['kernel'])
        g, wts, res = ic.idw_ref_of(c, np.float64)
        m = c['mask']
        h, w = c['shape']
        if 'main' in c['name']:
            assert m[0, 0] and m[0, w - 1] and m[h - 1, 0] and m[h - 1, w - 1] and res['filled'][m].all()
        if 'masked window' in c['name']:
            assert (m & ~res['filled']).any() and (m & res['filled']).any()
        if c['nan']:
            assert np.isnan(res['out'][m]).any() and not np.isnan(res['out'][m]).all()
    assert have == {k: {v} for k, v in want.items()}
    shapes = {(c['k'], c['shape']) for c in ic.IDW}
    assert {(k, s) for k in (8, 16, 31) for s in ((7, 9), (3, 70))} <= shapes
    assert {(k, (6, w)) for k in (1, 8, 16) for w in (64, 65, 128, 129)} <= shapes
    assert any(c['centre_weight'] for c in ic.IDW)


FAST_DEFECTS = ('reset64', 'no_stop_hit', 'far_or', 'far_no_c')


@pytest.mark.parametrize('defect', FAST_DEFECTS + ('centre', 'mask_pitch fast', 'mask_pitch idw'))
def test_wrong_variants_fail_a_case(defect):
    """each wrong variant of a reference exceeds, on at least one case, the bound under which the
    device result is held against the exact one (float32 grids: the wider of the two bounds)"""
    failed = []
    for dt in (np.float32,):
        if defect in FAST_DEFECTS or defect == 'mask_pitch fast':
            for c in ic.FAST:
                pitch = c['shape'][1] + ic.PITCH_PAD
                g, res = ic.fast_ref(c, dt)
                bad = ic.fast_ref(c, dt, defect.split()[0], pitch)[1]['out'].astype(dt)
                try:
                    if ref.worst(bad, res, dt) > 1.0:
                        failed.append(c['name'])
                except AssertionError:
                    failed.append(c['name'])
        else:
            for c in ic.IDW:
                pitch = c['shape'][1] + ic.PITCH_PAD
                g, wts, res = ic.idw_ref_of(c, dt)
                bad = ic.idw_ref_of(c, dt, defect.split()[0], pitch)[2]['out'].astype(dt)
                try:
                    if ref.worst(bad, res, dt) > 1.0:
                        failed.append(c['name'])
                except AssertionError:
                    failed.append(c['name'])
    print('%s fails: %s' % (defect, ', '.join(sorted(set(failed)))))
    assert failed
