"""CPU-only: temporal signal stability (csrc/tss.hip, uncertainty/temporalSignalStability.py)
without a device.

  * the numpy / scipy restatement (tests/tss_ref.py) against the reference's own outputs
    (tests/golden/tss.npz);
  * the count form the kernel rests on against scipy's median, bit for bit on the event cube,
    over the whole case table (tests/tss_cases.py);
  * what the scenes are for: ties and counts of exactly 62 and 63 in the lattice scenes, 25 samples
    a plane in the plane scenes, the run counter on its own;
  * sensitivity: every defect a kernel could have (tss_ref.DEFECTS) changes the result of some
    scene, and every scene of the case table of 2, 5, 9 and 17 frames is changed by some defect -
    a scene that no defect changes proves nothing, which is why the table holds no one-pixel
    lattice and no border scene along an axis shorter than six.  Not every scene can see every
    defect: a halo that is one ring short cannot show in a one-tile image, a second reflection
    only where an axis has one sample.  The other frame counts run the same generators; there a
    one-pixel fitted scene can be blind by construction (the residuals of a line through three
    samples are all beyond half their rms, so every frame is an event whatever the defect) and is
    kept because the table asks for that shape in every type;
  * the refusals that need no device, the binding and the exports.
"""
import numpy as np
import pytest

from .conftest import load_golden
from . import tss_cases as tc
from . import tss_ref as ref
from .test_cpu_dark import same


@pytest.fixture(scope='module')
def g():
    return load_golden('tss.npz')


def unpack(bits, shape):
    return np.unpackbits(bits, count=int(np.prod(shape))).reshape(shape).astype(bool)


# ------------------------------------------------------------------ the fixture
@pytest.mark.parametrize('name', ('demo', 'demo16'))
def test_restatement_equals_the_fixture(g, name):
    """error, ascent, offset: bit for bit.  Events and raw event length: equal where the fixture's
    regression is the restatement, else on the stable-decision mask.  The final map: the zeros
    exactly, the rest within the tolerance test_cpu_stencil_refs grants masked_mean in float64
    (the reference sums its 7 x 7 window in plain float64, stencil_ref in extended precision; the
    maximum and the median after it only select)."""
    times, frames = getattr(tc, name)()
    p = name + '_'
    assert same(np.array([f.astype(np.float64).sum() for f in frames]), g[p + 'in_sum']), 'another scene'
    assert same(np.asarray(times, np.float64), g[p + 'times'])
    got = ref.temporal_signal_stability(frames, times)
    for k in ('error', 'ascent', 'offset'):
        assert same(got[k], g[p + k]), k
    events, stable = unpack(g[p + 'events'], frames.shape), unpack(g[p + 'stable'], frames.shape)
    assert float(g['unstable_worst']) <= 0.01
    if str(g['linreg_source']) == 'restatement':
        assert np.array_equal(got['events'], events) and same(got['raw'], g[p + 'raw'])
    else:
        assert np.array_equal(got['events'][stable], events[stable])
        ok = np.all(stable, axis=0)
        assert same(got['raw'][ok], g[p + 'raw'][ok])
    want = g[p + 'avlen']
    assert np.array_equal(got['avlen'] == 0, want == 0)
    np.testing.assert_allclose(got['avlen'], want, rtol=1e-13, atol=1e-15)
    # the count form end to end
    counted = ref.temporal_signal_stability(frames, times, events=ref.events_count)
    assert np.array_equal(counted['events'], got['events']) and same(counted['avlen'], got['avlen'])
    assert events.any() and not events.all() and (want > 0).any() and (want == 0).any()


# ------------------------------------------------------------------ count form == median form
@pytest.mark.parametrize('T', tc.T_VALUES)
def test_count_form_equals_median_form(T):
    n_evt = 0
    for kind, shape, dt, v in tc.case_ids(T):
        sc = tc.scene(kind, T, shape, dt, v)
        want, raw = tc.reference(kind, T, shape, dt, v)
        got = ref.events_count(*sc)
        assert np.array_equal(got, want), (kind, T, shape, dt, v, int((got != want).sum()))
        assert same(ref.run_lengths(got), raw)
        n_evt += int(want.sum())
    assert n_evt > 0


def test_lattice_scenes_sit_on_the_decisions():
    """every multi-tile lattice scene of five or more frames has windows at counts of exactly 62
    and 63 and samples equal to c (the float types: to -c as well).  Shorter stacks and smaller
    images quantise the counts (a 1 x 1 image: to multiples of 25)."""
    for T in tc.T_VALUES:
        if T < 5:
            continue
        for dt in tc.ALL_DTYPES:
            st, times, off, asc, err = tc.scene('lattice', T, tc.MULTI, dt, 0)
            cp, cm = ref.window_counts(*ref.plane_counts(st, times, off, asc, err))
            counts = np.concatenate([cp.ravel(), cm.ravel()]) if np.dtype(dt).kind == 'f' else cp.ravel()
            assert (counts == 62).any() and (counts == 63).any(), (T, dt)
            r = st.astype(np.float64)
            assert (r == 0.5 * err[None]).any(), (T, dt)
            if np.dtype(dt).kind == 'f':
                assert (r == -0.5 * err[None]).any() and (cm == 62).any() and (cm == 63).any(), (T, dt)


def test_plane_scenes_count_25_a_plane_and_test_the_run_counter():
    seen = set()
    for T in tc.T_VALUES:
        for v in range(2):
            st, times, off, asc, err = tc.scene('planes', T, (5, 7), np.float32, v)
            hot = tc.z_pattern(T, v)
            cp, cm = ref.window_counts(*ref.plane_counts(st, times, off, asc, err))
            k = np.arange(T)
            n_hot = sum(hot[ref._reflect(k + dz, T)].astype(int) for dz in range(-2, 3))
            assert np.array_equal(cp, np.broadcast_to(25 * n_hot[:, None, None], cp.shape)) and not cm.any()
            evt = ref.events_count(st, times, off, asc, err)
            assert np.array_equal(evt[:, 2, 3], n_hot >= 3)
            assert same(ref.run_lengths(evt), ref.run_lengths_grouped(evt))
            # run lengths and gaps that occur
            e = ''.join('1' if b else '0' for b in evt[:, 0, 0])
            seen |= {(ch, len(run)) for ch in '01' for run in e.split('0' if ch == '1' else '1') if run}
    assert {(ch, n) for ch in '01' for n in (1, 2, 3, 4, 5)} <= seen, sorted(seen)


def test_run_counter_on_random_cubes():
    rng = np.random.default_rng(3)
    for T in (2, 3, 7, 64):
        evt = rng.random((T, 6, 9)) < 0.5
        evt[:, 0, 0], evt[:, 0, 1] = False, True
        a = ref.run_lengths(evt)
        assert same(a, ref.run_lengths_grouped(evt)) and a[0, 0] == 0 and a[0, 1] == T
        if T >= 3:
            assert not same(ref.run_lengths(evt, merge=True), a)


# ------------------------------------------------------------------ sensitivity
# the whole case table of four frame counts - the shortest, one that is exactly the window, and two
# longer ones - and a few scenes beside it
SENS_T = (2, 5, 9, 17)
SENS = [(kind, T, shape, dt, v) for T in SENS_T for kind, shape, dt, v in tc.case_ids(T)]
SENS += [('continuous', 16, tc.MULTI, np.uint16, 0), ('continuous', 6, (5, 7), np.float32, 0),
         ('borders_x', 6, tc.MULTI, np.float32, 1), ('borders_y', 3, tc.MULTI, np.float64, 1)]


def changed_by(case, defect):
    sc = tc.scene(*case)
    want, raw = tc.reference(*case)
    if defect == 'merge_runs':
        return not same(ref.run_lengths(want, merge=True), raw)
    return not np.array_equal(ref.events_count(*sc, defect=defect), want)


@pytest.fixture(scope='module')
def sensitivity():
    return {(case[0], case[1], case[2], np.dtype(case[3]).name, case[4], d): changed_by(case, d)
            for case in SENS for d in ref.DEFECTS}


def test_every_defect_changes_some_scene_and_every_scene_sees_some_defect(sensitivity):
    for d in ref.DEFECTS:
        hit = [k[:5] for k, v in sensitivity.items() if k[5] == d and v]
        print('%-13s changes %d of %d scenes' % (d, len(hit), len(SENS)))
        assert hit, 'no scene notices %s' % d
    for case in SENS:
        key = (case[0], case[1], case[2], np.dtype(case[3]).name, case[4])
        assert any(v for k, v in sensitivity.items() if k[:5] == key), 'scene %s sees no defect' % (key,)


def test_what_each_kind_of_scene_is_for(sensitivity):
    def sees(kind, defect, shape=None):
        return any(v for k, v in sensitivity.items()
                   if k[0] == kind and k[5] == defect and (shape is None or k[2] == shape))
    # the lattice: the majority and the strictness of the comparison
    assert sees('lattice', 'thr62') and sees('lattice', 'thr64') and sees('lattice', 'ge')
    assert sees('lattice', 'nb_threshold')
    # an axis of one sample reflects more than once
    assert sees('continuous', 'reflect_once', (1, 1)) and sees('planes', 'reflect_once', (1, 1))
    # the planes: reflection along the frames and the run counter
    assert sees('planes', 'clamp_z') and sees('planes', 'merge_runs')
    # the borders: the halo's outer ring and the reflection in x and y
    for kind in ('borders_x', 'borders_y'):
        assert sees(kind, 'halo_short') and sees(kind, 'clamp_xy')
    # a fitted scene: a halo sample lies on its own pixel's line
    assert sees('continuous', 'centre_line', tc.MULTI)


def test_border_probes_are_decided_beyond_the_tile():
    """at the first and last output pixel of a tile and at the image corners the alternating
    scenes' decisions flip when the halo is a ring short or the edge is repeated"""
    T, (h, w) = 5, tc.MULTI
    flipped_halo, flipped_edge = set(), set()
    for kind, axis in (('borders_x', 2), ('borders_y', 1)):
        for v in range(2):
            sc = tc.scene(kind, T, tc.MULTI, np.float32, v)
            want = ref.events_count(*sc)
            short, clamp = ref.events_count(*sc, defect='halo_short'), ref.events_count(*sc, defect='clamp_xy')
            for p in tc.probes(T, h, w):
                if short[p] != want[p]:
                    flipped_halo.add((axis, p[axis]))
                if clamp[p] != want[p]:
                    flipped_edge.add((axis, p[axis]))
    assert {(2, tc.TILE_W - 1), (2, tc.TILE_W), (2, 2 * tc.TILE_W - 1), (2, 2 * tc.TILE_W),
            (1, tc.TILE_H - 1), (1, tc.TILE_H)} <= flipped_halo, sorted(flipped_halo)
    assert {(2, 0), (2, w - 1), (1, 0), (1, h - 1)} <= flipped_edge, sorted(flipped_edge)


# ------------------------------------------------------------------ the 2-D tail
def test_finish_restates_the_reference_lines():
    rng = np.random.default_rng(11)
    raw = np.where(rng.random((23, 31)) < 0.3, 0.0, rng.integers(1, 6, (23, 31)) / rng.integers(1, 4, (23, 31)))
    mean, m0 = ref.masked_mean7(raw)
    assert np.array_equal(np.isnan(mean), m0)
    out = ref.finish(mean, m0)
    assert np.isfinite(out).all() and (out == 0).any() and (out > 0).any()
    # selection only: every value is one of the means, or zero
    assert np.isin(out[out != 0], mean[~m0]).all()


# ------------------------------------------------------------------ refusals, binding, exports
def test_refusals_need_no_device():
    from imgprocessor_amd import ops
    from imgprocessor_amd.uncertainty import temporalSignalStability
    fr = np.zeros((4, 5, 6), np.float32)
    t = np.arange(4.0)
    with pytest.raises(NotImplementedError):
        temporalSignalStability(fr, t, down_scale_factor=2)
    with pytest.raises(ValueError):
        temporalSignalStability(fr[:1], t[:1])
    with pytest.raises(NotImplementedError):
        temporalSignalStability(np.zeros((65, 2, 2), np.float32), np.arange(65.0))
    with pytest.raises(ValueError):
        temporalSignalStability(fr, t[:3])
    with pytest.raises(ValueError):
        temporalSignalStability(np.zeros((4, 5, 6, 3), np.uint8), t)
    with pytest.raises(ValueError):
        temporalSignalStability([np.zeros((5, 6, 3), np.uint8)] * 4, t)
    z = np.zeros((5, 6))
    for bad_fr, bad_t, exc in ((fr[:1], t[:1], ValueError), (np.zeros((65, 5, 6), np.float32), np.arange(65.0),
                                                             NotImplementedError), (fr, t[:3], ValueError)):
        with pytest.raises(exc):
            ops.tss_event_length(bad_fr, bad_t, z, z, z)


def test_binding_and_exports():
    from imgprocessor_amd import _lib, ops, ops_tss, uncertainty
    lib = _lib.lib()
    for n in ('ipa_tss_event_length_dev', 'ipa_tss_finish_dev'):
        assert n in _lib.PROTOTYPES and hasattr(lib, n)
    assert ops.tss_event_length is ops_tss.tss_event_length and ops.tss_finish is ops_tss.tss_finish
    assert uncertainty.temporalSignalStability.__module__.endswith('temporalSignalStability')
    assert callable(uncertainty.positionToIntensityUncertainty)
    assert (tc.TILE_W, tc.TILE_H, tc.MAX_FRAMES) == (64, 16, ops_tss.MAX_FRAMES)


def test_tile_constants_are_the_kernels():
    import os
    import re
    from .conftest import ROOT
    src = open(os.path.join(ROOT, 'imgprocessor_amd', 'csrc', 'tss.hip')).read()
    m = re.search(r'kTssTileW = (\d+), kTssTileH = (\d+)', src)
    assert (int(m.group(1)), int(m.group(2))) == (tc.TILE_W, tc.TILE_H)
    m = re.search(r'kFinW = (\d+), kFinH = (\d+)', src)
    assert (int(m.group(1)), int(m.group(2))) == (tc.FIN_TILE_W, tc.FIN_TILE_H)
    assert int(re.search(r'kTssMajority = (\d+)', src).group(1)) == ref.MAJORITY
