"""CPU-only: the numpy restatement of the flat-field kernels and functions (tests/flat_ref.py)
equals the reference's own outputs in tests/golden/flat.npz, and everything the GPU path refuses is
refused before a device is touched.  The GPU tests (test_gpu_flat.py) compare the kernels with the
restatement and the functions with the fixture.

Scene (a) - flatFieldFromCloseDistance on colour frames - has nothing fitted in it and is equal bit
for bit.  Scene (b) - flatFieldFromCloseDistance2 - is restated with the noise level function the
reference fitted (the fixture holds its three parameters) and compared on the pixels none of whose
decisions lies within 1e-5 of a threshold; the sort order is the reference's.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy.ndimage import median_filter

from .conftest import GOLDEN, load_golden
from . import dark_ref
from . import flat_cases as fc
from . import flat_ref as ref
from .test_cpu_dark import same

SUB = 2   # gen_flat_golden.SUB


@pytest.fixture(scope='module')
def g():
    return load_golden('flat.npz')


def test_scene_a_equals_the_reference_bit_for_bit(g):
    for dtype in fc.ALL_DTYPES:
        frames, bgs = fc.colour_scene(dtype)
        p = 'a_%s_' % np.dtype(dtype).name
        assert same(g[p + 'in_sum'], np.array([np.asarray(f, np.float64).sum() for f in frames + bgs])), \
            'the scene drifted from the fixture'
        assert same(ref.flat_field_1(frames, bgs), g[p + 'ff']), dtype
        assert same(ref.flat_field_1(frames, 9.5), g[p + 'ff_scalar_bg']), dtype
        # what the scene is: a field scaled by the median of a 3 x 4 grid of samples - its peak lies
        # between the samples, so the maximum is somewhat above 1
        assert 1.0 <= g[p + 'ff'].max() < 1.3 and g[p + 'ff'].min() > 0.3


def test_luma_is_numpys_weighted_average():
    rng = np.random.default_rng(1)
    img = rng.uniform(-5, 3000, (33, 130, 3))
    img[0, 1, 2], img[2, 3, 0] = np.nan, np.inf
    assert same(ref.luma(img), np.average(img, axis=-1, weights=ref.LUMA_WEIGHTS))


def test_strided_median_max_is_scipys():
    rng = np.random.default_rng(2)
    for shape, step in (((1, 1), 10), ((3, 67), 10), ((33, 130), 10), ((41, 2570), 10), ((5, 7), 1)):
        a = rng.uniform(0, 1000, shape)
        assert ref.strided_median_max(a, step) == median_filter(a[::step, ::step], 3).max(), (shape, step)


def test_sort_key_wraps_for_unsigned_frames():
    a = np.full((20, 30), 7, np.uint16)
    b = np.full((20, 30), 0, np.uint16)
    assert ref.sort_key(a) == 65529 and ref.sort_key(a).dtype == np.uint16
    assert ref.sort_key(b) == 0                       # a frame with a zero sorts first
    assert ref.sort_key(a.astype(np.float32)) == -7.0
    assert ref.sort_key(a.astype(np.uint8)) == 249


def test_scene_b_equals_the_reference_on_the_stable_pixels(g):
    frames, bgs = fc.vignetting_scene()
    assert same(g['b_in_sum'], np.array([np.asarray(f, np.float64).sum() for f in frames + bgs]))
    assert float(g['unstable_worst']) <= 0.01
    stable = g['b_stable']
    assert stable.mean() >= 0.99
    seen = []

    def listen(frame, avg, thr, lower):
        seen.append((avg, thr))
    ff, order = ref.flat_field_2(frames, bgs, dark_ref.NLF_BOUNDED_SQRT, tuple(g['b_nlf']), fc.B_NSTD, listen)
    assert list(order) == list(g['b_order']) and order != sorted(order)
    assert len(seen) == len(frames) - 1
    assert same(seen[0][1][::SUB, ::SUB], g['b_thr'])
    got = ff[::SUB, ::SUB]
    assert same(got[stable], g['b_ff'][stable])
    # the divisor is pinned: every pixel of its grid is stable
    assert stable[::10 // SUB, ::10 // SUB].all() and ref.strided_median_max(ff) == 1.0
    # what the scene is for
    for _, pts in fc.B_HITS:
        for pt in pts:
            assert ff[pt] < 1.05
    # the dark block (60 % in one frame of six) did not reach the average: the plain mean has it
    plain = ref.stack_mean(frames) - ref.stack_mean(bgs)
    plain /= ref.strided_median_max(plain)
    inside = np.zeros(ff.shape, dtype=bool)
    inside[fc.B_DARK[1]] = True
    assert (ff[inside] > 1.04 * plain[inside]).all()
    for _, pts in fc.B_HITS:            # (the plain mean has the hits too)
        for pt in pts:
            inside[pt] = True
    assert np.abs(ff[~inside] / plain[~inside] - 1).max() < 0.02


def test_refusals_need_no_device():
    from imgprocessor_amd.camera import flatField as FF
    from imgprocessor_amd.transform.imgAverage import imgAverage
    from imgprocessor_amd.utils.getBackground import getBackground
    from imgprocessor_amd.utils.getBackground2 import getBackground2
    from imgprocessor_amd import ops
    assert {'flatFieldFromCloseDistance', 'flatFieldFromCloseDistance2', 'sensitivity'} <= set(dir(FF))
    grey = [np.zeros((20, 30), np.uint16)] * 3
    colour = [np.zeros((20, 30, 3), np.uint16)] * 3
    # a number is returned as it is, None is refused
    assert getBackground2(3) == 3 and getBackground2(2.5) == 2.5
    with pytest.raises(NotImplementedError):
        getBackground2(None)
    assert getBackground(None) == 0
    assert getBackground(grey[:1]) is grey[0] and getBackground(grey[0]) is grey[0]
    with pytest.raises(NotImplementedError):
        FF.flatFieldFromCloseDistance(colour)
    with pytest.raises(NotImplementedError):
        FF.flatFieldFromCloseDistance2(grey)
    with pytest.raises(NotImplementedError):
        FF.flatFieldFromCloseDistance2(grey, 0.0, calcStd=True)
    with pytest.raises(ValueError):
        FF.flatFieldFromCloseDistance2(grey[:1], 0.0)
    with pytest.raises(ValueError):
        FF.flatFieldFromCloseDistance2([np.zeros((9, 30), np.uint16)] * 2, 0.0)    # slice step 0
    with pytest.raises(ValueError):
        FF.flatFieldFromCloseDistance2([np.zeros((20, 9), np.uint16)] * 2, 0.0)
    with pytest.raises(ValueError):
        FF.flatFieldFromCloseDistance2(colour, 0.0)
    with pytest.raises(ValueError):
        FF.flatFieldFromCloseDistance2(grey, [np.zeros((5, 5))])                   # background shape
    with pytest.raises(TypeError):
        FF.flatFieldFromCloseDistance2(['a.tif', 'b.tif'], 0.0)
    with pytest.raises(TypeError):
        FF.flatFieldFromCloseDistance(['a.tif'], 0.0)
    with pytest.raises(ValueError):
        FF.flatFieldFromCloseDistance([], 0.0)
    with pytest.raises(ValueError):
        FF.flatFieldFromCloseDistance([np.zeros((4, 5, 2))], 0.0)
    with pytest.raises(TypeError):
        imgAverage(['a.tif'])
    with pytest.raises(ValueError):
        imgAverage([])
    with pytest.raises(ValueError):
        FF.sensitivity([np.zeros((4, 30))])                                        # round(4 / 10) == 0
    with pytest.raises(ValueError):
        FF.sensitivity([])
    with pytest.raises(NotImplementedError):
        FF.sensitivity(grey, f=0.5)                                                # enlarging
    for bad in (np.zeros((5, 5)), [np.zeros((5, 5))] * 2, np.zeros((3, 5, 5))):
        with pytest.raises(ValueError):
            FF.sensitivity(grey, bad)                                              # background shape
    with pytest.raises(ValueError):
        ops.sens_shrink(np.zeros((4, 30)), f=10)
    with pytest.raises(TypeError):
        ops.nlf_lower_mask(grey[0], np.zeros((20, 30)), lambda x: x)
    with pytest.raises(ValueError):
        ops.strided_min(grey[0], 0, 1)
    with pytest.raises(ValueError):
        ops.luma(np.zeros((4, 5)))
    with pytest.raises(ValueError):
        ops.stack_mean(np.zeros((0, 4, 5)))


def test_flat_abi_declared():
    from imgprocessor_amd import _lib, ops
    names = ('ipa_stack_mean_dev', 'ipa_luma_dev', 'ipa_strided_extremum_dev', 'ipa_flat_scale_dev',
             'ipa_nlf_lower_mask_dev', 'ipa_sens_shrink_dev', 'ipa_sens_accumulate_dev')
    lib = _lib.lib()
    for n in names:
        assert n in _lib.PROTOTYPES and hasattr(lib, n)
    assert (_lib.EXTREMUM_MEDIAN_MAX, _lib.EXTREMUM_MIN) == (0, 1)
    # a NULL context is refused before anything is looked at
    assert lib.ipa_stack_mean_dev(None, None, 0, 1, 1, 1, 1, 1, None, 1) == _lib.ERR_BAD_ARG
    assert lib.ipa_sens_shrink_dev(None, None, 0, 1, 1, 1, None, 0, 0.0, 1, 1, None, 1) == _lib.ERR_BAD_ARG
    for n in ('stack_mean', 'luma', 'strided_median_max', 'strided_min', 'flat_scale', 'nlf_lower_mask',
              'sens_shrink', 'sens_accumulate'):
        assert callable(getattr(ops, n))


def test_generator_reproduces_the_fixture(tmp_path):
    """where the reference exists: every array of the committed fixture, byte for byte"""
    sys.path.insert(0, GOLDEN)
    try:
        from gen_golden import REF
    finally:
        sys.path.remove(GOLDEN)
    if not os.path.isdir(os.path.join(REF, 'imgProcessor')):
        pytest.skip('the reference source is not on this machine')
    out = str(tmp_path / 'flat.npz')
    subprocess.check_call([sys.executable, os.path.join(GOLDEN, 'gen_flat_golden.py'), out],
                          stdout=subprocess.DEVNULL)
    new, old = dict(np.load(out)), load_golden('flat.npz')
    assert sorted(new) == sorted(old)
    for k in old:
        assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape, k
        assert new[k].tobytes() == old[k].tobytes(), k
