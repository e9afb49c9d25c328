"""CPU-only: the flat field from spot images (csrc/spot.hip, ops_spot.py,
camera/flatField/vignettingFromSpotAverage.py) without a device.

  * the binding: the seven symbols exist and a NULL context is refused before anything is read (the
    prototypes are compared with the header by tests/test_cpu_host.py);
  * the ops and the routine refuse bad arguments before they touch a device;
  * the numpy restatement (tests/spot_ref.py) against its yardsticks: the histogram rule against
    np.histogram (values exactly on bin edges included), the erosion against scipy's
    minimum_filter, the labelling against scipy.ndimage.label and the stored skimage / scipy labels,
    and the whole routine against the fixture the unchanged reference wrote
    (tests/golden/spot.npz): thresholds, counts, label images, sizes, mx, fitimg and mask bit for bit.
"""
import contextlib
import io

import numpy as np
import pytest
from scipy import ndimage

from . import spot_cases as sc
from . import spot_ref as ref
from .conftest import load_golden
from .test_cpu_dark import same

SCENES = sc.scenes()
EIGHT = np.ones((3, 3), int)


@pytest.fixture(scope='module')
def g():
    return load_golden('spot.npz')


def V():
    from imgprocessor_amd.camera.flatField import vignettingFromSpotAverage
    return vignettingFromSpotAverage


# ------------------------------------------------------------------ binding
def test_binding_and_exports():
    from imgprocessor_amd import _lib, ops, ops_spot
    lib = _lib.lib()
    names = ('ipa_spot_range_dev', 'ipa_spot_histogram_dev', 'ipa_spot_mask_dev', 'ipa_label_dev',
             'ipa_label_sizes_dev', 'ipa_label_largest_dev', 'ipa_spot_take_dev')
    for n in names:
        assert n in _lib.PROTOTYPES and hasattr(lib, n)
    for n in ('histogram', 'otsu_threshold', 'spot_mask', 'label', 'largest_component', 'spot_take'):
        assert getattr(ops, n) is getattr(ops_spot, n)
    # a NULL context is refused before anything is looked at
    assert lib.ipa_spot_range_dev(None, None, 0, 1, 1, 1, None, 1, 0.0, None) == _lib.ERR_BAD_ARG
    assert lib.ipa_spot_histogram_dev(None, None, 0, 1, 1, 1, None, 1, 0.0, None, 1, None) == _lib.ERR_BAD_ARG
    assert lib.ipa_spot_mask_dev(None, None, 0, 1, 1, 1, None, 1, 0.0, 0.0, None, 1) == _lib.ERR_BAD_ARG
    assert lib.ipa_label_dev(None, None, 1, 1, 1, 2, None, 1, None) == _lib.ERR_BAD_ARG
    assert lib.ipa_label_sizes_dev(None, None, 1, 1, 1, 1, None) == _lib.ERR_BAD_ARG
    assert lib.ipa_label_largest_dev(None, None, 1, 1, 1, 1, None) == _lib.ERR_BAD_ARG
    assert lib.ipa_spot_take_dev(None, None, 0, 1, 1, 1, None, 1, 0.0, None, 1, 1, 0, 0, None, 1, None, 1,
                                 None) == _lib.ERR_BAD_ARG


def test_the_family_imports_no_layer_built_on_it():
    import subprocess
    import sys
    code = ('import sys, imgprocessor_amd.ops_spot\n'
            'up = [m for m in ("features", "camera", "uncertainty") if "imgprocessor_amd." + m in sys.modules]\n'
            'assert not up, up')
    subprocess.check_call([sys.executable, '-c', code])


def test_ops_refuse_before_a_device():
    from imgprocessor_amd import ops
    img = np.zeros((4, 5), np.float32)
    for nbins in (0, -3, 2.5):
        with pytest.raises(ValueError):
            ops.histogram(img, nbins)
        with pytest.raises(ValueError):
            ops.otsu_threshold(img, nbins=nbins)
    with pytest.raises(NotImplementedError):
        ops.histogram(img, 2049)
    with pytest.raises(NotImplementedError):
        ops.otsu_threshold(img, nbins=4096)
    for conn in (0, 3, None):
        with pytest.raises(ValueError):
            ops.label(img > 0, conn)
    with pytest.raises(ValueError):
        ops.largest_component(np.zeros((4, 5), np.int32))          # labels without their count
    with pytest.raises(ValueError):
        ops.largest_component(img > 0, connectivity=4)
    with pytest.raises(ValueError):
        ops.spot_take(img)                                          # neither labels nor rows
    with pytest.raises(ValueError):
        ops.spot_take(img, np.zeros((4, 5), np.int32), 1, rows=(0, 1))


def test_the_routine_refuses_before_a_device():
    f = V()
    frames = [np.zeros((6, 8), np.uint16)] * 2
    with pytest.raises(NotImplementedError):
        f(frames)                                                   # bgImages=None: getBackground2
    with pytest.raises(TypeError):
        f('spots.tif', 0)
    with pytest.raises(TypeError):
        f(['a.tif', 'b.tif'], 0)
    with pytest.raises(TypeError):
        f([np.zeros((6, 8, 3))], 0)                                 # colour frames
    with pytest.raises(ValueError):
        f([], 0)
    with pytest.raises(ValueError):
        f(np.zeros((6, 8)), 0)                                      # one frame is no stack
    with pytest.raises(ValueError):
        f(frames, [np.zeros((6, 9))])                               # background of another shape
    with pytest.raises(TypeError):
        f(frames, ['bg.tif'])
    with pytest.raises((TypeError, ValueError)):
        f(frames, 0, thresh='high')


# ------------------------------------------------------------------ the restatement: histogram, Otsu
def edge_data():
    """values exactly on bin edges, and not"""
    rng = np.random.default_rng(9)
    out = [rng.integers(0, top + 1, 3000).astype(np.float64) for top in (7, 100, 255)]
    for a, top in zip(out, (7, 100, 255)):
        a[:2] = 0, top
    out.append(rng.random(3000) * 1e-3 - 17.0)
    out.append(rng.standard_normal(3000).astype(np.float32).astype(np.float64))
    out.append(np.array([4.25]))
    out.append(np.full(77, -3.0))
    return out


@pytest.mark.parametrize('nbins', (1, 2, 7, 256, 2048))
def test_histogram_rule_is_numpys(nbins):
    for x in edge_data():
        counts, edges = ref.histogram(x, nbins)
        want, want_edges = np.histogram(x, nbins)
        assert same(edges, want_edges)
        assert np.array_equal(counts, want) and counts.sum() == x.size and counts.dtype == np.int64
    with pytest.raises(ValueError):
        ref.histogram(np.array([1.0, np.nan]), nbins)
    with pytest.raises(ValueError):
        ref.histogram(np.array([1.0, np.inf]), nbins)


def test_otsu_early_return_and_fixture(g):
    assert ref.otsu(np.full((3, 4), 2.5)) == 2.5
    z = np.zeros((2, 2))
    z[0, 0] = -0.0
    assert np.signbit(ref.otsu(z))            # the first pixel itself
    for name, scene in SCENES.items():
        if scene['thresh'] is not None:
            continue
        bg = ref.background(scene['bg'])
        for k, im in enumerate(scene['images']):
            x = ref.frame(im, bg)
            assert ref.otsu(x) == g[name + '_t'][k], (name, k)
            assert np.array_equal(ref.histogram(x)[0], g[name + '_counts'][k]), (name, k)


# ------------------------------------------------------------------ erosion, labelling
def test_erosion_is_scipys():
    rng = np.random.default_rng(4)
    for shape in ((1, 1), (1, 9), (7, 1), (2, 2), (3, 3), (17, 23)):
        for d in (0.5, 0.9, 1.0):
            b = rng.random(shape) < d
            assert np.array_equal(ref.erode(b), ndimage.minimum_filter(b, 3))
    x = np.array([[1.0, 2.0, np.nan], [2.0, 2.0, 2.0], [3.0, 2.5, 2.0]])
    assert ref.spot_mask(x, 2.0).sum() == 0 and ref.spot_mask(x, 0.5).dtype == np.uint8


@pytest.mark.parametrize('conn', (1, 2))
def test_labelling_is_skimages_and_scipys(g, conn):
    for name, m in sc.golden_patterns().items():
        labels, n = ref.label(m, conn)
        assert n == int(g['label_%s_c%d_n' % (name, conn)]), name
        assert labels.dtype == np.int32 and np.array_equal(labels, g['label_%s_c%d' % (name, conn)]), name
        assert np.array_equal(ref.sizes(labels, n), np.bincount(labels.ravel(), minlength=n + 1)[1:])
    for shape in ((1, 1), (5, 1), (1, 7), (30, 50)):
        for d in (0.3, 0.5, 0.62, 0.9):
            m = sc.random_field(shape, d, int(100 * d) + shape[1])
            want, n_want = ndimage.label(m, EIGHT if conn == 2 else None)
            labels, n = ref.label(m, conn)
            assert n == n_want and np.array_equal(labels, want)
    s = (2 * sc.TILE_H + 1, 2 * sc.TILE_W + 2)
    assert ref.label(sc.checkerboard(s), 2)[1] == 1 and ref.label(sc.checkerboard(s), 1)[1] == (s[0] * s[1] + 1) // 2
    assert ref.label(sc.spiral(s), 1)[1] == 1 and ref.label(sc.u_shape(s), 1)[1] == 1


def test_largest_takes_the_lower_label_on_a_tie():
    m = np.zeros((9, 12), np.uint8)
    m[0:2, 8:11] = 1      # 6 pixels, first in raster order
    m[4:7, 1:3] = 1       # 6 pixels
    m[8, 5:10] = 1        # 5 pixels
    labels, n = ref.label(m)
    assert n == 3 and ref.largest(labels, n) == (1, 6, (3, 54))
    assert ref.largest(np.zeros((3, 3), np.int32), 0) is None


# ------------------------------------------------------------------ the routine
@pytest.mark.parametrize('name', sorted(SCENES))
def test_routine_restatement_equals_the_fixture(g, name):
    scene = SCENES[name]
    frames = scene['images'] + ([] if np.ndim(scene['bg']) == 0 else scene['bg'])
    assert np.array_equal([np.asarray(f, np.float64).sum() for f in frames], g[name + '_in_sum']), \
        'the scene is not the one the fixture was generated from'
    if scene['raises'] is not None:
        with pytest.raises(scene['raises']):
            ref.spot_average(scene['images'], scene['bg'], scene['averageSpot'], scene['thresh'])
        assert name + '_fitimg' not in g and int(g[name + '_label'][-1]) < 0
        return
    fitimg, mask, info = ref.spot_average(scene['images'], scene['bg'], scene['averageSpot'], scene['thresh'])
    assert np.array_equal(info['t'], g[name + '_t'])
    assert np.array_equal(info['n'], g[name + '_n']) and np.array_equal(info['label'], g[name + '_label'])
    for k, s in enumerate(info['sizes']):
        assert np.array_equal(s, g[name + '_sizes'][k][:len(s)]) and not g[name + '_sizes'][k][len(s):].any()
    assert same(np.array(info['mx2']), g[name + '_mx2']) and float(info['mx']) == float(g[name + '_mx'])
    assert same(fitimg, g[name + '_fitimg']) and same(mask, g[name + '_mask'])
    bg = ref.background(scene['bg'])
    for k, im in enumerate(scene['images']):
        spots, n = ref.label(ref.spot_mask(ref.frame(im, bg), info['t'][k]))
        assert np.array_equal(spots, g[name + '_spots'][k]), (name, k)


def test_fixture_holds_every_kind_of_scene(g):
    kinds = set()
    for name, scene in SCENES.items():
        kinds.add(('rows' if scene['averageSpot'] else 'spot', scene['raises'] is not None))
        kinds.add('thresh' if scene['thresh'] is not None else 'otsu')
        kinds.add('scalar' if np.ndim(scene['bg']) == 0 else 'frames')
        if (g[name + '_label'] == 0).any():
            kinds.add('no spot')
            assert "couldn't find spot in image" in str(g[name + '_printed'])
    assert kinds == {('rows', False), ('rows', True), ('spot', False), 'thresh', 'otsu', 'scalar', 'frames',
                     'no spot'}
    # the planted tie of scene (a), frame 2: two components of 49 pixels, the first chosen
    assert g['a_u16_bgframes_otsu_spot_sizes'][2][:2].tolist() == [49, 49]
    assert int(g['a_u16_bgframes_otsu_spot_label'][2]) == 1
    # no spot anywhere: mx stays 0 and the division gives NaN without raising
    assert float(g['e_u8_no_spot_mx']) == 0.0 and np.isnan(g['e_u8_no_spot_fitimg']).all()
    # in the spot scenes the two largest spot means are apart: a last digit cannot change mx
    for name, scene in SCENES.items():
        v = g[name + '_mx2'][np.isfinite(g[name + '_mx2'])]
        if not scene['averageSpot'] and v.size >= 2:
            top = np.sort(v)[-2:]
            assert top[1] - top[0] > 1e-9 * top[1]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        ref.spot_average(SCENES['e_u8_no_spot']['images'], 1.0, False, None)
