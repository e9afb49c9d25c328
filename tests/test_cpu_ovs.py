"""CPU-only: object / vignetting separation (csrc/ovs.hip,
camera/flatField/vignettingFromRandomSteps.py) without a device.

  * the binding: the three symbols exist and a NULL context is refused before anything is read (the
    prototypes are compared with the header by tests/test_cpu_host.py);
  * the class validates its input before it touches a device;
  * the stop rule on made-up residuum sequences, every branch;
  * the numpy restatement (tests/ovs_ref.py) with the oracle's warp: one step through the restated
    kernels equals the step written with explicit per-image warps, bit for bit; on the loop scene
    both steps accept some pixels and reject others, nothing non-finite arises, the residuum falls
    and an early stop between the 3rd and 4th residuum ends the loop before maxIter.

The loop is NOT tested for recovering the true vignetting: the reference's loop does not get there
on such scenes, and that is its property, not this project's.
"""
import numpy as np
import pytest

from . import ovs_cases as oc
from . import ovs_ref as ref
from .test_cpu_dark import same


@pytest.fixture(scope='module')
def warp(oracle):
    def w(src, M, shape):
        return oracle.warp_perspective(np.ascontiguousarray(src, dtype=np.float64), M, tuple(shape),
                                       oracle.LINEAR | oracle.Q5, oracle.CONSTANT, 0.0)
    return w


def V():
    from imgprocessor_amd.camera.flatField import vignettingFromRandomSteps
    return vignettingFromRandomSteps


# ------------------------------------------------------------------ binding
def test_binding_and_exports():
    from imgprocessor_amd import _lib, ops, ops_ovs
    lib = _lib.lib()
    for n in ('ipa_ovs_object_dev', 'ipa_ovs_flatfield_dev', 'ipa_masked_running_mean_dev'):
        assert n in _lib.PROTOTYPES and hasattr(lib, n)
    assert ops.ovs_object is ops_ovs.ovs_object and ops.ovs_flatfield is ops_ovs.ovs_flatfield
    assert ops.masked_running_mean_update is ops_ovs.masked_running_mean_update
    assert (oc.MAX_FRAMES, V().MAX_FITS) == (ops_ovs.MAX_FRAMES, 64)
    assert lib.ipa_version() == 100
    # a NULL context is refused before anything is looked at
    assert lib.ipa_ovs_object_dev(None, None, 1, 1, 1, None, 0, 1, 1, 1, 1, 1, None, None, 1, None, 1) \
        == _lib.ERR_BAD_ARG
    assert lib.ipa_ovs_flatfield_dev(None, None, 1, None, 0, 1, 1, 1, 1, 1, None, 1, 1, None, None, 1, 1, 1, None,
                                     1, 0, None, 1, 1) == _lib.ERR_BAD_ARG
    assert lib.ipa_masked_running_mean_dev(None, None, 1, None, 1, None, 0, 1, None, 1, 1, 1) == _lib.ERR_BAD_ARG


def test_ops_refuse_without_a_device():
    from imgprocessor_amd import ops
    ff, z = np.ones((5, 6)), np.zeros((0, 3, 4), np.float32)
    with pytest.raises(ValueError):
        ops.ovs_object(ff, z, np.zeros((0, 3, 3)))
    with pytest.raises(NotImplementedError):
        ops.ovs_object(ff, np.zeros((65, 3, 4), np.float32), np.zeros((65, 3, 3)))
    with pytest.raises(ValueError):
        ops.ovs_object(ff, np.zeros((2, 3, 4), np.float32), np.zeros((3, 3, 3)))
    with pytest.raises(ValueError):
        ops.ovs_flatfield(np.ones((3, 4)), np.zeros((2, 3, 4), np.float32), np.zeros((2, 3, 4), bool),
                          np.zeros((2, 2, 3)), (5, 6))
    with pytest.raises(NotImplementedError):
        ops.ovs_flatfield(np.ones((3, 4)), np.zeros((65, 3, 4), np.float32), np.zeros((65, 3, 4), bool),
                          np.zeros((65, 3, 3)), (5, 6))


# ------------------------------------------------------------------ the class, before a device
def test_the_class_validates_before_touching_a_device():
    m = V()
    s = m.ObjectVignettingSeparation((60, 80), (30, 40))
    fit, mask, img = np.ones((30, 40), np.float32), np.zeros((30, 40), bool), np.ones((60, 80), np.float32)
    H = np.eye(3)
    for bad in (dict(fit=fit[:-1]), dict(mask=mask[:, :-1]), dict(img=img[:-1]), dict(img_mask=img[:, 1:] > 0),
                dict(H=np.eye(4)), dict(H=np.ones((2, 3))), dict(H_inv=np.eye(2))):
        kw = dict(fit=fit, mask=mask, H=H, img=img)
        kw.update(bad)
        with pytest.raises(ValueError):
            s.addFit(**kw)
    with pytest.raises(ValueError):
        s.addFit(fit, mask, H, img_mask=img > 0)       # a mask without its image
    assert s.ctx is None and not s.fits and not s.Hs, 'a refused fit left something behind'
    with pytest.raises(ValueError):
        s.separate()                                    # no fits
    with pytest.raises(ValueError):
        iter(s)
    with pytest.raises(ValueError):
        m.ObjectVignettingSeparation((60, 80, 3), (30, 40))
    with pytest.raises(ValueError):
        s.flatField = np.ones((5, 5))
    # the 65th fit, and a loop without a flat field to start from: the lists filled by hand, so no
    # device is involved
    s.fits = [None] * 64
    with pytest.raises(NotImplementedError):
        s.addFit(fit, mask, H)
    s.fits = [None]
    with pytest.raises(ValueError):
        s.separate()
    assert s.ctx is None
    for call in (lambda: s.addImg(img), lambda: s._findObject(img), s.smooth, s.error,
                 lambda: m.vignettingFromRandomSteps([img], None)):
        with pytest.raises(NotImplementedError):
            call()
    assert s.flatField is None and s.lens is None


# ------------------------------------------------------------------ the stop rule
def test_stop_rule_branches():
    stop = V().stopIteration
    # maxIter = 0 stops on the first pass; otherwise the first pass never stops (last_dev is None)
    assert stop(0, 0.5, None, 0, 1e-4) is True
    assert stop(0, 0.0, None, 10, 1e-4) is False and stop(0, 1e-9, None, 1, 1e-4) is False
    assert stop(1, 0.5, 0.6, 1, 1e-4) is True             # n reached maxIter
    # dev < maxDev stops as soon as there is a last_dev
    assert stop(1, 5e-5, 0.2, 10, 1e-4) is True and stop(1, 2e-4, 0.2, 10, 1e-4) is False
    # a growing residuum stops only once n > 4
    for n in (1, 2, 3, 4):
        assert stop(n, 0.3, 0.2, 10, 1e-4) is False, n
    assert stop(5, 0.3, 0.2, 10, 1e-4) is True and stop(5, 0.2, 0.2, 10, 1e-4) is False
    # a last residuum of exactly 0 reads as "none" in the reference's rule
    assert stop(6, 0.3, 0.0, 10, 1e-4) is False
    # a whole made-up sequence
    seq, last, n, steps = [0.2, 0.1, 0.05, 0.06, 0.07, 0.08, 0.09], None, 0, 0
    for dev in seq:
        if stop(n, dev, last, 10, 1e-4):
            break
        n, last, steps = n + 1, dev, steps + 1
    assert steps == 5
    for n, dev, last, mi, md in ((0, 0.5, None, 0, 1e-4), (3, 0.3, 0.2, 10, 1e-4), (5, 0.3, 0.2, 10, 1e-4),
                                 (2, 5e-5, 0.2, 10, 1e-4)):
        assert stop(n, dev, last, mi, md) == ref.stop(n, dev, last, mi, md)


def test_residuum_reads_every_tenth_pixel():
    rng = np.random.default_rng(2)
    new, old = rng.random((41, 57)), rng.random((41, 57))
    new[0, 10], old[20, 30] = np.nan, np.nan
    got = V().residuum(np.ascontiguousarray(new[::10, ::10]), np.ascontiguousarray(old[::10, ::10]))
    assert got == ref.residuum(new, old) and np.isfinite(got)


# ------------------------------------------------------------------ the restatement
def test_running_mean_is_the_stand_in():
    rng = np.random.default_rng(3)
    m = ref.MaskedMovingAverage((7, 9))
    seen = np.zeros((7, 9), int)
    vals = []
    for k in range(4):
        data, mask = rng.random((7, 9)), rng.random((7, 9)) < 0.6
        mask[0, 0] = False
        m.update(data, mask)
        seen += mask
        vals.append(np.where(mask, data, np.nan))
    assert np.array_equal(m.n, seen) and m.n[0, 0] == 0 and m.avg[0, 0] == 0
    st = np.stack(vals)[:, seen > 0]
    np.testing.assert_allclose(m.avg[seen > 0], np.nanmean(st, axis=0), rtol=1e-14)
    a, n = ref.masked_running_mean(m.avg, m.n, np.full((7, 9), 2.0), None)
    assert np.array_equal(n, seen + 1) and a[0, 0] == 2.0


@pytest.mark.parametrize('dtype', (np.float64, np.uint16))
def test_one_step_equals_the_explicit_step(warp, dtype):
    sc = oc.loop_scene(dtype=dtype)
    fits, masks, Hs = list(sc['fits']), list(sc['masks']), list(sc['Hs'])
    Hinvs = [np.linalg.inv(h) for h in Hs]
    s = ref.Separation(warp, sc['ff0'], fits, masks, Hs, Hinvs, max_iter=10)
    it = iter(s)
    next(it)
    obj, new = ref.next_explicit(warp, sc['ff0'], fits, masks, Hs, Hinvs)
    assert same(s.object, obj) and same(s.flatField, np.clip(new, 0, 1))
    # the second step starts from a flat field that is 0 outside the fits: pixels of the object are
    # rejected too
    ff1 = s.flatField.copy()
    next(it)
    obj, new = ref.next_explicit(warp, ff1, fits, masks, Hs, Hinvs)
    assert same(s.object, obj) and same(s.flatField, np.clip(new, 0, 1))
    n_obj, n_ff = s.counts
    assert len(np.unique(n_obj)) >= 2 and len(np.unique(n_ff)) >= 2
    assert n_ff.min() == 0 and n_ff.max() <= len(fits) and n_obj.max() == len(fits)


@pytest.mark.parametrize('scene', (dict(), dict(ff_shape=(96, 130), obj_shape=(40, 60), n=9, seed=2)),
                         ids=('60x80', '96x130'))
def test_the_loop_scene(warp, scene):
    sc = oc.loop_scene(**scene)
    s = ref.Separation(warp, sc['ff0'], list(sc['fits']), list(sc['masks']), list(sc['Hs']))
    ff, obj = s.run()
    r = s.residua
    print('residua:', ' '.join('%.3e' % d for d in r))
    n_obj, n_ff = s.counts
    cover = (n_ff > 0).mean()
    print('flat-field coverage %.2f, counts %d..%d' % (cover, n_ff.min(), n_ff.max()))
    assert np.isfinite(ff).all() and np.isfinite(obj).all()
    assert 0.2 <= cover <= 0.7 and n_ff.min() == 0 and len(np.unique(n_ff)) >= 2 and len(np.unique(n_obj)) >= 2
    assert len(r) == 11 and s.n == 10, 'the default maxDev stops by maxIter'
    assert all(b < a for a, b in zip(r, r[1:])), 'the residuum falls'
    # an early stop: maxDev between the 3rd and the 4th residuum
    early = ref.Separation(warp, sc['ff0'], list(sc['fits']), list(sc['masks']), list(sc['Hs']),
                           max_dev=0.5 * (r[2] + r[3]))
    early.run()
    assert early.n == 3 and len(early.residua) == 4 and early.residua == r[:4]
