"""CPU-only: the numpy restatement of single-time-effect removal (features/
SingleTimeEffectDetection.py:13-75 with a given noise level function) equals the reference's own
outputs in tests/golden/ste.npz bit for bit, and the parts that are not on the GPU path refuse
before any device is touched.  The GPU tests (test_gpu_ste.py) compare the kernel with both.
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
