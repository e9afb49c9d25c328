"""GPU: the single-image ops that Python stages (ops._stage_in / ops._stage_out: a numpy input goes up with
Context.to_device, the `_dev` export runs, the result comes back with DeviceArray.get) give byte for byte what
they give for the same data as a DeviceArray.  tests/test_gpu_host_staging.py does the same for the exports the
C side stages.

Shapes: one 37 x 53 float32 image with one NaN (odd, more than one block, no multiple of a tile), 3 x 37 x 53
for nl_means and nan_to_zero; masks about 20 % set."""
import numpy as np
import pytest

from .gpu_helpers import frames
from .test_gpu_host_staging import same_bytes

pytestmark = pytest.mark.gpu

N, H, W = 3, 37, 53


@pytest.fixture(scope='module')
def ia():
    import imgprocessor_amd
    imgprocessor_amd.default_context(0)  # raises without a gfx950 device: no fallback
    return imgprocessor_amd


@pytest.fixture(scope='module')
def data():
    """read-only: every test copies what an op writes in place"""
    batch = frames(N, H, W)
    batch[1, 30, 7] = np.nan
    img = np.ascontiguousarray(batch[1])
    mask = (np.random.default_rng(3).random((H, W)) < 0.2).astype(np.uint8)
    for a in (batch, img, mask):
        a.setflags(write=False)
    return batch, img, mask


def both(ia, run, *arrays):
    """run(*arrays) on the numpy arrays and on their device copies"""
    ctx = ia.default_context(0)
    return run(*arrays), run(*[ctx.to_device(a) for a in arrays])


@pytest.mark.parametrize('kxy', [(3, 5), (5, 3)])
def test_extend_array(ia, data, kxy):
    host, dev = both(ia, lambda a: ia.ops.extend_array(a, kxy, 'wrap', 'reflect'), data[1])
    assert host.shape == (H + 2 * (kxy[1] // 2), W + 2 * (kxy[0] // 2))
    same_bytes(host, dev, 'extend_array')


def test_conv_ydep(ia, data):
    k = np.random.default_rng(5).random((H, 3, 5))
    same_bytes(*both(ia, lambda a: ia.ops.conv_ydep(a, k), data[1]), 'conv_ydep')


def test_var_y_gauss(ia, data):
    rowk = ia.ops.gaussian_kernel1d(0.8, radius=2)
    same_bytes(*both(ia, lambda a: ia.ops.var_y_gauss(a, 0.5, 2.0, 5, rowk), data[1]), 'var_y_gauss')


@pytest.mark.parametrize('ksize', [(3, 3), (5, 3)])
def test_local_std(ia, data, ksize):
    blurred = ia.ops.gaussian_filter(np.nan_to_num(data[1]), 1.0)
    same_bytes(*both(ia, lambda a, b: ia.ops.local_std(a, b, ksize), data[1], blurred), 'local_std %s' % (ksize,))


@pytest.mark.parametrize('fn', ['mean', 'median'])
@pytest.mark.parametrize('fill_mask', [True, False])
def test_masked_mean(ia, data, fn, fill_mask):
    ctx = ia.default_context(0)
    h_arr, d_arr = data[1].copy(), ctx.to_device(data[1])
    host = ia.ops.masked_mean(h_arr, data[2], 5, fill_mask, fn=fn)
    dev = ia.ops.masked_mean(d_arr, ctx.to_device(data[2]), 5, fill_mask, fn=fn)
    same_bytes(host, dev, 'masked_mean %s' % fn)
    if fill_mask:   # in place: the arrays that went in are the result
        assert host is h_arr and dev is d_arr
        same_bytes(h_arr, d_arr, 'masked_mean %s, the array filled in place' % fn)
        assert h_arr.tobytes() != data[1].tobytes()
    else:
        assert h_arr.tobytes() == data[1].tobytes() and d_arr.get().tobytes() == data[1].tobytes()


@pytest.mark.parametrize('ksize', [3, 5])
def test_nan_max(ia, data, ksize):
    same_bytes(*both(ia, lambda a: ia.ops.nan_max(a, ksize), data[1]), 'nan_max %d' % ksize)


@pytest.mark.parametrize('dtype', [np.uint16, np.float64])
def test_closest_distance(ia, data, dtype):
    host, dev = both(ia, lambda a: ia.ops.closest_distance(a, 5, dtype), data[2])
    assert host.dtype == dtype
    same_bytes(host, dev, 'closest_distance %s' % np.dtype(dtype))


def test_pos_intensity_unc(ia, data):
    same_bytes(*both(ia, lambda a: ia.ops.pos_intensity_unc(a, 0.7, 1.1, 3), data[1]), 'pos_intensity_unc, scalars')
    rng = np.random.default_rng(6)
    sx, sy = 0.5 + rng.random((H, W)), 0.5 + rng.random((H, W))
    same_bytes(*both(ia, lambda a, x, y: ia.ops.pos_intensity_unc(a, x, y, 3), data[1], sx, sy),
               'pos_intensity_unc, maps')


@pytest.mark.parametrize('size', [3, 5])
def test_median_threshold(ia, data, size):
    (h_out, h_idx), (d_out, d_idx) = both(ia, lambda a: ia.ops.median_threshold(a, 0.05, size=size), data[1])
    same_bytes(h_out, d_out, 'median_threshold %d' % size)
    assert h_idx.dtype == bool and h_idx.any()
    same_bytes(h_idx.astype(np.uint8), d_idx, 'median_threshold %d, indices' % size)


def test_calib_prefilter(ia, data):
    bg, ff = data[1] * np.float32(0.1), np.float32(0.5) + np.nan_to_num(data[1])
    same_bytes(*both(ia, lambda a, b, f: ia.ops.calib_prefilter(a, b, f, 0.05), data[1], bg, ff), 'calib_prefilter')
    same_bytes(*both(ia, lambda a: ia.ops.calib_prefilter(a), data[1]), 'calib_prefilter, threshold only')


def test_remove_single_pixels(ia, data):
    host, dev = both(ia, ia.ops.remove_single_pixels, data[2])
    assert host.dtype == bool and 0 < host.sum() < data[2].sum()
    same_bytes(host.astype(np.uint8), dev, 'remove_single_pixels')


def test_nl_means(ia, data):
    run = lambda a: ia.ops.nl_means(a, patch_size=5, patch_distance=3)
    same_bytes(*both(ia, run, data[0]), 'nl_means, batch')
    same_bytes(*both(ia, run, data[1]), 'nl_means, one image')


def test_nan_to_zero(ia, data):
    """device arrays only: the result against numpy, the refusal of a host array"""
    ctx = ia.default_context(0)
    d = ctx.to_device(data[0])
    assert ia.ops.nan_to_zero(d) is d
    want = data[0].copy()
    want[np.isnan(want)] = 0
    same_bytes(want, d, 'nan_to_zero')
    with pytest.raises(TypeError):
        ia.ops.nan_to_zero(data[0].copy())
