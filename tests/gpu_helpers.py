"""helpers of the GPU tests: synthetic frame batches, map pairs, kernels, bit comparison"""
import numpy as np

from .conftest import synth


def frames(n, h, w, dtype=np.float32):
    out = np.stack([synth((h, w), 100 + i) for i in range(n)])
    if dtype == np.uint16:
        return np.round(out * 4095).astype(np.uint16)
    return out.astype(dtype)


def radial_maps(h, w, k1=-0.12, shift=0.0):
    K = np.array([[float(w), 0, (w - 1) / 2.0], [0, float(w), (h - 1) / 2.0], [0, 0, 1.0]])
    dist = np.array([k1, 0.03, 1e-3, -5e-4, 0.0])
    from imgprocessor_amd import ops
    mx, my = ops.build_undistort_map(K, dist, K, h, w)
    return (mx + np.float32(shift)).astype(np.float32), my.astype(np.float32), K, dist


def rot_maps(h, w, deg):
    a = np.deg2rad(deg)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    mx = np.cos(a) * (x - cx) - np.sin(a) * (y - cy) + cx
    my = np.sin(a) * (x - cx) + np.cos(a) * (y - cy) + cy
    return mx.astype(np.float32), my.astype(np.float32)


_hint_serial = [0]


def fresh_ring_hint(ctx):
    """ring_plan_prepare keeps ONE hint (clean strip pairs of the last key) and skips the ring 15 calls of
    16 on it, also at ring_remap = 2.  A ring call with a key no other call has - its own matrix - takes
    the slot, so that the call after it plans and launches whatever ran before."""
    from imgprocessor_amd import ops
    old = ctx.set_tuning(ring_remap=2, ring_min=1, tile_warp=0)
    try:
        _hint_serial[0] += 1
        M = np.array([[1.0, 0, 2.0 + _hint_serial[0] / 64.0], [0, 1.0, 2.0], [0, 0, 1.0]])
        ops.warp_perspective(ctx.to_device(np.zeros((1, 40, 140), np.float32)), M, (32, 128), 'cubic')
    finally:
        ctx.set_tuning(**old)


def remap_path(ctx):
    """the kernels the last plain remap call launched (IPA_REMAP_PATH_* bits)"""
    return ctx.get_tuning('remap_path')


def path_names(mask):
    from imgprocessor_amd import _lib
    names = [n[len('REMAP_PATH_'):] for n in dir(_lib) if n.startswith('REMAP_PATH_')]
    return '|'.join(sorted((n for n in names if mask & getattr(_lib, 'REMAP_PATH_' + n)),
                           key=lambda n: getattr(_lib, 'REMAP_PATH_' + n))) or '0'


def only_gather(mask):
    """no alternative kernel ran: the gather kernel, with the frame index fastest or not"""
    from imgprocessor_amd import _lib
    return mask in (_lib.REMAP_PATH_GATHER, _lib.REMAP_PATH_GATHER | _lib.REMAP_PATH_FRAMES_INNER)


def kern(K, seed=5):
    k = np.random.default_rng(seed).random((K, K))
    return k / k.sum()


def same_bits(a, b, what):
    assert a.shape == b.shape
    bad = a.view(np.uint32) != b.view(np.uint32)
    bad &= ~(np.isnan(a) & np.isnan(b))
    assert not bad.any(), '%s: %d of %d values differ, first at %s (%r vs %r)' % (
        what, bad.sum(), a.size, np.argwhere(bad)[0], a[bad][0], b[bad][0])
