#!/usr/bin/env python3
"""One refinement step of the object / vignetting separation on device-resident data: one JSON line.

10 float64 fitted images on a 1200 x 2000 object grid, a 2160 x 3840 flat field.  It times, after
warm-up, the median of --reps steps of
  - the fused step: ipa_ovs_object_dev + ipa_ovs_flatfield_dev, two launches (HIP events around
    each kernel and around the pair, and a host clock around the pair that ends in a synchronise);
  - the same step composed from the wrappers of camera/flatField/vignettingFromRandomSteps.py as
    they were used before: 2 x 10 ops.warp_perspective launches on host arrays, the divisions and
    the running means in numpy (host clock);
and reports the compulsory bytes of each fused kernel - fits (+ masks) read once, flat field or
object read once, result + count written -, the rate they reach and its fraction of a
device-to-device copy's rate measured in the same process.  The two steps' results are compared
bit for bit once.

    python tools/ovs_bench.py [--reps 20] [--out profiles/ovs_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import imgprocessor_amd as ia  # noqa: E402
from imgprocessor_amd import DeviceArray, _lib as L  # noqa: E402
from imgprocessor_amd.camera.flatField.vignettingFromRandomSteps import (  # noqa: E402
    warpFlatField, warpRatioToFlatField)

N, OBJ, FF = 10, (1200, 2000), (2160, 3840)


def scene(rng, n, obj_shape, ff_shape):
    oh, ow = obj_shape
    fh, fw = ff_shape
    y, x = np.mgrid[0:fh, 0:fw].astype(np.float64)
    ff = np.clip(1.0 - 0.8 * (((y - 0.5 * fh) / fh) ** 2 + ((x - 0.5 * fw) / fw) ** 2), 0, 1)
    del x, y
    fits = 0.2 + 0.8 * rng.random((n, oh, ow))
    masks = np.zeros((n, oh, ow), np.uint8)
    masks[:, :3, :] = masks[:, -3:, :] = 1
    masks[:, :, :3] = masks[:, :, -3:] = 1
    Hs = []
    for _ in range(n):
        a, s = np.deg2rad(rng.uniform(-4, 4)), rng.uniform(0.95, 1.05)
        c, si = s * np.cos(a), s * np.sin(a)
        Hs.append(np.array([[c, -si, rng.uniform(100, fw - 1.1 * ow - 100)],
                            [si, c, rng.uniform(100, fh - 1.1 * oh - 100)],
                            [rng.uniform(-1e-6, 1e-6), rng.uniform(-1e-6, 1e-6), 1.0]]))
    return ff, fits, masks, Hs


class RunningMean(object):
    """the MaskedMovingAverage of the composed step, on the host"""

    def __init__(self, shape):
        self.avg, self.n = np.zeros(shape), np.zeros(shape, np.int32)

    def update(self, arr, mask):
        self.n[mask] += 1
        n, a, x = self.n[mask], self.avg[mask], arr[mask]
        self.avg[mask] = np.where(n == 1, x, a + (x - a) / n)


def composed_step(ctx, ff, fits, masks, Hs, Hinvs):
    obj = RunningMean(fits[0].shape)
    with np.errstate(all='ignore'):
        for f, h in zip(fits, Hinvs):
            w = warpFlatField(ff, h, f.shape, ctx=ctx)
            obj.update(f / w, w != 0)
        s = RunningMean(ff.shape)
        for f, m, h in zip(fits, masks, Hs):
            div = warpRatioToFlatField(f, obj.avg, m, h, ff.shape, ctx=ctx)
            s.update(div, div != 0)
    return obj.avg, s.avg


def event_ms(ctx, fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = ctx.event(), ctx.event()
        a.record()
        fn()
        b.record()
        ts.append(a.elapsed_ms(b))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def host_ms(ctx, fn, reps, warm=1):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--composed-reps', type=int, default=20)
    ap.add_argument('--fits', type=int, default=N)
    ap.add_argument('--obj', type=int, nargs=2, default=list(OBJ))
    ap.add_argument('--ff', type=int, nargs=2, default=list(FF))
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    n, (oh, ow), (fh, fw) = args.fits, args.obj, args.ff
    ctx = ia.default_context(0)
    lib = ctx._lib
    ff, fits, masks, Hs = scene(np.random.default_rng(0), n, (oh, ow), (fh, fw))
    Hinvs = [np.linalg.inv(h) for h in Hs]
    # what cv2 forms: the destination -> source matrices
    m_obj = np.ascontiguousarray(np.stack([np.linalg.inv(h) for h in Hinvs]))
    m_ff = np.ascontiguousarray(np.stack([np.linalg.inv(h) for h in Hs]))
    d_ff, d_fits, d_masks = ctx.to_device(ff), ctx.to_device(fits), ctx.to_device(masks)
    d_obj, d_new = ctx.empty((oh, ow), np.float64), ctx.empty((fh, fw), np.float64)
    d_on, d_fn = DeviceArray.counts(ctx, (oh, ow)), DeviceArray.counts(ctx, (fh, fw))
    d_sub = ctx.empty((-(-fh // 10), -(-fw // 10)), np.float64)

    def step_a():
        ctx._check(lib.ipa_ovs_object_dev(ctx.handle, d_ff.ptr, fh, fw, fw, d_fits.ptr, L.F64, n, oh, ow, ow, oh * ow,
                                          m_obj.ctypes.data_as(L._dp), d_obj.ptr, ow, d_on.ptr, ow), 'ovs_object')

    def step_b():
        ctx._check(lib.ipa_ovs_flatfield_dev(
            ctx.handle, d_obj.ptr, ow, d_fits.ptr, L.F64, n, oh, ow, ow, oh * ow, d_masks.ptr, ow, oh * ow,
            m_ff.ctypes.data_as(L._dp), d_new.ptr, fh, fw, fw, d_fn.ptr, fw, 1, d_sub.ptr, 10, d_sub.shape[1]),
            'ovs_flatfield')

    def fused():
        step_a()
        step_b()
        return d_sub.get()   # the residuum's grid comes down every step

    a_ms = event_ms(ctx, step_a, args.reps)
    b_ms = event_ms(ctx, step_b, args.reps)
    fused_ev = event_ms(ctx, fused, args.reps)
    fused_host = host_ms(ctx, fused, args.reps)
    composed_host = host_ms(ctx, lambda: composed_step(ctx, ff, fits, masks, Hs, Hinvs), args.composed_reps)
    # the same bits
    obj_c, new_c = composed_step(ctx, ff, fits, masks, Hs, Hinvs)
    fused()
    equal = bool(np.array_equal(d_obj.get(), obj_c, equal_nan=True) and
                 np.array_equal(d_new.get(), np.clip(new_c, 0, 1), equal_nan=True))
    coverage = float(np.mean(d_fn.get() > 0))
    bytes_a = n * oh * ow * 8 + fh * fw * 8 + oh * ow * (8 + 4)
    bytes_b = n * oh * ow * (8 + 1) + oh * ow * 8 + fh * fw * (8 + 4)
    half = max(bytes_a, bytes_b) // 2
    src, dst = ctx.empty((half,), np.uint8), ctx.empty((half,), np.uint8)
    copy = event_ms(ctx, lambda: dst.copy_from(src), args.reps)
    copy_rate = 2 * half / (copy[0] * 1e-3)

    def kernel_row(ms, nbytes):
        rate = nbytes / (ms[0] * 1e-3)
        return {'ms': round(ms[0], 4), 'ms_min_max': [round(ms[1], 4), round(ms[2], 4)], 'compulsory_bytes': int(nbytes),
                'GB_per_s': round(rate / 1e9, 1), 'fraction_of_copy_rate': round(rate / copy_rate, 4)}

    line = json.dumps({
        'metric': 'ovs_step', 'device': ctx.device_info().get('name'), 'fits': n, 'obj': [oh, ow], 'ff': [fh, fw],
        'reps': args.reps, 'object_kernel': kernel_row(a_ms, bytes_a), 'flatfield_kernel': kernel_row(b_ms, bytes_b),
        'fused_step_ms_events': round(fused_ev[0], 4), 'fused_step_ms_host_clock': round(fused_host[0], 4),
        'fused_step_ms_host_clock_min_max': [round(fused_host[1], 4), round(fused_host[2], 4)], 'fused_launches': 2,
        'composed_step_ms_host_clock': round(composed_host[0], 2),
        'composed_step_ms_host_clock_min_max': [round(composed_host[1], 2), round(composed_host[2], 2)],
        'composed_launches': 2 * n, 'composed_reps': args.composed_reps,
        'speedup': round(composed_host[0] / fused_host[0], 1), 'same_bits': equal,
        'flat_field_coverage': round(coverage, 3),
        'd2d_copy_GB_per_s': round(copy_rate / 1e9, 1)})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fo:
            fo.write(line + '\n')
    if not equal:
        sys.exit('the fused and the composed step differ')
    if not fused_host[0] < composed_host[0]:
        sys.exit('the fused step is not faster than the composed step')


if __name__ == '__main__':
    main()
