#!/usr/bin/env python3
"""Temporal signal stability on device-resident 4K stacks: one JSON line.

For stacks of 15 (the reference demo's count) and 64 frames of 3840 x 2160 (uint16 and float32)
it times, with HIP events, the median of --reps calls after warm-up:
  - ipa_tss_event_length_dev on its own (avlen and the zero mask; and once more with the
    optional (T, h, w) event cube), and reports
      * the compulsory bytes: the T frames read once + offset, ascent and error read + avlen
        written (T * itemsize + 32 B/px), and the fraction of the 8 TB/s peak they reach,
      * a device-to-device copy of the same byte count in the same process;
  - the other launches of the routine: ipa_stack_linregress_dev, ipa_masked_mean_dev (7 x 7),
    ipa_tss_finish_dev;
  - the whole temporalSignalStability call on the device stack.

    python tools/tss_bench.py [--reps 20] [--out profiles/tss_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import imgprocessor_amd as ia  # noqa: E402
from imgprocessor_amd import _lib as L, ops  # noqa: E402
from imgprocessor_amd.uncertainty import temporalSignalStability  # noqa: E402

H, W = 2160, 3840
PEAK = 8.0e12


def timed_ms(ctx, fn, reps, warm=3):
    """-> (median, min, max) of `reps` event-timed calls"""
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


def stack_on_device(ctx, T, dtype, rng):
    """a decaying gradient with noise and blocks that fluctuate, uploaded frame by frame"""
    d = ctx.empty((T, H, W), dtype)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    base = 1000 + 300 * np.sin(x / 211) * np.cos(y / 173)
    blocks = ((x // 64 + y // 64) % 5 == 0).astype(np.float32)
    del x, y
    for k in range(T):
        f = base - 2.0 * k + 30 * rng.standard_normal((H, W), dtype=np.float32) + 60 * np.sin(0.9 * k) * blocks
        d.frame(k).set(np.clip(np.round(f), 0, 65535).astype(dtype) if np.dtype(dtype).kind == 'u' else f.astype(dtype))
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--frames', type=int, nargs='*', default=[15, 64])
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    ctx = ia.default_context(0)
    lib = ctx._lib
    rng = np.random.default_rng(0)
    rows = []
    for dtype in (np.uint16, np.float32):
        for T in args.frames:
            d = stack_on_device(ctx, T, dtype, rng)
            times = np.ascontiguousarray(np.linspace(0.0, 100.0, T))
            tp = times.ctypes.data_as(L._dp)
            off, asc, err = ops.stack_linregress(times, d, mx_intensity=np.inf, min_ascent=0)
            avlen = ctx.empty((H, W), np.float64)
            mean = ctx.empty((H, W), np.float64)
            out = ctx.empty((H, W), np.float64)
            zero = ctx.empty((H, W), np.uint8)
            did = ia.device.dtype_id(d.dtype)

            def events(cube=None):
                ctx._check(lib.ipa_tss_event_length_dev(
                    ctx.handle, d.ptr, did, T, H, W, W, H * W, tp, off.ptr, asc.ptr, err.ptr, W, avlen.ptr, W,
                    zero.ptr, W, cube.ptr if cube is not None else None, W, H * W), 'tss_event_length')

            def fit():
                ctx._check(lib.ipa_stack_linregress_dev(
                    ctx.handle, d.ptr, did, T, H, W, W, H * W, tp, float('inf'), 0.0, off.ptr, asc.ptr, err.ptr, W),
                    'stack_linregress')

            def masked():
                ctx._check(lib.ipa_masked_mean_dev(ctx.handle, avlen.ptr, 3, zero.ptr, H, W, W, W, 7, 0, mean.ptr, W),
                           'masked_mean')

            def finish():
                ctx._check(lib.ipa_tss_finish_dev(ctx.handle, mean.ptr, zero.ptr, H, W, W, W, out.ptr, W), 'tss_finish')

            ms = timed_ms(ctx, events, args.reps)
            cube = ctx.empty((T, H, W), np.uint8)
            ms_cube = timed_ms(ctx, lambda: events(cube), args.reps)
            del cube
            ms_fit = timed_ms(ctx, fit, args.reps)
            events()
            ms_mean = timed_ms(ctx, masked, args.reps)
            ms_fin = timed_ms(ctx, finish, args.reps)
            ms_all = timed_ms(ctx, lambda: temporalSignalStability(d, times), args.reps)
            event_share = float(np.mean(zero.get() == 0))
            nbytes = T * H * W * np.dtype(dtype).itemsize + 32 * H * W
            src = ctx.empty((nbytes,), np.uint8)
            dst = ctx.empty((nbytes,), np.uint8)
            mc = timed_ms(ctx, lambda: dst.copy_from(src), args.reps)
            del src, dst, d, off, asc, err, avlen, mean, out, zero
            ctx.trim()
            rows.append({'dtype': np.dtype(dtype).name, 'T': T,
                         'event_length_ms': round(ms[0], 4), 'event_length_ms_min_max': [round(ms[1], 4), round(ms[2], 4)],
                         'compulsory_bytes': int(nbytes),
                         'peak_fraction': round(nbytes / (ms[0] * 1e-3) / PEAK, 4),
                         'd2d_copy_ms': round(mc[0], 4), 'vs_d2d': round(ms[0] / mc[0], 3),
                         'ns_per_voxel': round(ms[0] * 1e6 / (T * H * W), 5),
                         'event_length_with_cube_ms': round(ms_cube[0], 4),
                         'stack_linregress_ms': round(ms_fit[0], 4), 'masked_mean_ms': round(ms_mean[0], 4),
                         'finish_ms': round(ms_fin[0], 4),
                         'temporalSignalStability_ms': round(ms_all[0], 4),
                         'temporalSignalStability_ms_min_max': [round(ms_all[1], 4), round(ms_all[2], 4)],
                         'pixels_with_events': round(event_share, 4)})
    info = ctx.device_info()
    line = json.dumps({'metric': 'tss_4k', 'device': info.get('name'), 'shape': [H, W], 'reps': args.reps,
                       'rows': rows})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fo:
            fo.write(line + '\n')


if __name__ == '__main__':
    main()
