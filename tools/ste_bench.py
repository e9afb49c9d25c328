#!/usr/bin/env python3
"""Single-time-effect removal on device-resident 4K stacks: one JSON line.

For stacks of 2, 4, 8 and 16 frames of 3840 x 2160 (uint16 and float32) it times the
constructor's work (ipa_ste_dev with the first pair and a (minY, ax, ay) NLF) with HIP events,
median of --reps calls after warm-up, and reports
  - the compulsory bytes: the N frames read once + the state written (avg 8 + thr 8 + count 4
    = 20 B/px), and the fraction of the 8 TB/s peak they reach;
  - a device-to-device copy of the same byte count in the same process;
  - the same stack as one launch per frame (tuning knob ste_frames = 1).

    python tools/ste_bench.py [--reps 20] [--out profiles/ste_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import imgprocessor_amd as ia  # noqa: E402
from imgprocessor_amd import _lib as L  # noqa: E402

H, W = 2160, 3840
PEAK = 8.0e12


def median_ms(ctx, fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = ctx.event(), ctx.event()
        a.record()
        fn()
        b.record()
        ts.append(a.elapsed_ms(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    ctx = ia.default_context(0)
    lib = ctx._lib
    nlf = L.dbl((3.0, 150.0, 1.1), 3)
    avg = ctx.empty((H, W), np.float64)
    thr = ctx.empty((H, W), np.float64)
    cnt = ia.DeviceArray.counts(ctx, (H, W))
    rng = np.random.default_rng(0)
    rows = []
    for dtype in (np.uint16, np.float32):
        for n in (2, 4, 8, 16):
            f = (1000 + 30 * rng.standard_normal((n, H, W))).astype(dtype)
            f[:, ::97, ::89] += dtype(3000)
            d = ctx.to_device(f)
            del f

            def run():
                ctx._check(lib.ipa_ste_dev(ctx.handle, d.ptr, ia.device.dtype_id(d.dtype), n, H, W,
                                           W, H * W, 1, nlf, 4.0, avg.ptr, cnt.ptr, thr.ptr, W,
                                           None, None, None, W), 'ste')

            ms = median_ms(ctx, run, args.reps)
            ctx.set_tuning(ste_frames=1)
            try:
                ms1 = median_ms(ctx, run, args.reps)
            finally:
                ctx.set_tuning(ste_frames=8)
            nbytes = n * H * W * np.dtype(dtype).itemsize + 20 * H * W
            src = ctx.empty((nbytes,), np.uint8)
            dst = ctx.empty((nbytes,), np.uint8)
            mc = median_ms(ctx, lambda: dst.copy_from(src), args.reps)
            del src, dst, d
            ctx.trim()
            rows.append({'dtype': np.dtype(dtype).name, 'frames': n, 'ms': round(ms, 4),
                         'compulsory_bytes': int(nbytes),
                         'peak_fraction': round(nbytes / (ms * 1e-3) / PEAK, 4),
                         'd2d_copy_ms': round(mc, 4), 'vs_d2d': round(ms / mc, 3),
                         'f1_launches_ms': round(ms1, 4), 'halo_speedup': round(ms1 / ms, 3)})
    info = ctx.device_info()
    line = json.dumps({'metric': 'ste_4k', 'device': info.get('name'), 'shape': [H, W],
                       'reps': args.reps, 'rows': rows})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fo:
            fo.write(line + '\n')


if __name__ == '__main__':
    main()
