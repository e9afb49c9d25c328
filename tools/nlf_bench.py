#!/usr/bin/env python3
"""Noise level function estimation on device-resident 4K frames: one JSON line.

For 3840 x 2160 frames (uint16 and float64; a noisy gradient scene, whose pixels spread over all
100 bins, and a flat one, whose pixels crowd into a few) it times, with HIP events, median of
--reps calls after warm-up,
  - each kernel call of calcNLF through the C ABI: the signal (3x3 median), the moments (two
    passes and their two final kernels) and the binned reduction (with its final kernel and the
    copy of the 100 results to the host);
  - calcNLF as a whole, Python included;
and reports each beside its compulsory bytes (signal: the frame read + 8 B/px written; moments:
the signal read twice; bins: the frame and the signal read), the fraction of the 8 TB/s peak
they reach, and a device-to-device copy of a buffer of that many bytes in the same process (the
convention of tools/ste_bench.py).

    python tools/nlf_bench.py [--reps 20] [--out profiles/nlf_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import imgprocessor_amd as ia  # noqa: E402
from imgprocessor_amd.camera import NoiseLevelFunction as N  # noqa: E402

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


def scene(kind, dtype, rng):
    if kind == 'gradient':
        y, x = np.mgrid[0:H, 0:W].astype(np.float64)
        base = 200 + 3000 * (x + y) / (H + W - 2)
        f = base + 0.8 * np.sqrt(base) * rng.standard_normal((H, W))
    else:
        f = 1000 + 3 * rng.standard_normal((H, W))
    return (np.round(f) if np.dtype(dtype).kind == 'u' else f).astype(dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    ctx = ia.default_context(0)
    lib = ctx._lib
    dp = C.POINTER(C.c_double)
    rng = np.random.default_rng(0)
    sig = ctx.empty((H, W), np.float64)
    rows = []
    for kind in ('gradient', 'flat'):
        for dtype in (np.uint16, np.float64):
            d = ctx.to_device(scene(kind, dtype, rng))
            dt, es, px = ia.device.dtype_id(d.dtype), np.dtype(dtype).itemsize, H * W

            def signal():
                ctx._check(lib.ipa_nlf_signal_dev(ctx.handle, d.ptr, dt, None, H, W, W, 0, None, 0, 0.0,
                                                  sig.ptr, W), 'signal')
            m = np.empty(5)

            def moments():
                ctx._check(lib.ipa_nlf_moments_dev(ctx.handle, sig.ptr, 3, H, W, W, m.ctypes.data_as(dp)),
                           'moments')
            signal()
            mn, mx, nbins, _ = N._binning(None, sig, (H, W))
            step = (mx - mn) / nbins
            e = N._edges(mn, step, nbins)
            cnt, sm = np.zeros(nbins, np.uint64), np.zeros(nbins)

            def bins():
                ctx._check(lib.ipa_nlf_bins_dev(ctx.handle, d.ptr, dt, None, H, W, W, 0, None, 0, 0.0, sig.ptr,
                                                W, e.ctypes.data_as(dp), nbins, step, N.F_NOISE_WITH_MEDIAN, 0,
                                                cnt.ctypes.data_as(C.c_void_p), sm.ctypes.data_as(dp)), 'bins')
            parts = {'signal': (signal, (es + 8) * px), 'moments': (moments, 16 * px),
                     'bins': (bins, (es + 8) * px), 'calcNLF': (lambda: N.calcNLF(d), (2 * es + 32) * px)}
            row = {'scene': kind, 'dtype': np.dtype(dtype).name, 'nbins': int(nbins),
                   'occupied_bins': None}
            for name, (fn, nbytes) in parts.items():
                ms = median_ms(ctx, fn, args.reps)
                src, dst = ctx.empty((nbytes,), np.uint8), ctx.empty((nbytes,), np.uint8)
                mc = median_ms(ctx, lambda: dst.copy_from(src), args.reps)
                del src, dst
                ctx.trim()
                row[name] = {'ms': round(ms, 4), 'compulsory_bytes': int(nbytes),
                             'peak_fraction': round(nbytes / (ms * 1e-3) / PEAK, 4),
                             'd2d_copy_ms': round(mc, 4), 'vs_d2d': round(ms / mc, 3)}
            row['occupied_bins'] = int(np.count_nonzero(cnt))
            rows.append(row)
            del d
            ctx.trim()
    info = ctx.device_info()
    line = json.dumps({'metric': 'nlf_4k', 'device': info.get('name'), 'shape': [H, W],
                       'reps': args.reps, 'rows': rows})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fo:
            fo.write(line + '\n')


if __name__ == '__main__':
    main()
