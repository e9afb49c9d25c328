#!/usr/bin/env python3
"""Dark current calibration on device-resident 4K frames: one JSON line.

For 3840 x 2160 frames it times, with HIP events around --inner back-to-back calls, median of
--reps windows after warm-up,
  - ipa_stack_linregress_dev through the C ABI for stacks of T = 6 and T = 16 frames, uint16 and
    float32, beside its compulsory bytes (T * h * w * elem read + 24 * h * w written), the
    fraction of the 8 TB/s peak they reach, and ipa_memcpy_d2d of a buffer of that many bytes in
    the same process (the copy moves every byte twice: the convention of tools/nlf_bench.py);
  - getDarkCurrentFunction as a whole on a device-resident series of 16 uint16 frames over 6
    exposure times (1, 2, 3, 3, 3 and 4 frames), Python included, and its stages one by one with
    a host clock around work that ends in a synchronise: the noise level function of every group
    (pair_min, calcNLF's three kernels, the host fit), the single-time-effect average, the cast
    and the fit.

    python tools/dark_bench.py [--reps 20] [--inner 10] [--out profiles/dark_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import imgprocessor_amd as ia  # noqa: E402
from imgprocessor_amd import ops  # noqa: E402
from imgprocessor_amd.camera import DarkCurrentMap as D  # noqa: E402
from imgprocessor_amd.camera.NoiseLevelFunction import oneImageNLF  # noqa: E402
from imgprocessor_amd.features.SingleTimeEffectDetection import SingleTimeEffectDetection  # noqa: E402

H, W = 2160, 3840
PEAK = 8.0e12
SERIES_TIMES = [1.0] + [2.0] * 2 + [4.0] * 3 + [8.0] * 3 + [16.0] * 3 + [32.0] * 4


def median_ms(ctx, fn, reps, inner, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = ctx.event(), ctx.event()
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        ts.append(a.elapsed_ms(b) / inner)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def dark_frame(t, rng, dtype):
    f = 200.0 + 0.3 * t + 3.0 * rng.standard_normal((H, W))
    return (np.round(f) if np.dtype(dtype).kind == 'u' else f).astype(dtype)


def wall_ms(ctx, fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def series_stages(ctx, times, frames):
    """getDarkCurrentFunction's flow, stage by stage -> milliseconds per stage"""
    ms = {'nlf': 0.0, 'ste': 0.0, 'cast': 0.0, 'fit': 0.0}
    x, groups = D.sortForSameExpTime(times, frames)
    stack = ctx.empty((len(x), H, W), frames[0].dtype)
    for n, group in enumerate(groups):
        if len(group) == 1:
            stack.frame(n).copy_from(group[0])
            continue
        t, nlf = wall_ms(ctx, lambda: oneImageNLF(ops.pair_min(group[0], group[1]))[0])
        ms['nlf'] += t

        def ste():
            s = SingleTimeEffectDetection(group[:2], nlf, nStd=3)
            for f in group[2:]:
                s.addImage(f)
            return s
        t, s = wall_ms(ctx, ste)
        ms['ste'] += t
        ms['cast'] += wall_ms(ctx, lambda: ops.cast_trunc(s.noSTE, stack.dtype, out=stack.frame(n)))[0]
    ms['fit'] = wall_ms(ctx, lambda: D.getLinearityFunction(x, stack))[0]
    return {k: round(v, 3) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    ctx = ia.default_context(0)
    lib = ctx._lib
    dp = C.POINTER(C.c_double)
    rng = np.random.default_rng(0)
    outs = [ctx.empty((H, W), np.float64) for _ in range(3)]
    rows = []
    for dtype in (np.uint16, np.float32):
        for T in (6, 16):
            times = np.array([1.0, 2.0, 4.0, 8.0, 16.0, 32.0] if T == 6 else np.arange(1.0, 17.0))
            d = ctx.to_device(np.stack([dark_frame(t, rng, dtype) for t in times]))
            dt, es = ia.device.dtype_id(d.dtype), np.dtype(dtype).itemsize

            def fit():
                ctx._check(lib.ipa_stack_linregress_dev(
                    ctx.handle, d.ptr, dt, T, H, W, W, H * W, times.ctypes.data_as(dp), 65535.0, 0.001,
                    outs[0].ptr, outs[1].ptr, outs[2].ptr, W), 'stack_linregress')
            nbytes = (T * es + 24) * H * W
            ms = median_ms(ctx, fit, args.reps, args.inner)
            src, dst = ctx.empty((nbytes,), np.uint8), ctx.empty((nbytes,), np.uint8)
            mc = median_ms(ctx, lambda: dst.copy_from(src), args.reps, args.inner)
            del src, dst, d
            ctx.trim()
            rows.append({'dtype': np.dtype(dtype).name, 'T': T, 'ms': round(ms[0], 4),
                         'ms_min_max': [round(ms[1], 4), round(ms[2], 4)], 'compulsory_bytes': int(nbytes),
                         'bytes_per_s': round(nbytes / (ms[0] * 1e-3), 0),
                         'peak_fraction': round(nbytes / (ms[0] * 1e-3) / PEAK, 4),
                         'd2d_copy_ms': round(mc[0], 4), 'vs_d2d': round(ms[0] / mc[0], 3)})
    # the whole calibration of a device-resident series
    frames = [ctx.to_device(dark_frame(t, rng, np.uint16)) for t in SERIES_TIMES]
    for _ in range(2):
        D.getDarkCurrentFunction(SERIES_TIMES, frames)
    whole = [wall_ms(ctx, lambda: D.getDarkCurrentFunction(SERIES_TIMES, frames))[0] for _ in range(5)]
    stages = series_stages(ctx, SERIES_TIMES, frames)
    info = ctx.device_info()
    line = json.dumps({'metric': 'dark_current_4k', 'device': info.get('name'), 'shape': [H, W],
                       'reps': args.reps, 'inner': args.inner, 'stack_linregress': rows,
                       'series': {'frames': len(SERIES_TIMES), 'exposure_times': 6, 'dtype': 'uint16',
                                  'getDarkCurrentFunction_ms': round(float(np.median(whole)), 3),
                                  'getDarkCurrentFunction_ms_min_max': [round(min(whole), 3), round(max(whole), 3)],
                                  'stages_ms': stages}})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fo:
            fo.write(line + '\n')


if __name__ == '__main__':
    main()
