#!/usr/bin/env python3
"""Kang-Weiss and angle-of-view fits of a masked 4K field on the device: one JSON line.

On a device-resident 2160 x 3840 field with a 30 % mask, float64 and float32, it times with HIP events
the median of --reps calls after warm-up:
  - one ipa_fn2d_normal_dev call per model (each call ends with its sums on the host; the same call on
    an 8 x 64 frame is timed beside them: the cost of two launches and the wait for the result),
  - ipa_poly2d_moments_dev at order 2 on the same field in the same process: the kernel that reads the
    same compulsory bytes - the frame and the mask once,
  - a device-to-device copy of those bytes,
  - ipa_fn2d_eval_dev in its three modes (fill into a copy, rewrite, an outgrid of the frame's size), with
    the maximum,
  - one whole function(..., replace_all=True) ('KW replace') and one whole repair on the device field,
    with the normal-equation calls their fits made.
The host side is not timed here: the JSON carries the measurement recorded with the feature request,
scipy.optimize.curve_fit on the reference's own vignetting() at 540 x 960.

    python tools/fn2d_bench.py [--reps 20] [--out profiles/fn2d_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import imgprocessor_amd as ia  # noqa: E402
from imgprocessor_amd import _lib as L, ops  # noqa: E402
from imgprocessor_amd.camera.flatField import function  # noqa: E402

H, W = 2160, 3840
PEAK = 8.0e12
TRUE = (1900.0, 1e-4, 1010.3, 2000.6)


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


def scene(h, w, dtype, seed=0, noise=0.01, frac=0.3):
    rng = np.random.default_rng(seed)
    x, y = np.mgrid[0:h, 0:w].astype(np.float64)
    f, alpha, cx, cy = TRUE
    d = np.sqrt((x - cx) ** 2 + (y - cy) ** 2)
    field = (1 - alpha * d) / (1 + (d / f) ** 2) ** 2 + noise * rng.standard_normal((h, w))
    return field.astype(dtype), rng.random((h, w)) < frac


def row(ms, nbytes, copy_ms):
    return {'ms': round(ms[0], 4), 'ms_min_max': [round(ms[1], 4), round(ms[2], 4)], 'compulsory_bytes': int(nbytes),
            'peak_fraction': round(nbytes / (ms[0] * 1e-3) / PEAK, 4), 'd2d_copy_ms': round(copy_ms, 4),
            'vs_d2d': round(ms[0] / copy_ms, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    ctx = ia.default_context(0)
    lib = ctx._lib
    px = H * W
    copies = {}

    def copy_ms(nbytes):
        """a device-to-device copy moves nbytes / 2 in and nbytes / 2 out"""
        if nbytes not in copies:
            src, dst = ctx.empty((nbytes // 2,), np.uint8), ctx.empty((nbytes // 2,), np.uint8)
            copies[nbytes] = timed_ms(ctx, lambda: dst.copy_from(src), args.reps)[0]
        return copies[nbytes]

    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    d_yy, d_xx = ctx.to_device(yy + 0.25), ctx.to_device(xx - 0.25)
    del yy, xx
    out = {}
    for dtype in (np.float64, np.float32):
        es, dt = np.dtype(dtype).itemsize, L.F64 if dtype == np.float64 else L.F32
        a, m = scene(H, W, dtype)
        d_a, d_m = ctx.to_device(a), ctx.to_device(m.view(np.uint8))
        d_out = ctx.empty((H, W), dtype)
        n_masked = int(m.sum())
        r = {'masked_fraction': round(n_masked / px, 4)}
        guess = {'KW': (H * 0.7, 0.0, H / 2, W / 2), 'AoV': (0.01, H / 2, W / 2)}
        nb = (es + 1) * px                     # the frame and the mask read once
        for model, mid in (('KW', L.FN2D_KW), ('AoV', L.FN2D_AOV)):
            par = np.array(guess[model], dtype=np.float64)
            par[0] = np.tan(par[0]) if model == 'AoV' else par[0]
            sums = np.empty(16)

            def normal():
                ctx._check(lib.ipa_fn2d_normal_dev(ctx.handle, d_a.ptr, dt, H, W, W, d_m.ptr, W, mid,
                                                   par.ctypes.data_as(L._dp), sums.ctypes.data_as(L._dp)), 'normal')

            r['normal_' + model] = row(timed_ms(ctx, normal, args.reps), nb, copy_ms(nb))
        mom = np.empty(35)

        def moments():
            ctx._check(lib.ipa_poly2d_moments_dev(ctx.handle, d_a.ptr, dt, H, W, W, d_m.ptr, W, 2,
                                                  mom.ctypes.data_as(L._dp)), 'moments')

        r['poly2d_moments_o2'] = row(timed_ms(ctx, moments, args.reps), nb, copy_ms(nb))
        r['normal_KW_vs_poly2d_moments_o2'] = round(r['normal_KW']['ms'] / r['poly2d_moments_o2']['ms'], 3)
        r['normal_AoV_vs_poly2d_moments_o2'] = round(r['normal_AoV']['ms'] / r['poly2d_moments_o2']['ms'], 3)

        # what a call costs before it moves a frame: two launches, 16 numbers to the host, the wait for them
        d_small = ctx.to_device(a[:8, :64].copy())
        par = np.array(TRUE)
        small = np.empty(16)
        floor = timed_ms(ctx, lambda: ctx._check(lib.ipa_fn2d_normal_dev(
            ctx.handle, d_small.ptr, dt, 8, 64, 64, None, 64, L.FN2D_KW, par.ctypes.data_as(L._dp),
            small.ctypes.data_as(L._dp)), 'normal'), args.reps)
        r['normal_call_floor_8x64_ms'] = round(floor[0], 4)

        top = C.c_double()

        def evaluate(mode, gy=None, gx=None):
            ctx._check(lib.ipa_fn2d_eval_dev(ctx.handle, L.FN2D_KW, par.ctypes.data_as(L._dp), mode, d_a.ptr, dt, H, W,
                                             W, d_m.ptr, W, gy, gx, H if gy else 0, W if gy else 0, W, d_out.ptr, W,
                                             C.byref(top)), 'eval')

        nb = (2 * es + 1) * px                 # frame + mask in, the copy out
        r['eval_fill_copy'] = row(timed_ms(ctx, lambda: evaluate(L.POLY_FILL), args.reps), nb, copy_ms(nb))
        nb = es * px                           # the frame out
        r['eval_all'] = row(timed_ms(ctx, lambda: evaluate(L.POLY_ALL), args.reps), nb, copy_ms(nb))
        nb = (16 + es) * px                    # two float64 position frames in, the frame out
        r['eval_outgrid'] = row(timed_ms(ctx, lambda: evaluate(L.POLY_GRID, d_yy.ptr, d_xx.ptr), args.reps), nb,
                                copy_ms(nb))

        for name, kw in (('function_replace_all', dict(replace_all=True)), ('function_repair', dict())):
            fit = ops.fn2d_fit(d_a, d_m, 'KW', guess['KW'])
            ms = timed_ms(ctx, lambda: function(d_a, d_m, **kw), max(3, args.reps // 4), warm=1)
            r[name] = {'ms': round(ms[0], 3), 'ms_min_max': [round(ms[1], 3), round(ms[2], 3)],
                       'normal_calls': fit[3], 'params': [float('%.6g' % v) for v in fit[0]]}
        out[np.dtype(dtype).name] = r
        del d_a, d_m, d_out

    out['host_curve_fit_540x960'] = {
        's': 0.72, 'measured_here': False,
        'note': 'scipy.optimize.curve_fit on the reference\'s vignetting(), noisy 540 x 960 field, on the host of the '
                'session that wrote the feature request; not re-measured by this tool'}
    out['kernel_times_from_a_profiler_trace'] = 'not taken'
    info = ctx.device_info()
    line = json.dumps(dict({'metric': 'fn2d_4k', 'device': info.get('name'), 'shape': [H, W], 'reps': args.reps}, **out))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fo:
            fo.write(line + '\n')


if __name__ == '__main__':
    main()
