#!/usr/bin/env python3
"""2-D polynomial fits of a masked 4K field on the device: one JSON line.

On a device-resident 2160 x 3840 float64 field with a 30 % mask it times, with HIP events, the median
of --reps calls after warm-up:
  - ipa_poly2d_moments_dev at orders 2, 3 and 5 (each call ends with its sums on the host; the same call
    on an 8 x 64 frame is timed beside them: the cost of two launches and the wait for the result),
  - ipa_poly2d_eval_dev filling the masked pixels at the same orders, into a copy (what the POLY repair
    loop does) and in place, both with the residuum,
  - ipa_high_grad_dev,
  each beside its compulsory bytes - the frame and the mask read once, the filled pixels (or the
  copy, or the mask) written once -, the fraction of the 8 TB/s peak they reach, and a
  device-to-device copy of the same byte count in the same process;
  - one whole polynomial() call ('POLY repair') on the device field, with its iterations.
Beside these, on the host: the reference's method - the design matrix of raw pixel monomials handed to
np.linalg.lstsq, then the polynomial evaluated at the masked pixels - restated in numpy at 270 x 480,
order 2 (at 4K its design matrix alone is 600 MB), with the rms residuals of both fits there.

    python tools/poly_bench.py [--reps 20] [--out profiles/poly_bench.json]
"""
import argparse
import ctypes as C
import itertools
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import imgprocessor_amd as ia  # noqa: E402
from imgprocessor_amd import _lib as L, ops  # noqa: E402
from imgprocessor_amd.camera.flatField import polynomial  # noqa: E402
from imgprocessor_amd.interpolate import polyfit2dGrid  # noqa: E402

H, W = 2160, 3840
PEAK = 8.0e12
ORDERS = (2, 3, 5)


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


def scene(h, w, seed=0, noise=0.001, frac=0.3):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    f = 1.0 - 0.6 * (((x - 0.45 * w) / w) ** 2 + ((y - 0.55 * h) / h) ** 2) + noise * rng.standard_normal((h, w))
    return f, rng.random((h, w)) < frac


def monomial_fit(arr, mask, order):
    """the reference's method, restated: raw monomials x**i * y**j, lstsq, evaluation at the masked pixels"""
    y, x = np.nonzero(~mask)
    ij = list(itertools.product(range(order + 1), repeat=2))
    G = np.stack([x.astype(np.float64) ** i * y.astype(np.float64) ** j for i, j in ij], 1)
    p = np.linalg.lstsq(G, arr[~mask], rcond=None)[0]
    resid = np.sqrt(np.mean((G @ p - arr[~mask]) ** 2))
    yy, xx = np.nonzero(mask)
    out = arr.copy()
    out[mask] = sum(a * xx.astype(np.float64) ** i * yy.astype(np.float64) ** j for a, (i, j) in zip(p, ij))
    return out, float(resid), float(np.linalg.cond(G))


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
    a, m = scene(H, W)
    d_a, d_m = ctx.to_device(a), ctx.to_device(m.view(np.uint8))
    d_out = ctx.empty((H, W), np.float64)
    d_hg = ctx.empty((H, W), np.uint8)
    n_masked = int(m.sum())
    px = H * W

    copies = {}

    def copy_ms(nbytes):
        """a device-to-device copy moves nbytes / 2 in and nbytes / 2 out"""
        if nbytes not in copies:
            src, dst = ctx.empty((nbytes // 2,), np.uint8), ctx.empty((nbytes // 2,), np.uint8)
            copies[nbytes] = timed_ms(ctx, lambda: dst.copy_from(src), args.reps)[0]
        return copies[nbytes]

    out = {'moments': {}, 'fill_copy': {}, 'fill_in_place': {}}
    res = C.c_double()
    for o in ORDERS:
        mom = np.empty((2 * o + 1) ** 2 + (o + 1) ** 2 + 1)

        def moments():
            ctx._check(lib.ipa_poly2d_moments_dev(ctx.handle, d_a.ptr, 3, H, W, W, d_m.ptr, W, o,
                                                  mom.ctypes.data_as(L._dp)), 'moments')

        nb = 9 * px
        out['moments'][str(o)] = row(timed_ms(ctx, moments, args.reps), nb, copy_ms(nb))
        coef = np.ascontiguousarray(ops.poly2d_solve(*ops.poly2d_moments(d_a, d_m, o), o))
        cp = coef.ctypes.data_as(L._dp)

        def fill(dst):
            ctx._check(lib.ipa_poly2d_eval_dev(ctx.handle, cp, o, L.POLY_FILL, d_a.ptr, 3, H, W, W, d_m.ptr, W, None,
                                               None, 0, 0, 0, dst.ptr, W, C.byref(res)), 'fill')

        nb = 17 * px                       # frame + mask in, the copy out
        out['fill_copy'][str(o)] = row(timed_ms(ctx, lambda: fill(d_out), args.reps), nb, copy_ms(nb))
        nb = px + 16 * n_masked            # mask in, the masked pixels in (the residuum) and out
        out['fill_in_place'][str(o)] = row(timed_ms(ctx, lambda: fill(d_a), args.reps), nb, copy_ms(nb))
        d_a.set(a)

    # what a call costs before it moves a frame: two launches, 35 numbers to the host, the wait for them
    d_small = ctx.to_device(a[:8, :64].copy())
    small = np.empty(35)
    floor = timed_ms(ctx, lambda: ctx._check(lib.ipa_poly2d_moments_dev(
        ctx.handle, d_small.ptr, 3, 8, 64, 64, None, 64, 2, small.ctypes.data_as(L._dp)), 'moments'), args.reps)
    out['moments_call_floor_8x64_ms'] = round(floor[0], 4)

    cnt = C.c_double()

    def high():
        ctx._check(lib.ipa_high_grad_dev(ctx.handle, d_out.ptr, 3, H, W, W, 0.01, 15, d_hg.ptr, W, C.byref(cnt)),
                   'high_grad')

    nb = 9 * px                            # frame in, mask out
    out['high_grad'] = row(timed_ms(ctx, high, args.reps), nb, copy_ms(nb))
    out['high_grad']['masked_fraction'] = round(cnt.value / px, 4)

    trace = []
    polynomial(d_a, d_m, trace=trace)
    ms = timed_ms(ctx, lambda: polynomial(d_a, d_m), max(3, args.reps // 4), warm=1)
    out['polynomial'] = {'ms': round(ms[0], 3), 'ms_min_max': [round(ms[1], 3), round(ms[2], 3)],
                         'iterations': len(trace),
                         'residua': [None if r is None else float('%.4g' % r) for r, _ in trace],
                         'high_gradient_pixels': [k for _, k in trace]}

    # the host yardstick, where its design matrix still fits and is still usable
    h, w = H // 8, W // 8
    sa, sm = scene(h, w, 1)
    t0 = time.perf_counter()
    host_out, host_rms, cond = monomial_fit(sa, sm, 2)
    host_ms = (time.perf_counter() - t0) * 1e3
    polyfit2dGrid(sa, sm, order=2, ctx=ctx)
    t0 = time.perf_counter()
    dev_out = polyfit2dGrid(sa, sm, order=2, ctx=ctx)
    dev_ms = (time.perf_counter() - t0) * 1e3
    fit_all = polyfit2dGrid(sa, sm, order=2, replace_all=True, ctx=ctx)
    out['host_monomial_lstsq_270x480_o2'] = {
        'ms': round(host_ms, 2), 'cond': float('%.3g' % cond), 'rms_residual': float('%.3g' % host_rms),
        'device_call_from_host_arrays_ms': round(dev_ms, 2),
        'device_rms_residual': float('%.3g' % np.sqrt(np.mean((fit_all[~sm] - sa[~sm]) ** 2))),
        'max_difference': float('%.3g' % np.abs(dev_out - host_out).max())}

    info = ctx.device_info()
    line = json.dumps(dict({'metric': 'poly_4k', 'device': info.get('name'), 'shape': [H, W], 'dtype': 'float64',
                            'masked_fraction': round(n_masked / px, 4), 'reps': args.reps}, **out))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fo:
            fo.write(line + '\n')


if __name__ == '__main__':
    main()
