#!/usr/bin/env python3
"""The flat field from spot images on 4K frames on the device: one JSON line.

On device-resident 2160 x 3840 uint16 and float32 frames with one 30 x 30 spot it times, with HIP
events, the median of --reps calls after warm-up, of every entry point of csrc/spot.hip:
  - the range, the 256-bin histogram (each ends with its numbers on the host), the eroded threshold
    mask,
  - the labelling of three masks - that spot alone, a 50 % random field, one component that fills
    the frame - with the sizes and the largest component of each,
  - the take in its spot form and its row form,
  each beside its compulsory bytes - the frame, the mask or the label image read once, the mask or
  the label image written once -, the fraction of the 8 TB/s peak those reach, and a device-to-device
  copy of the same byte count in the same process;
  - vignettingFromSpotAverage on 16 such frames, device-resident and from host arrays, in both
    averageSpot forms, per frame.
Beside these, on this machine's host: the same routine composed from numpy and scipy (np.histogram
under the Otsu formula, scipy.ndimage.minimum_filter, label and center_of_mass) on the same 16
frames.  The condition: the device path is not slower.

    python tools/spot_bench.py [--reps 20] [--out profiles/spot_bench.json]
"""
import argparse
import contextlib
import ctypes as C
import io
import json
import os
import sys
import time

import numpy as np
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import imgprocessor_amd as ia  # noqa: E402
from imgprocessor_amd import DeviceArray, _lib as L, ops  # noqa: E402
from imgprocessor_amd.camera.flatField import vignettingFromSpotAverage  # noqa: E402

H, W = 2160, 3840
PEAK = 8.0e12
FRAMES = 16
SPOT = 30
DT_ID = {np.dtype(np.uint16): L.U16, np.dtype(np.float32): L.F32}


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


def frames_of(dtype, n, seed=0):
    """n frames of one noise field with a 30 x 30 spot at n positions left of column H (the row form
    of the routine reads the spot's column as a row)"""
    rng = np.random.default_rng(seed)
    base = 100.0 + 4.0 * rng.standard_normal((H, W))
    out = []
    for k in range(n):
        a = base.copy()
        r, c = int(rng.integers(0, H - SPOT)), int(rng.integers(0, H - SPOT))
        a[r:r + SPOT, c:c + SPOT] += 1000.0 - 300.0 * k / n
        out.append(np.round(a).astype(dtype) if np.dtype(dtype).kind == 'u' else a.astype(dtype))
    return out


def host_routine(images, bg):
    """vignettingFromSpotAverage(averageSpot=False) composed from numpy and scipy"""
    fitimg, mask, mx = None, None, 0
    for im in images:
        img = np.asarray(im, dtype=np.float64) - bg
        if fitimg is None:
            fitimg, mask = np.zeros_like(img), np.zeros(img.shape, bool)
        counts, e = np.histogram(img.ravel(), 256)
        counts = counts.astype(float)
        centers = (e[:-1] + e[1:]) / 2.
        w1, w2 = np.cumsum(counts), np.cumsum(counts[::-1])[::-1]
        m1 = np.cumsum(counts * centers) / w1
        m2 = (np.cumsum((counts * centers)[::-1]) / w2[::-1])[::-1]
        t = centers[np.argmax(w1[:-1] * w2[1:] * (m1[:-1] - m2[1:]) ** 2)]
        spots, n = ndimage.label(ndimage.minimum_filter(img > t, 3), np.ones((3, 3)))
        if n == 0:
            continue
        spot = spots == np.argmax(np.bincount(spots.ravel())[1:]) + 1
        mx2 = img[spot].mean()
        fitimg[spot] = img[spot]
        mask[spot] = 1
        mx = max(mx, mx2)
    fitimg /= mx
    return fitimg, mask


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

    def bench(fn, nbytes):
        return row(timed_ms(ctx, fn, args.reps), nbytes, copy_ms(nbytes))

    out = {}
    bg = 100.0
    for dtype in (np.uint16, np.float32):
        name = np.dtype(dtype).name
        img = frames_of(dtype, 1)[0]
        es = img.itemsize
        d = ctx.to_device(img)
        src = (ctx.handle, d.ptr, DT_ID[d.dtype], H, W, W, None, 0, bg)
        rng5, cnt = (C.c_double * 5)(), np.zeros(256, np.uint64)
        lib.ipa_spot_range_dev(*(src + (rng5,)))
        edges = np.linspace(rng5[0], rng5[1], 257)
        t = ops.otsu_threshold(d, bg=bg)
        d_mask = ctx.empty((H, W), np.uint8)
        r = {}
        r['range'] = bench(lambda: ctx._check(lib.ipa_spot_range_dev(*(src + (rng5,))), 'range'), px * es)
        r['histogram_256'] = bench(lambda: ctx._check(lib.ipa_spot_histogram_dev(*(src + (
            edges.ctypes.data_as(L._dp), 256, cnt.ctypes.data_as(C.c_void_p)))), 'histogram'), px * es)
        r['otsu_threshold'] = bench(lambda: ops.otsu_threshold(d, bg=bg), 2 * px * es)
        r['spot_mask'] = bench(lambda: ctx._check(lib.ipa_spot_mask_dev(*(src + (t, d_mask.ptr, W))), 'mask'),
                               px * es + px)
        spots, n = ops.label(d_mask)
        label = ops.largest_component(spots, n)[0]
        d_fit, d_valid, res = ctx.empty((H, W), np.float64), ctx.empty((H, W), np.uint8), (C.c_double * 3)()
        r['take_spot'] = bench(lambda: ctx._check(lib.ipa_spot_take_dev(*(src + (
            spots.ptr, W, label, 0, 0, d_fit.ptr, W, d_valid.ptr, W, res))), 'take'), 4 * px)
        r['take_rows'] = bench(lambda: ctx._check(lib.ipa_spot_take_dev(*(src + (
            None, 0, 0, 7, 900, d_fit.ptr, W, d_valid.ptr, W, res))), 'take'), 2 * W * (es + 9))
        out[name] = r
        if dtype == np.uint16:
            spot_mask = d_mask.get()

    rng = np.random.default_rng(5)
    masks = {'one_spot': spot_mask, 'random_50': (rng.random((H, W)) < 0.5).astype(np.uint8),
             'frame_filling': np.ones((H, W), np.uint8)}
    out['label'] = {}
    for name, m in masks.items():
        d_m = ctx.to_device(m)
        d_labels = DeviceArray.counts(ctx, (H, W))
        n, big = C.c_int(), (C.c_longlong * 4)()

        def lab():
            ctx._check(lib.ipa_label_dev(ctx.handle, d_m.ptr, H, W, W, 2, d_labels.ptr, W, C.byref(n)), 'label')

        r = {'label': bench(lab, 5 * px)}
        d_sizes = DeviceArray._wrap(ctx, ctx._alloc(max(n.value, 1) * 8), (max(n.value, 1),), np.int64, True)
        r['sizes'] = bench(lambda: ctx._check(lib.ipa_label_sizes_dev(
            ctx.handle, d_labels.ptr, H, W, W, n.value, d_sizes.ptr), 'sizes'), 4 * px)
        r['largest'] = bench(lambda: ctx._check(lib.ipa_label_largest_dev(
            ctx.handle, d_labels.ptr, H, W, W, n.value, big), 'largest'), 4 * px)
        r['n'], r['largest_size'] = n.value, int(big[1])
        t0 = time.perf_counter()
        want, n_want = ndimage.label(m, np.ones((3, 3)))
        r['scipy_label_ms'] = round((time.perf_counter() - t0) * 1e3, 2)
        r['equals_scipy'] = bool(n.value == n_want and np.array_equal(d_labels.get(), want))
        out['label'][name] = r

    # the whole routine, 16 frames
    out['routine'] = {}
    quiet = io.StringIO()
    for dtype in (np.uint16, np.float32):
        name = np.dtype(dtype).name
        images = frames_of(dtype, FRAMES, 1)
        d_stack = ctx.to_device(np.stack(images))
        r = {}
        with contextlib.redirect_stdout(quiet):
            for avg in (False, True):
                key = 'averageSpot_%s' % avg
                reps = max(3, args.reps // 4)
                ms = timed_ms(ctx, lambda: vignettingFromSpotAverage(d_stack, bg, averageSpot=avg), reps, warm=1)
                r[key + '_device_frames_ms_per_frame'] = round(ms[0] / FRAMES, 3)
                r[key + '_vs_frame_d2d_copy'] = round(ms[0] / FRAMES / copy_ms(2 * px * images[0].itemsize), 2)
                t0 = time.perf_counter()
                dev_fit, dev_mask = vignettingFromSpotAverage(images, bg, averageSpot=avg)
                r[key + '_host_frames_ms_per_frame'] = round((time.perf_counter() - t0) * 1e3 / FRAMES, 3)
                if not avg:
                    fit, mask = dev_fit, dev_mask
        t0 = time.perf_counter()
        host_fit, host_mask = host_routine(images, bg)
        r['numpy_scipy_host_ms_per_frame'] = round((time.perf_counter() - t0) * 1e3 / FRAMES, 3)
        r['speedup_device_frames'] = round(r['numpy_scipy_host_ms_per_frame'] /
                                           r['averageSpot_False_device_frames_ms_per_frame'], 1)
        r['speedup_host_frames'] = round(r['numpy_scipy_host_ms_per_frame'] /
                                         r['averageSpot_False_host_frames_ms_per_frame'], 1)
        r['mask_equals_host'] = bool(np.array_equal(mask, host_mask))
        with np.errstate(invalid='ignore'):
            r['fitimg_max_rel_difference'] = float('%.3g' % np.nanmax(np.abs(fit - host_fit)[host_mask] /
                                                                         np.abs(host_fit[host_mask])))
        out['routine'][name] = r

    info = ctx.device_info()
    line = json.dumps(dict({'metric': 'spot_4k', 'device': info.get('name'), 'shape': [H, W], 'frames': FRAMES,
                            'reps': args.reps}, **out))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fo:
            fo.write(line + '\n')


if __name__ == '__main__':
    main()
