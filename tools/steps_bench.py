#!/usr/bin/env python3
"""The flat field from discrete steps on 4K frames on the device: one JSON line.

On device-resident 2160 x 3840 frames of a 4 x 5-cell device on a raster of 300 x 350-pixel cells (a
grid of 8 x 11 cells that starts at pixel (10, 20)) it times, with HIP events, the median of --reps
calls after warm-up, of
  - cell_means on 16 and 64 uint16 and float32 frames, without and with a float32 background frame,
    beside its compulsory bytes - every frame read once, the background once -, the fraction of the
    8 TB/s peak those reach, and a device-to-device copy of the same byte count in the same process;
  - steps_separate for a 64 x 8 x 12 grid (random cell means, a 4 x 5 device, run to the cap of
    max_iter = 100: 102 iterations) and for the raster's own grid;
  - vignettingFromDiscreteSteps from 64 device-resident uint16 frames, 'POLY replace' and 'POLY repair'.
Beside these, on this machine's host: the reference's method restated in numpy (a Python loop over
the cells of every frame, then the loop of nanmeans) on the same 16 and 64 uint16 frames.

    python tools/steps_bench.py [--reps 20] [--out profiles/steps_bench.json]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import imgprocessor_amd as ia  # noqa: E402
from imgprocessor_amd import ops  # noqa: E402
from imgprocessor_amd.ops_steps import device_grid_slices  # noqa: E402
from imgprocessor_amd.camera.flatField import (positionsFromRaster, vignettingFromDiscreteSteps)  # noqa: E402

H, W = 2160, 3840
PEAK = 8.0e12
D0, D1 = 300, 350
N0, N1 = 4, 5
ORIGIN = (10, 20)


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


def scene(n):
    """-> (positions, uint16 frames (n, H, W)): the device at the first n positions of a 9-wide raster
    that starts one cell above / left of the grid"""
    positions = positionsFromRaster((-1, -1), n, 9, (D1, D0), (ORIGIN[1] - D1, ORIGIN[0] - D0), 1, 1)
    g0, g1 = int(H / D0) + 1, int(W / D1) + 1
    re, ce = ops.cell_edges(H, g0, D0, ORIGIN[0]), ops.cell_edges(W, g1, D1, ORIGIN[1])
    rng = np.random.default_rng(0)
    obj = 0.6 + 0.4 * rng.random((N0, N1))
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    V = (3000.0 / (1.0 + 1.5 * (((y - 0.45 * H) / H) ** 2 + ((x - 0.55 * W) / W) ** 2))).astype(np.float32)
    frames = np.empty((n, H, W), np.uint16)
    for k, (p0, p1) in enumerate(positions[1]):
        f = np.zeros((H, W), np.float32)
        for a in range(N0):
            for b in range(N1):
                i, j = p0 + a, p1 + b
                if 0 <= i < g0 and 0 <= j < g1:
                    f[re[i]:re[i + 1], ce[j]:ce[j + 1]] = obj[a, b]
        frames[k] = f * V + 100.0
    return positions, frames


def host_routine(frames, positions, bg_value):
    """the reference's method in numpy -> (ff, avgobj, seconds of the cell pass, seconds of the loop)"""
    n = len(frames)
    g0, g1 = int(H / D0) + 1, int(W / D1) + 1
    re, ce = ops.cell_edges(H, g0, D0, ORIGIN[0]), ops.cell_edges(W, g1, D1, ORIGIN[1])
    t0 = time.perf_counter()
    grid = np.full((n, g0, g1), np.nan)
    for k in range(n):
        img = frames[k].astype(float)
        for i in range(g0):
            for j in range(g1):
                c = img[re[i]:re[i + 1], ce[j]:ce[j + 1]]
                ind = c > bg_value
                if c.size and not ind.sum() < 0.5 * ind.size:
                    grid[k, i, j] = c[ind].mean()
    t1 = time.perf_counter()
    rects = device_grid_slices((N0, N1), (g0, g1), positions[1])
    devices = np.full((n, N0, N1), np.nan)
    for k, (q0, q1, qq0, qq1, l0, l1) in enumerate(rects):
        devices[k, q0:q0 + l0, q1:q1 + l1] = grid[k, qq0:qq0 + l0, qq1:qq1 + l1]
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        ff = np.nanmean(grid, axis=0) - bg_value
        ff /= np.nanmax(ff)
        ffs, obj = np.full_like(grid, np.nan), np.full_like(devices, np.nan)
        for it in range(1, 103):
            for k, (q0, q1, qq0, qq1, l0, l1) in enumerate(rects):
                obj[k, q0:q0 + l0, q1:q1 + l1] = devices[k, q0:q0 + l0, q1:q1 + l1] / ff[qq0:qq0 + l0, qq1:qq1 + l1]
            avgobj = np.nanmean(obj, axis=0)
            for k, (q0, q1, qq0, qq1, l0, l1) in enumerate(rects):
                ffs[k, qq0:qq0 + l0, qq1:qq1 + l1] = devices[k, q0:q0 + l0, q1:q1 + l1] / avgobj[q0:q0 + l0, q1:q1 + l1]
            ff2 = np.nanmean(ffs, axis=0)
            dev = np.nanmean((ff - ff2) ** 2) ** 0.5
            ff = ff2
            if dev < 1e-6:
                break
    return ff, avgobj, it, t1 - t0, time.perf_counter() - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    ctx = ia.default_context(0)
    px = H * W
    copies = {}

    def copy_ms(nbytes):
        """a device-to-device copy moves nbytes / 2 in and nbytes / 2 out"""
        if nbytes not in copies:
            src, dst = ctx.empty((nbytes // 2,), np.uint8), ctx.empty((nbytes // 2,), np.uint8)
            copies[nbytes] = timed_ms(ctx, lambda: dst.copy_from(src), args.reps)[0]
            src.free()
            dst.free()
        return copies[nbytes]

    def row(ms, nbytes):
        c = copy_ms(nbytes)
        return {'ms': round(ms[0], 4), 'ms_min_max': [round(ms[1], 4), round(ms[2], 4)], 'compulsory_bytes': int(nbytes),
                'peak_fraction': round(nbytes / (ms[0] * 1e-3) / PEAK, 4), 'd2d_copy_ms': round(c, 4),
                'vs_d2d': round(ms[0] / c, 3)}

    bg_value = 300.0
    positions, frames = scene(64)
    g0, g1 = int(H / D0) + 1, int(W / D1) + 1
    re, ce = ops.cell_edges(H, g0, D0, ORIGIN[0]), ops.cell_edges(W, g1, D1, ORIGIN[1])
    rng = np.random.default_rng(1)
    d_bg = ctx.to_device((20.0 * rng.random((H, W))).astype(np.float32))
    out = {'cell_means': {}, 'grid': [g0, g1], 'cell': [D0, D1]}
    d_u16 = ctx.to_device(frames)
    for dtype in (np.uint16, np.float32):
        name = np.dtype(dtype).name
        d_all = d_u16 if dtype == np.uint16 else ctx.to_device(frames.astype(np.float32))
        es = d_all.dtype.itemsize
        for n in (16, 64):
            d = ia.DeviceArray._wrap(ctx, d_all.ptr, (n, H, W), d_all.dtype, False, base=d_all)
            out['cell_means']['%s_%d' % (name, n)] = row(
                timed_ms(ctx, lambda: ops.cell_means(d, re, ce, bg_value), args.reps), n * px * es)
            out['cell_means']['%s_%d_bg' % (name, n)] = row(
                timed_ms(ctx, lambda: ops.cell_means(d, re, ce, bg_value, bg=d_bg), args.reps), n * px * es + px * 4)
        if dtype != np.uint16:
            d_all.free()

    # the loop
    grid = ops.cell_means(d_u16, re, ce, bg_value)
    sep = {}
    rnd = ctx.to_device(0.5 + rng.random((64, 8, 12)))
    res = ops.steps_separate(rnd, (N0, N1), positions[1], bg_value=0.0, max_iter=100, max_dev=0.0)
    ms = timed_ms(ctx, lambda: ops.steps_separate(rnd, (N0, N1), positions[1], bg_value=0.0, max_iter=100, max_dev=0.0),
                  args.reps)
    sep['random_64x8x12_to_the_cap'] = {'ms': round(ms[0], 4), 'ms_min_max': [round(ms[1], 4), round(ms[2], 4)],
                                        'iterations': res[3], 'us_per_iteration': round(ms[0] * 1e3 / res[3], 2)}
    res = ops.steps_separate(grid, (N0, N1), positions[1], bg_value=bg_value)
    ms = timed_ms(ctx, lambda: ops.steps_separate(grid, (N0, N1), positions[1], bg_value=bg_value), args.reps)
    sep['raster_64x%dx%d' % (g0, g1)] = {'ms': round(ms[0], 4), 'ms_min_max': [round(ms[1], 4), round(ms[2], 4)],
                                         'iterations': res[3], 'last_dev': float('%.3g' % res[4])}
    out['steps_separate'] = sep

    # the whole routine, 64 uint16 frames on the device
    rt = {}
    for method in ('POLY replace', 'POLY repair'):
        def call():
            return vignettingFromDiscreteSteps(d_u16, (N1, N0), positions, bg_value=bg_value,
                                               postprocessing_method=method)
        ms = timed_ms(ctx, call, max(3, args.reps // 4), warm=1)
        rt[method.replace(' ', '_') + '_ms'] = round(ms[0], 3)
        rt[method.replace(' ', '_') + '_vs_frames_d2d_copy'] = round(ms[0] / copy_ms(64 * px * 2), 3)
    dev_ff, _, dev_obj, _ = vignettingFromDiscreteSteps(d_u16, (N1, N0), positions, bg_value=bg_value)
    for n in (16, 64):
        pos_n = (positions[0], positions[1][:n], positions[2])
        ff, avgobj, it, t_cells, t_loop = host_routine(frames[:n], pos_n, bg_value)
        rt['numpy_host_%d_frames' % n] = {'cells_ms': round(t_cells * 1e3, 1), 'loop_ms': round(t_loop * 1e3, 2),
                                          'iterations': it}
    with np.errstate(invalid='ignore'):
        rt['ff_max_rel_difference_from_host'] = float('%.3g' % np.nanmax(np.abs(dev_ff.get() - ff) / np.abs(ff)))
        rt['avgobj_max_rel_difference_from_host'] = float('%.3g' % np.nanmax(np.abs(dev_obj.get() - avgobj) / np.abs(avgobj)))
    rt['speedup_cells_64_uint16'] = round(rt['numpy_host_64_frames']['cells_ms'] / out['cell_means']['uint16_64']['ms'], 1)
    rt['speedup_routine_64_uint16'] = round((rt['numpy_host_64_frames']['cells_ms'] + rt['numpy_host_64_frames']['loop_ms'])
                                            / rt['POLY_replace_ms'], 1)
    out['routine'] = rt

    info = ctx.device_info()
    line = json.dumps(dict({'metric': 'steps_4k', 'device': info.get('name'), 'shape': [H, W], 'reps': args.reps}, **out))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fo:
            fo.write(line + '\n')


if __name__ == '__main__':
    main()
