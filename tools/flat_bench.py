#!/usr/bin/env python3
"""Flat field calibration on device-resident 4K frames: one JSON line.

For 16 frames of 3840 x 2160, uint16 and float32, it times - a host clock around --inner calls that
end in one synchronise, Python included, per call; the median of --reps such windows after warm-up,
the variants of a comparison alternating -
  - sensitivity() through the fused kernels (ops.sens_shrink, ops.sens_accumulate);
  - the same result through the ops that were there before: ops.nlf_signal(frame, bg) -> fastMean
    (INTER_AREA down, INTER_LINEAR up) on the device, then - no op divides or adds two frames -
    the smooth frame and the frame brought down and `(frame - bg) / smooth` summed in numpy (a
    third of a second a call: 3 windows of one call each, `composed_reps`).  Its
    device part alone (nlf_signal and fastMean for the 16 frames, nothing else) is timed too: a
    lower bound of any composition.  The results are compared, bit for bit, before anything is
    timed;
  - ipa_memcpy_d2d of the compulsory bytes of the fused form per frame (the frame read twice, the
    accumulator read and written), the copy moving every byte twice (tools/nlf_bench.py's
    convention);
  - imgAverage of the 16 frames (compared with numpy's sum first), and flatFieldFromCloseDistance2
    end to end (3 windows of one call) with the share of its noise level function estimate
    (oneImageNLF on the two brightest frames).

The process is one sample: run it three times (fresh processes) and keep every line.

    python tools/flat_bench.py [--reps 7] [--inner 10] [--out profiles/flat_bench.json] [--append]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import imgprocessor_amd as ia  # noqa: E402
from imgprocessor_amd import ops  # noqa: E402
from imgprocessor_amd.camera.NoiseLevelFunction import oneImageNLF  # noqa: E402
from imgprocessor_amd.camera.flatField import flatFieldFromCloseDistance2, sensitivity  # noqa: E402
from imgprocessor_amd.filters.fastMean import fastMean  # noqa: E402
from imgprocessor_amd.transform import imgAverage  # noqa: E402

H, W, N = 2160, 3840, 16
BG = 400.0


def frames_of(dtype, rng):
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    field = 400.0 + 30000.0 * (1.0 - 1.3 * (((x - W / 2) / W) ** 2 + ((y - H / 2) / H) ** 2))
    out = []
    for k in range(N):
        f = field * (1.0 - 0.002 * k) + np.sqrt(field) * rng.standard_normal((H, W), dtype=np.float32)
        out.append(np.round(f).astype(dtype) if np.dtype(dtype).kind == 'u' else f.astype(dtype))
    return np.stack(out)


COMPOSED_REPS = 3


def wall_ms(ctx, fn, inner=1):
    """milliseconds per call of `inner` back-to-back calls that end in one synchronise"""
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        out = fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--out', default=None)
    ap.add_argument('--append', action='store_true')
    args = ap.parse_args()
    ctx = ia.default_context(0)
    rng = np.random.default_rng(0)
    rows = []
    for dtype in (np.uint16, np.float32):
        stack = ctx.to_device(frames_of(dtype, rng))
        es = np.dtype(dtype).itemsize

        def fused():
            return sensitivity(stack, BG, 10)

        def device_part():
            for k in range(N):
                fastMean(ops.nlf_signal(stack.frame(k), bg=BG), 10)

        def composition():
            out = None
            for k in range(N):
                smooth = fastMean(ops.nlf_signal(stack.frame(k), bg=BG), 10).get()
                q = (stack.frame(k).get().astype(np.float64) - BG) / smooth
                out = q if out is None else out + q
            return out / N

        equal = bool(np.array_equal(fused().get(), composition(), equal_nan=True))
        device_part()
        # alternate the variants
        tf, tc, tp = [], [], []
        for _ in range(args.reps):
            tf.append(wall_ms(ctx, fused, args.inner)[0])
            tp.append(wall_ms(ctx, device_part, args.inner)[0])
            if len(tc) < COMPOSED_REPS:
                tc.append(wall_ms(ctx, composition)[0])
        nbytes = N * (2 * es + 16) * H * W
        src, dst = ctx.empty((nbytes // N,), np.uint8), ctx.empty((nbytes // N,), np.uint8)

        def copy():
            for _ in range(N):
                dst.copy_from(src)
        copy()
        tm = [wall_ms(ctx, copy, args.inner)[0] for _ in range(args.reps)]
        del src, dst
        want = np.zeros((H, W))
        for f in stack.get():
            want += f
        mean_equal = bool(np.array_equal(imgAverage(stack).get(), want / N, equal_nan=True))
        ta = [wall_ms(ctx, lambda: imgAverage(stack), args.inner)[0] for _ in range(args.reps)]
        rows.append({'dtype': np.dtype(dtype).name,
                     'sensitivity_fused_ms': round(float(np.median(tf)), 3),
                     'sensitivity_fused_ms_min_max': [round(min(tf), 3), round(max(tf), 3)],
                     'sensitivity_composed_ms': round(float(np.median(tc)), 3),
                     'sensitivity_composed_ms_min_max': [round(min(tc), 3), round(max(tc), 3)],
                     'composed_reps': COMPOSED_REPS,
                     'composed_over_fused': round(float(np.median(tc) / np.median(tf)), 3),
                     'composed_device_part_ms': round(float(np.median(tp)), 3),
                     'composed_device_part_ms_min_max': [round(min(tp), 3), round(max(tp), 3)],
                     'device_part_over_fused': round(float(np.median(tp) / np.median(tf)), 3),
                     'results_equal': equal,
                     'compulsory_bytes': int(nbytes),
                     'd2d_copy_ms': round(float(np.median(tm)), 3),
                     'fused_over_d2d': round(float(np.median(tf) / np.median(tm)), 3),
                     'imgAverage_equal': mean_equal,
                     'imgAverage_ms': round(float(np.median(ta)), 3),
                     'imgAverage_bytes': int((N * es + 8) * H * W)})
        if np.dtype(dtype) == np.uint16:
            bgs = ctx.to_device(np.full((3, H, W), int(BG), np.uint16))
            flatFieldFromCloseDistance2(stack, bgs)
            tw = [wall_ms(ctx, lambda: flatFieldFromCloseDistance2(stack, bgs))[0] for _ in range(3)]
            i0 = ops.flat_scale(imgAverage([stack.frame(0)]), bg=BG)
            i1 = ops.flat_scale(imgAverage([stack.frame(1)]), bg=BG)
            tn = [wall_ms(ctx, lambda: oneImageNLF(i0, i1))[0] for _ in range(3)]
            rows[-1]['flatFieldFromCloseDistance2_ms'] = round(float(np.median(tw)), 3)
            rows[-1]['oneImageNLF_ms'] = round(float(np.median(tn)), 3)
            rows[-1]['nlf_share'] = round(float(np.median(tn) / np.median(tw)), 3)
            del bgs, i0, i1
        del stack
        ctx.trim()
    info = ctx.device_info()
    line = json.dumps({'metric': 'flat_field_4k', 'device': info.get('name'), 'shape': [H, W], 'frames': N,
                       'reps': args.reps, 'inner': args.inner, 'pid': os.getpid(), 'rows': rows})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a' if args.append else 'w') as fo:
            fo.write(line + '\n')


if __name__ == '__main__':
    main()
