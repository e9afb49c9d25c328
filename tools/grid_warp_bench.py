#!/usr/bin/env python3
"""Time PerspectiveCorrection.correctGrid's one launch (ops.warp_grid) against the same cells done
the reference's way, one ops.warp_perspective call per cell, and write profiles/grid_warp_bench.json.

3840 x 2160 frames, float32 and uint16, a mildly bent 7 x 11-point lattice (6 x 10 cells, border 0),
Lanczos4 and bilinear, batches of 1 and 16; everything device-resident, outputs preallocated.
hipEvent-timed around the call (the loop: around all 60 calls, so the gaps between its small
launches count, as they do for a caller), WARMUP warm-ups, median of RUNS.  The loop leaves out the
pastes into one output array, which favours it.  ratio = loop / one launch: above 1 the one launch
is faster.

    python tools/grid_warp_bench.py [--runs 20] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 2160, 3840
N0, N1 = 6, 10


def bent_lattice():
    """(7, 11, 2) points (x, y) over the frame, bowed by up to 6 px"""
    gx, gy = np.meshgrid(np.linspace(40, W - 41, N0 + 1), np.linspace(30, H - 31, N1 + 1), indexing='ij')
    u, v = gx / W, gy / H
    return np.stack([gx + 6 * np.sin(np.pi * v), gy + 4 * np.sin(np.pi * u) * np.cos(np.pi * v)], axis=-1)


def timed_pair(ctx, fa, fb, warmup, runs):
    """the two alternated, so that whatever else the machine does meets both alike"""
    for _ in range(warmup):
        fa()
        fb()
    ms = ([], [])
    for _ in range(runs):
        for fn, m in zip((fa, fb), ms):
            e0 = ctx.event().record()
            fn()
            e1 = ctx.event().record()
            m.append(e0.elapsed_ms(e1))
    return [(float(np.median(m)), float(min(m)), float(max(m))) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'grid_warp_bench.json'))
    a = ap.parse_args()
    import imgprocessor_amd as ia
    from imgprocessor_amd import ops
    from imgprocessor_amd.camera.PerspectiveCorrection import PerspectiveCorrection
    ctx = ia.default_context(0)
    rng = np.random.default_rng(0)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.clip(0.5 + 0.25 * np.sin(x / 15) + 0.25 * np.cos(y / 10) +
                  0.05 * rng.standard_normal((H, W)), 0, 1).astype(np.float32)
    rects, M = PerspectiveCorrection((H, W), new_size=(W, H), border=0)._gridCells(bent_lattice())
    col, row, owner = ops.warp_grid_plan(rects, (H, W))
    own = owner[row.astype(np.intp)[:, None], col.astype(np.intp)[None, :]]   # per pixel, for the comparison only
    res = {'device': ctx.device_info()['name'], 'frame': [H, W], 'cells': [N0, N1], 'n_cells': len(rects),
           'runs': a.runs, 'warmup': a.warmup, 'ratio': 'loop_ms / grid_ms', 'cases': []}
    for dtype in (np.float32, np.uint16):
        frame = img if dtype == np.float32 else np.round(img * 65535).astype(np.uint16)
        for n in (1, 16):
            src = frame if n == 1 else np.stack([np.roll(frame, 7 * i, axis=1) for i in range(n)])
            d_src = ctx.to_device(src)
            lead = () if n == 1 else (n,)
            d_out = ctx.empty(lead + (H, W), dtype)
            d_cells = [ctx.empty(lead + (int(r[3]), int(r[2])), dtype) for r in rects]
            for interp in ('lanczos4', 'linear'):
                def grid():
                    ops.warp_grid(d_src, rects, M, (H, W), interp, out=d_out)

                def loop():
                    for r, m, o in zip(rects, M, d_cells):
                        ops.warp_perspective(d_src, m, (int(r[3]), int(r[2])), interp, out=o)
                g, l = timed_pair(ctx, grid, loop, a.warmup, a.runs)
                # the two must agree bit for bit at the size timed (first frame; every cell where it owns the pixel)
                got = d_out.get().reshape(-1, H, W)[0]
                same = all(np.array_equal(got[y0:y0 + h, x0:x0 + w][own[y0:y0 + h, x0:x0 + w] == i],
                                          o.get().reshape(-1, h, w)[0][own[y0:y0 + h, x0:x0 + w] == i])
                           for i, ((x0, y0, w, h), o) in enumerate(zip(rects.tolist(), d_cells)))
                case = {'dtype': np.dtype(dtype).name, 'frames': n, 'interpolation': interp,
                        'grid_ms_median': round(g[0], 4), 'grid_ms_min': round(g[1], 4),
                        'grid_ms_max': round(g[2], 4), 'loop_ms_median': round(l[0], 4),
                        'loop_ms_min': round(l[1], 4), 'loop_ms_max': round(l[2], 4),
                        'ratio': round(l[0] / g[0], 3), 'identical': bool(same)}
                res['cases'].append(case)
                print(json.dumps(case), flush=True)
            del d_src, d_out, d_cells
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
