#!/usr/bin/env python3
"""Time ops.nl_means on one 3840 x 2160 float32 frame (hipEvent-timed, median of RUNS launches
after warm-up) at (patch_size, patch_distance) = (7, 11), (3, 11), (7, 5) and write
profiles/nlm_bench.json: milliseconds, pixel-shift pairs per second, counted vector flops against
the fp32 vector peak, and time(s=7) / time(s=3) - far below the patch-area ratio 36 / 4 when the
box sum is shared.  --skimage-ms-512 takes scikit-image's time for a 512 x 512 crop (measured
elsewhere, where skimage is installed); it is scaled by area and labelled as scaled.

    python tools/nlm_bench.py [--runs 10] [--skimage-ms-512 MS]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 2160, 3840
PEAK_FP32_VECTOR_TFLOPS = 157.3   # MI355X: 256 CUs x 128 lanes x 2 (FMA) x 2.4 GHz


def flops_per_pair(s):
    """counted vector operations per pixel-shift pair of csrc/nlm.hip: difference, square, s - 2
    lane-shift additions, s - 2 ring additions, distance (2), clamp, cut-off, exp (2), self
    select, weight sum, neighbour difference and fma (2 flops)"""
    return 2 + (s - 2) + (s - 2) + 2 + 1 + 1 + 2 + 1 + 1 + 1 + 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--skimage-ms-512', type=float, default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'nlm_bench.json'))
    a = ap.parse_args()
    import imgprocessor_amd as ia
    from imgprocessor_amd import ops
    ctx = ia.default_context(0)
    rng = np.random.default_rng(0)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.clip(0.5 + 0.25 * np.sin(x / 15) + 0.25 * np.cos(y / 10) +
                  0.05 * rng.standard_normal((H, W)), 0, 1).astype(np.float32)
    d_img, d_out = ctx.to_device(img), ctx.empty((H, W), np.float32)
    res = {'device': ctx.device_info()['name'], 'frame': [H, W], 'dtype': 'float32', 'h': 0.1,
           'runs': a.runs, 'warmup': a.warmup, 'cases': []}
    for s, d in ((7, 11), (3, 11), (7, 5)):
        for _ in range(a.warmup):
            ops.nl_means(d_img, s, d, 0.1, out=d_out)
        ms = []
        for _ in range(a.runs):
            e0, e1 = ctx.event().record(), None
            ops.nl_means(d_img, s, d, 0.1, out=d_out)
            e1 = ctx.event().record()
            ms.append(e0.elapsed_ms(e1))
        t = float(np.median(ms))
        pairs = H * W * (2 * d + 1) ** 2
        case = {'patch_size': s, 'patch_distance': d, 'ms_median': round(t, 3),
                'ms_min': round(min(ms), 3), 'ms_max': round(max(ms), 3),
                'pairs_per_s': pairs / (t * 1e-3),
                'counted_flops_per_pair': flops_per_pair(s),
                'fraction_of_fp32_vector_peak': round(pairs * flops_per_pair(s) / (t * 1e-3) /
                                                      (PEAK_FP32_VECTOR_TFLOPS * 1e12), 4)}
        res['cases'].append(case)
        print(json.dumps(case))
    by = {(c['patch_size'], c['patch_distance']): c['ms_median'] for c in res['cases']}
    res['time_s7_over_s3'] = round(by[(7, 11)] / by[(3, 11)], 3)
    res['patch_area_ratio'] = 9.0
    if a.skimage_ms_512 is not None:
        res['skimage_cpu'] = {'measured_ms_512x512_s7_d11': a.skimage_ms_512,
                              'scaled_by_area_to_frame_ms': a.skimage_ms_512 * H * W / 512.0 ** 2,
                              'note': 'scikit-image 0.18.3, one CPU thread, 512 x 512 crop, SCALED by area'}
    print(json.dumps({k: v for k, v in res.items() if k != 'cases'}))
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
