"""Non-local means as scikit-image 0.18 computes it (skimage.restoration.denoise_nl_means,
fast_mode=True, 2-D), restated in numpy: the yardstick of ops.nl_means.

With s = patch_size (an even s becomes s + 1), o = s // 2, d = patch_distance:
  P        the image padded by o + d + 1 with numpy `reflect` (no edge repeat)
  D(p, t)  max(sum_q ((P[q] - P[q + t])**2 - 2 sigma**2) / (s**2 h**2), 0) for t in [-d, d]**2,
           q over the (s - 1) x (s - 1) window at offsets -o + 1 ... +o from p in both axes
  w(p, t)  exp(-D), 0 where D > 5 (strict), 2 exp(-0) for t == (0, 0)
  out[p]   sum_t w P[p + t] / sum_t w
`exp` may be replaced (skimage 0.18 uses its own fast_exp, +-3 %); `dtype` is the arithmetic the
whole evaluation runs in (float64: the yardstick).
"""
import numpy as np

CUTOFF = 5.0


def nlm_ref(img, patch_size=7, patch_distance=11, h=0.1, sigma=0.0, exp=np.exp, dtype=np.float64):
    """-> (out, margin): the denoised image and, per pixel, min over t != 0 of |D(p, t) - 5|
    (how far the pixel is from a weight switching between exp(-5) and 0)"""
    dtype = np.dtype(dtype).type
    img = np.asarray(img)
    if img.ndim != 2 or min(img.shape) < 2:
        raise ValueError('nlm_ref takes a 2-D image of at least 2 x 2 pixels')
    s = int(patch_size) + (1 - int(patch_size) % 2)
    o, d = s // 2, int(patch_distance)
    pad = o + d + 1
    P = np.pad(img.astype(dtype), pad, mode='reflect')
    H, W = img.shape
    scale = dtype(s * s) * dtype(h) * dtype(h)
    two_sig = dtype(2.0) * dtype(sigma) * dtype(sigma)
    num = np.zeros((H, W), dtype)
    den = np.zeros((H, W), dtype)
    margin = np.full((H, W), np.inf)
    # rows / columns of P the windows of all pixels cover: offsets -o + 1 ... +o
    r0, r1 = pad - o + 1, pad + H + o
    c0, c1 = pad - o + 1, pad + W + o
    n = s - 1
    for tr in range(-d, d + 1):
        for tc in range(-d, d + 1):
            if tr == 0 and tc == 0:
                # the self pair is added twice, through the same exp as every other pair
                w = np.full((H, W), 2, dtype) * exp(-np.zeros((H, W), dtype)).astype(dtype)
            else:
                q = (P[r0:r1, c0:c1] - P[r0 + tr:r1 + tr, c0 + tc:c1 + tc]) ** 2 - two_sig
                box = np.zeros((H, W), dtype)
                for i in range(n):
                    for j in range(n):
                        box += q[i:i + H, j:j + W]
                D = np.maximum(box / scale, dtype(0))
                margin = np.minimum(margin, np.abs(D.astype(np.float64) - CUTOFF))
                w = np.where(D > dtype(CUTOFF), dtype(0), exp(-D).astype(dtype))
            num += w * P[pad + tr:pad + tr + H, pad + tc:pad + tc + W]
            den += w
    return num / den, margin
