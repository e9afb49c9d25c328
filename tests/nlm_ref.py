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


VARIANTS = ('window', 'sigma_s2', 'self1', 'ge', 'symmetric')


def nlm_ref(img, patch_size=7, patch_distance=11, h=0.1, sigma=0.0, exp=np.exp, dtype=np.float64,
            variant=None):
    """-> (out, margin): the denoised image and, per pixel, min over t != 0 of |D(p, t) - 5|
    (how far the pixel is from a weight switching between exp(-5) and 0).
    `variant` names a wrong version, for the sensitivity test of test_cpu_nlm.py: the window at
    offsets -o ... o - 1, s**2 for (s - 1)**2 in the sigma term, a self weight of 1, `>=` at the
    cut-off, `symmetric` padding."""
    dtype = np.dtype(dtype).type
    img = np.asarray(img)
    if img.ndim != 2 or min(img.shape) < 2:
        raise ValueError('nlm_ref takes a 2-D image of at least 2 x 2 pixels')
    s = int(patch_size) + (1 - int(patch_size) % 2)
    o, d = s // 2, int(patch_distance)
    pad = o + d + 1
    P = np.pad(img.astype(dtype), pad, mode='symmetric' if variant == 'symmetric' else 'reflect')
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
    if variant == 'window':
        r0, r1, c0, c1 = r0 - 1, r1 - 1, c0 - 1, c1 - 1
    if variant == 'sigma_s2':
        two_sig = two_sig * dtype(s * s) / dtype(n * n)
    for tr in range(-d, d + 1):
        for tc in range(-d, d + 1):
            if tr == 0 and tc == 0:
                # the self pair is added twice, through the same exp as every other pair
                w = np.full((H, W), 1 if variant == 'self1' else 2, dtype) * exp(-np.zeros((H, W), dtype)).astype(dtype)
            else:
                q = (P[r0:r1, c0:c1] - P[r0 + tr:r1 + tr, c0 + tc:c1 + tc]) ** 2 - two_sig
                box = np.zeros((H, W), dtype)
                for i in range(n):
                    for j in range(n):
                        box += q[i:i + H, j:j + W]
                D = np.maximum(box / scale, dtype(0))
                margin = np.minimum(margin, np.abs(D.astype(np.float64) - CUTOFF))
                cut = D >= dtype(CUTOFF) if variant == 'ge' else D > dtype(CUTOFF)
                w = np.where(cut, dtype(0), exp(-D).astype(dtype))
            num += w * P[pad + tr:pad + tr + H, pad + tc:pad + tc + W]
            den += w
    return num / den, margin


# ------------------------------------------------------------------ the geometry table ----
WAVES, ROWS = 4, {'float32': 16, 'float64': 8}     # nlm_kernel: output rows per wave
GEO_SIZES = (2, 3, 4, 5, 8, 9, 10, 11)             # 6 and 7 have test_geometry of test_gpu_nlm.py
GEO_D, GEO_H, GEO_SIGMAS = 2, 0.1, (0.0, 0.03)


def instantiation(patch_size):
    """-> (W, TX): nlm_kernel<T, W> of a patch size and its output tile's columns 65 - W"""
    w = (int(patch_size) | 1) - 1
    return w, 65 - w


def geo_shapes(patch_size):
    """frames one past the 32-row tile and one column past the column tile, one past the 64-row
    tile at exactly one column tile, and 64 rows over two column tiles and one column"""
    tx = instantiation(patch_size)[1]
    return (33, tx + 1), (65, tx), (64, 2 * tx + 1)


def workgroups(patch_size, shape, dtype):
    """-> (in x, in y) of ipa_nl_means_dev's launch"""
    tx, ty = instantiation(patch_size)[1], WAVES * ROWS[np.dtype(dtype).name]
    return -(-shape[1] // tx), -(-shape[0] // ty)


def knife_image(shape=(24, 30), seed=3):
    """values 0 and 4: with patch_size 5 and h = 0.8 every distance is an integer multiple of
    16 / (25 * 0.64) = 1, exact in float32 and float64, and many equal the cut-off 5 exactly"""
    return (np.random.default_rng(seed).random(shape) < 0.5) * 4.0


KNIFE = dict(patch_size=5, patch_distance=2, h=0.8)
_cache = {}


def geo_case(patch_size, shape_no, sigma):
    """-> (float32-exact image as float64, float64 reference, margin) of an odd patch size,
    computed once"""
    from .conftest import synth
    key = (patch_size, shape_no, sigma)
    if key not in _cache:
        shape = geo_shapes(patch_size)[shape_no]
        img = synth(shape, 200 + 10 * patch_size + shape_no, np.float32).astype(np.float64)
        out, margin = nlm_ref(img, patch_size, GEO_D, GEO_H, sigma)
        for a in (img, out, margin):
            a.setflags(write=False)
        _cache[key] = (img, out, margin)
    return _cache[key]


GEO_CASES = [(s, n, sg) for s in GEO_SIZES if s % 2 for n in range(3) for sg in GEO_SIGMAS]
