"""The secondary stencils restated in numpy float64, one plain loop per output pixel: the
yardstick of tests/test_gpu_stencil_paths.py (validated without a GPU against the reference's
own fixtures and the C oracle in tests/test_cpu_stencil_refs.py).

Written from the definitions (header comments of csrc/stencils.hip, csrc/stencils_ydep.hip and
the wrappers' docstrings), with no tile, wave or LDS logic:

  local_std          sqrt(sum_W (img - blurred[i, j])**2 / ((rows - 1) (cols - 1))), W the window
                     [i - kx // 2, i + kx // 2) x [j - ky // 2, j + ky // 2) clipped to the image
                     (kx on the row axis), rows / cols its clipped extent
  masked_mean        mean of the unmasked pixels of [i - k, i + k) x [j - k, j + k) clipped,
  masked_median      k = ksize // 2; fill: written into the masked pixels that have at least one
                     such neighbour, else: into the unmasked pixels of a NaN array.  The median
                     is np.median (two middle values averaged in the array dtype, NaN if any NaN)
  nan_max            np.nanmax over the same window, NaN when the window is all NaN
  closest_distance   distance to the closest set pixel within +-ksize (both ends included),
                     2 ksize when there is none (or none closer), 0 on set pixels; uint16 output
                     truncates
  pos_intensity_unc  sqrt(sum psf[ii, jj] (img[i - ii + c, j - jj + c] - img[i, j])**2), psf the
                     (2 k + 1)**2 Gaussian exp(-((ii - c)**2 / 2 sx**2 + (jj - c)**2 / 2 sy**2))
                     normalised to 1 (sx on the ROW axis); pixels closer than k to the rim and
                     NaN centres stay 0
  median_threshold   blur = rank size**2 // 2 of the size x size window at offsets
                     -size // 2 ... size - 1 - size // 2 (scipy's origin for even sizes), edge
                     pixels repeated; hit = |(img - blur) / blur| > thr ('<'); out = hit ? blur : img
  var_y_gauss        out[r] = sum kernels[r, ii, jj] ext[r + ii, c + jj] with NaN pixels skipped,
                     kernels[r] = scipy gaussian_filter(delta, (stdys[r], stdx)), ext the padded
                     frame (modex 'wrap' or 'reflect', modey 'reflect', edge pixels repeated)

Where a mean is formed the sum is taken in extended precision (np.longdouble: a 64-bit mantissa
on x86, pairwise float64 elsewhere), so that the error of an implementation against these is
its own.
"""
import math

import numpy as np


def _sum(v):
    return np.float64(np.sum(v, dtype=np.longdouble))


def _clip(i, k, n):
    return max(i - k, 0), min(i + k, n)


def local_std(img, blurred, ksize):
    img = np.asarray(img, dtype=np.float64)
    blurred = np.asarray(blurred, dtype=np.float64)
    hx, hy = int(ksize[0]) // 2, int(ksize[1]) // 2
    H, W = img.shape
    out = np.empty((H, W))
    with np.errstate(divide='ignore', invalid='ignore'):
        for i in range(H):
            r0, r1 = _clip(i, hx, H)
            for j in range(W):
                c0, c1 = _clip(j, hy, W)
                d = img[r0:r1, c0:c1] - blurred[i, j]
                val = _sum(d * d)
                out[i, j] = np.sqrt(val / np.float64((r1 - r0 - 1) * (c1 - c0 - 1)))
    return out


def _masked(arr, mask, ksize, fill_mask, stat):
    arr = np.asarray(arr)
    mask = np.asarray(mask) != 0
    k = int(ksize) // 2
    H, W = arr.shape
    out = arr.copy() if fill_mask else np.full_like(arr, np.nan)
    for i in range(H):
        r0, r1 = _clip(i, k, H)
        for j in range(W):
            if mask[i, j] != bool(fill_mask):
                continue
            c0, c1 = _clip(j, k, W)
            vals = arr[r0:r1, c0:c1][~mask[r0:r1, c0:c1]]
            if vals.size:
                out[i, j] = stat(vals)
    return out


def masked_mean(arr, mask, ksize, fill_mask=True):
    """float64 result whatever the dtype of arr (its values are taken as they are)"""
    return _masked(np.asarray(arr, dtype=np.float64), mask, ksize, fill_mask,
                   lambda v: _sum(v) / v.size)


def _median(v):
    if np.isnan(v).any():
        return np.nan
    s = np.sort(v)
    n = s.size
    with np.errstate(invalid='ignore', over='ignore'):
        return (s[(n - 1) // 2] + s[n // 2]) * v.dtype.type(0.5)


def masked_median(arr, mask, ksize, fill_mask=True):
    """in the dtype of arr: selection, and one addition and halving in that dtype"""
    return _masked(arr, mask, ksize, fill_mask, _median)


def nan_max(arr, ksize):
    arr = np.asarray(arr)
    k = int(ksize) // 2
    H, W = arr.shape
    out = np.full_like(arr, np.nan)
    for i in range(H):
        r0, r1 = _clip(i, k, H)
        for j in range(W):
            c0, c1 = _clip(j, k, W)
            w = arr[r0:r1, c0:c1]
            w = w[~np.isnan(w)]
            if w.size:
                out[i, j] = w.max()
    return out


def closest_distance(arr, ksize, dtype=np.uint16):
    a = np.asarray(arr) != 0
    H, W = a.shape
    si, sj = np.nonzero(a)
    out = np.zeros((H, W))
    for i in range(H):
        for j in range(W):
            if a[i, j]:
                continue
            md = 2.0 * ksize
            near = (np.abs(si - i) <= ksize) & (np.abs(sj - j) <= ksize)
            if near.any():
                d = math.sqrt(int(((si[near] - i) ** 2 + (sj[near] - j) ** 2).min()))
                if d < md:
                    md = d
            out[i, j] = md
    return np.floor(out).astype(np.uint16) if np.dtype(dtype) == np.uint16 else out


def pos_intensity_unc(image, sx, sy, k):
    img = np.asarray(image, dtype=np.float64)
    H, W = img.shape
    k = int(k)
    maps = isinstance(sx, np.ndarray)
    t = (np.arange(2 * k + 1) - k).astype(np.float64) ** 2
    out = np.zeros((H, W))
    for i in range(k, H - k):
        for j in range(k, W - k):
            c = img[i, j]
            if np.isnan(c):
                continue
            v0, v1 = (float(sx[i, j]), float(sy[i, j])) if maps else (float(sx), float(sy))
            psf = np.exp(-(t[:, None] / (2 * v0 * v0) + t[None, :] / (2 * v1 * v1)))
            psf /= psf.sum()
            # psf[ii, jj] meets img[i - ii + c, j - jj + c]: the window read backwards
            d = img[i - k:i + k + 1, j - k:j + k + 1][::-1, ::-1] - c
            out[i, j] = np.sqrt((psf * d * d).sum())
    return out


def median_threshold(img, threshold, size=3, condition='>'):
    """-> (out in the dtype of img, hit bool)"""
    img = np.asarray(img)
    size = int(size)
    lo, hi = size // 2, size - 1 - size // 2
    ext = np.pad(img, ((lo, hi), (lo, hi)), mode='symmetric')
    win = np.lib.stride_tricks.sliding_window_view(ext, (size, size))
    blur = np.sort(win.reshape(img.shape + (size * size,)), axis=-1)[..., (size * size) // 2]
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = np.abs((img.astype(np.float64) - blur.astype(np.float64)) / blur.astype(np.float64))
    hit = rel < threshold if condition == '<' else rel > threshold
    return np.where(hit, blur, img), hit


def var_y_sizes(stdyrange, stdx):
    """-> (mn, mx, ky, kx) as filters/varYSizeGaussianFilter derives them"""
    mn, mx = stdyrange if type(stdyrange) in (list, tuple) else (0, stdyrange)
    kx = int(stdx * 2.5)
    kx += 1 - kx % 2
    ky = int(mx * 2.5)
    ky += 1 - ky % 2
    return mn, mx, ky, kx


def var_y_gauss(arr, stdyrange, stdx=0, modex='wrap'):
    """float64 result whatever the dtype of arr"""
    import scipy.ndimage as ndi
    a = np.asarray(arr, dtype=np.float64)
    H, W = a.shape
    mn, mx, ky, kx = var_y_sizes(stdyrange, stdx)
    ext = np.pad(a, ((0, 0), (kx // 2, kx // 2)), mode='wrap' if modex == 'wrap' else 'symmetric')
    ext = np.pad(ext, ((ky // 2, ky // 2), (0, 0)), mode='symmetric')
    ext = np.where(np.isnan(ext), 0.0, ext)   # a skipped pixel adds nothing
    delta = np.zeros((ky, kx))
    delta[ky // 2, kx // 2] = 1
    out = np.zeros((H, W))
    for r, s in enumerate(np.linspace(mn, mx, H)):
        kern = ndi.gaussian_filter(delta, (s, stdx))
        for ii in range(ky):
            for jj in range(kx):
                out[r] += kern[ii, jj] * ext[r + ii, jj:jj + W]
    return out
