"""numpy restatement of csrc/poly.hip and of the layers above it (interpolate/polyfit2d.py,
camera/flatField/postprocessing/polynomial.py), written from the definitions in
include/imgproc_hip.h: no tile, wave or slab logic.

  * the coordinate map and the Chebyshev recurrence;
  * the moments, every sum exact (math.fsum), with sum |terms| beside each for the tolerance;
  * the Gram assembly T_i T_k = (T_{i+k} + T_{|i-k|}) / 2, written as four loops;
  * the evaluation in the kernel's operation order - equal to the device bit for bit;
  * _highGrad without scipy (the CPU tests compare it with scipy exactly);
  * polyfit2dGrid and the POLY repair loop on top of these.
"""
import math

import numpy as np


def coord(p, n):
    p = np.asarray(p, dtype=np.float64)
    if n == 1:
        return np.zeros_like(p)
    return (2.0 * p - float(n - 1)) / float(n - 1)


def cheb(u, n):
    """[T_0 .. T_n] of u"""
    t = [np.ones_like(u)]
    if n >= 1:
        t.append(u.copy())
    t2 = 2.0 * u
    for k in range(2, n + 1):
        t.append(t2 * t[k - 1] - t[k - 2])
    return t


def moments(arr, mask, order):
    """-> M, R, count, absM, absR over the pixels where mask is not set"""
    h, w = arr.shape
    valid = np.ones((h, w), bool) if mask is None else ~np.asarray(mask, bool)
    y, x = np.nonzero(valid)
    z = arr[valid].astype(np.float64)
    tu, tv = cheb(coord(x, w), 2 * order), cheb(coord(y, h), 2 * order)
    n, k = 2 * order + 1, order + 1
    M, aM, R, aR = np.zeros((n, n)), np.zeros((n, n)), np.zeros((k, k)), np.zeros((k, k))
    for b in range(n):
        for a in range(n):
            t = tv[b] * tu[a]
            M[b, a], aM[b, a] = math.fsum(t), math.fsum(np.abs(t))
    for j in range(k):
        for i in range(k):
            t = z * (tv[j] * tu[i])
            R[j, i], aR[j, i] = math.fsum(t), math.fsum(np.abs(t))
    return M, R, int(valid.sum()), aM, aR


def gram(M, order):
    k = order + 1
    G = np.zeros((k * k, k * k))
    for j in range(k):
        for i in range(k):
            for l in range(k):
                for m in range(k):
                    G[j * k + i, l * k + m] = 0.25 * (M[j + l, i + m] + M[j + l, abs(i - m)] +
                                                      M[abs(j - l), i + m] + M[abs(j - l), abs(i - m)])
    return G


def solve(M, R, count, order):
    k = order + 1
    if count < k * k:
        raise ValueError('too few valid pixels')
    G = gram(M, order)
    ev = np.linalg.eigvalsh(G)
    if not ev[0] > 1e-13 * ev[-1]:
        raise ValueError('singular')
    return np.linalg.solve(G, R.reshape(-1)).reshape(k, k)


def evaluate(coef, px, py, shape, dtype):
    """the polynomial at pixel positions (py, px) of a frame of `shape`, in the kernel's order"""
    h, w = shape
    o = coef.shape[0] - 1
    px, py = np.asarray(px, dtype=np.float64), np.asarray(py, dtype=np.float64)
    tu, tv = cheb(coord(px, w), o), cheb(coord(py, h), o)
    val = None
    for j in range(o + 1):
        s = np.full(px.shape, coef[j, 0])
        for i in range(1, o + 1):
            s = s + coef[j, i] * tu[i]
        val = s if j == 0 else val + s * tv[j]
    return val.astype(dtype)


def fill(coef, arr, mask):
    """-> (copy with the masked pixels replaced, sum |new - old| over them); mask None: every pixel"""
    h, w = arr.shape
    y, x = np.mgrid[0:h, 0:w]
    new = evaluate(coef, x, y, (h, w), arr.dtype)
    m = np.ones((h, w), bool) if mask is None else np.asarray(mask, bool)
    out = arr.copy()
    out[m] = new[m]
    return out, math.fsum(np.abs(new[m].astype(np.float64) - arr[m].astype(np.float64)))


def fit(arr, mask, order):
    M, R, count, _, _ = moments(arr, mask, order)
    return solve(M, R, count, order)


def polyfit2dGrid(arr, mask=None, order=3, replace_all=False, copy=True, outgrid=None):
    """-> (result, residuum sum or None); `arr` itself for an empty mask"""
    if mask is not None and not np.asarray(mask, bool).any() and not replace_all and outgrid is None:
        return arr, 0.0
    coef = fit(arr, mask, order)
    if outgrid is not None:
        return evaluate(coef, outgrid[1], outgrid[0], arr.shape, arr.dtype), None
    if mask is None:
        return fill(coef, arr, None)
    if replace_all:
        return fill(coef, arr, None)[0], None
    return fill(coef, arr, mask)


def laplace(arr):
    """scipy.ndimage.laplace(arr, mode='reflect'): per axis c * (-2) + (l + r) in double, stored in the
    array's type, axis 0 plus axis 1 in the array's type"""
    a = arr.astype(np.float64)
    out = None
    for axis in (0, 1):
        p = np.concatenate([a.take([0], axis), a, a.take([-1], axis)], axis)
        n = a.shape[axis]
        l, r = p.take(range(0, n), axis), p.take(range(2, n + 2), axis)
        d = (a * -2.0 + (l + r)).astype(arr.dtype)
        out = d if out is None else out + d
    return out


def window(shape):
    return min(max(min(shape) // 5, 3), 15)


def dilate(b, size):
    """maximum_filter(b, size) of a boolean with scipy's reflecting border: offsets -(size // 2) ..
    size - size // 2 - 1 per axis, clipped (the reflection repeats pixels inside the window)"""
    lo, hi = size // 2, size - size // 2 - 1
    out = b
    for axis in (1, 0):
        n = out.shape[axis]
        acc = np.zeros_like(out)
        for d in range(max(-lo, 1 - n), min(hi, n - 1) + 1):
            src = [slice(None)] * 2
            dst = [slice(None)] * 2
            src[axis] = slice(max(d, 0), n + min(d, 0))
            dst[axis] = slice(max(-d, 0), n + min(-d, 0))
            acc[tuple(dst)] |= out[tuple(src)]
        out = acc
    return out


def high_grad(arr, threshold=0.01, size=None):
    lap = laplace(arr)
    b = np.abs(lap) > arr.dtype.type(threshold)
    return dilate(b, window(arr.shape) if size is None else size)


def polynomial(img, mask, inplace=False, replace_all=False, max_dev=1e-5, max_iter=20, order=2):
    """the reference's loop on the restated fit -> (out, trace, exit): trace holds (residuum, m) per
    iteration (None where the iteration did not get there), exit is 'replace_all', 'res', 'same',
    'all' or 'max_iter'"""
    out = img if inplace else img.copy()
    lastm = 0
    trace, why = [], 'max_iter'
    for _ in range(max_iter):
        if inplace and mask is not None and not replace_all and np.asarray(mask, bool).any():
            coef = fit(out, mask, order)
            new, _ = fill(coef, out, mask)
            out[...] = new
            out2, rsum = out, 0.0
        else:
            out2, rsum = polyfit2dGrid(out, mask, order=order, replace_all=replace_all)
        if replace_all:
            out = out2
            trace.append((None, None))
            why = 'replace_all'
            break
        res = 0.0 if out2 is out else rsum / out.size
        if res < max_dev:
            out = out2
            trace.append((res, None))
            why = 'res'
            break
        out = out2
        mask = high_grad(out)
        m = int(mask.sum())
        trace.append((res, m))
        if m == lastm or m == img.size:
            why = 'same' if m == lastm else 'all'
            break
        lastm = m
    return np.clip(out, 0, 1), trace, why
