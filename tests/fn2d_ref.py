"""numpy restatement of csrc/fn2d.hip: the per-pixel terms operation by operation in float64 (numpy never
fuses a multiply into an add, the unit is compiled without contraction), the sums through math.fsum -
and, for the bit-for-bit check, in the device's own order.  Parameters as ops_fn2d takes them:
'KW' (f, alpha, cx, cy), 'AoV' (a, c0, c1).  The model's x is the row index.  numpy only, but
`function` drives the package's own host loop (ops.fn2d_fit) over `normal`."""
import math

import numpy as np

from . import reduce_ref as rr
from .fn2d_cases import index_grid

FITTED = {'KW': 4, 'AoV': 1}


def _f64(*a):
    return [np.asarray(v, dtype=np.float64) for v in a]


# ---------------------------------------------------------------- evaluation (Model<.>::value)
def value(model, params, x, y):
    """the model at the positions (x, y) in the reference's operation order, float64"""
    x, y = _f64(x, y)
    if model == 'KW':
        f, alpha, cx, cy = [np.float64(v) for v in params]
        dx, dy = x - cx, y - cy
        d = np.sqrt(dx * dx + dy * dy)
        t = d / f
        q = 1.0 + t * t
        A = 1.0 / (q * q)
        G = 1.0 - alpha * d
        return A * G
    a, c0, c1 = [np.float64(v) for v in params]
    tan_a = np.tan(a)
    dx, dy = x - c0, y - c1
    return 1.0 / np.sqrt(1.0 + tan_a * ((dx * dx + dy * dy) / c0))


def evaluate(model, params, arr, mask=None, outgrid=None):
    """ipa_fn2d_eval_dev -> (result in arr's type, its np.max as float64)"""
    arr = np.asarray(arr)
    if outgrid is not None:
        out = value(model, params, outgrid[0], outgrid[1]).astype(arr.dtype)
    else:
        out = value(model, params, *index_grid(arr.shape)).astype(arr.dtype)
        if mask is not None:
            out = np.where(np.asarray(mask, bool), out, arr)
    return out, np.float64(np.max(out))


def divide(arr, div):
    """arr / div as numpy divides an array by a scalar of its own type"""
    return arr / arr.dtype.type(div)


# ---------------------------------------------------------------- normal equations (Model<.>::terms)
def model_terms(model, params, shape):
    """-> (m, [J_0 .. J_{P-1}]) on the frame's index grid, in the kernel's cheaper formulation"""
    x, y = index_grid(shape)
    if model == 'KW':
        f, alpha, cx, cy = [np.float64(v) for v in params]
        f2 = f * f
        inv_f2, k4, k4f = 1.0 / f2, 4.0 / f2, 4.0 / (f2 * f)
        dx = x - cx
        dx2 = dx * dx
        dy = y - cy
        r2 = dx2 + dy * dy
        d = np.sqrt(r2)
        q = 1.0 + r2 * inv_f2
        dd = np.where(d == 0.0, 1.0, d)
        wq = 1.0 / (q * dd)
        iq = wq * dd
        idist = np.where(d == 0.0, 0.0, wq * q)
        A = iq * iq
        G = 1.0 - alpha * d
        gaq = G * A * iq
        cc = gaq * k4 + A * alpha * idist
        return A * G, [gaq * k4f * r2, -(A * d), cc * dx, cc * dy]
    a, c0, c1 = [np.float64(v) for v in params]
    tan_a = np.tan(a)
    inv_c0, hs = 1.0 / c0, -0.5 * (1.0 + tan_a * tan_a)
    dx = x - c0
    dx2 = dx * dx
    dy = y - c1
    g = (dx2 + dy * dy) * inv_c0
    u = 1.0 + tan_a * g
    m = 1.0 / np.sqrt(u)
    return m, [hs * (m * m * m) * g]


def sum_terms(img, model, params):
    """(NE, h, w): what every pixel adds to the upper triangle of J^T J by rows | J^T r | S | the count"""
    img = np.asarray(img)
    m, J = model_terms(model, params, img.shape)
    r = img.astype(np.float64) - m
    P = len(J)
    t = [J[i] * J[j] for i in range(P) for j in range(i, P)] + [J[i] * r for i in range(P)] + [r * r, np.ones(img.shape)]
    return np.stack(t)


def _valid(img, mask):
    return np.ones(np.shape(img), bool) if mask is None else ~np.asarray(mask, bool)


def _unpack(v, P):
    nt = P * (P + 1) // 2
    JtJ = np.zeros((P, P))
    JtJ[np.triu_indices(P)] = v[:nt]
    JtJ = JtJ + np.triu(JtJ, 1).T
    return JtJ, np.array(v[nt:nt + P]), float(v[nt + P]), int(v[nt + P + 1])


def flat_sums(img, mask, model, params):
    """-> (the NE sums through math.fsum, the NE sums of |term|) over the valid pixels"""
    with np.errstate(all='ignore'):
        t = sum_terms(img, model, params)[:, _valid(img, mask)]
    return (np.array([math.fsum(row) if np.isfinite(row).all() else np.sum(row) for row in t]),
            np.array([math.fsum(np.abs(row)) for row in t]))


def normal_sums(img, mask, model, params):
    """ipa_fn2d_normal_dev as ops.fn2d_normal returns it"""
    return _unpack(flat_sums(img, mask, model, params)[0], FITTED[model])


def normal(img, mask, model):
    """the `normal` callable of ops.fn2d_fit over this restatement"""
    return lambda params: normal_sums(img, mask, model, params)


def device_grid(h, cu_count):
    """the stage-1 grid of fn2d_normal_kernel and the trips of a workgroup"""
    quads = (h + 3) // 4
    grid = min(quads, min(cu_count * 8, 2048))
    return grid, (quads + grid - 1) // grid


def ordered_sums(img, mask, model, params, grid):
    """the NE sums in the device's order: a wave walks rows 4 (b + k grid) + wave, lane l adds the pixels
    l, l + 64, .. of each onto 0.0; the butterfly lane[l] + lane[l ^ d] for d = 32 .. 1; entry e of the four waves
    added onto 0.0, wave 0 first; the workgroups' partials through merge_partials (reduce_ref.fold_partials)"""
    t, live = sum_terms(img, model, params), _valid(img, mask)
    ne, h, w = t.shape
    iters = ((h + 3) // 4 + grid - 1) // grid
    lanes = np.arange(64)
    parts = np.zeros((grid, ne))
    for b in range(grid):
        for wave in range(4):
            acc = np.zeros((ne, 64))
            for it in range(iters):
                row = (it * grid + b) * 4 + wave
                if row >= h:
                    break
                for x0 in range(0, w, 64):
                    v, on = t[:, row, x0:x0 + 64], live[row, x0:x0 + 64]
                    n = v.shape[1]
                    acc[:, :n] = np.where(on, acc[:, :n] + v, acc[:, :n])
            d = 32
            while d:
                acc = acc + acc[:, lanes ^ d]
                d //= 2
            parts[b] = parts[b] + acc[:, 0]
    return np.array([rr.fold_partials(parts[:, e]) for e in range(ne)])


# ---------------------------------------------------------------- the whole routine
def function(img, mask=None, replace_all=False, outgrid=None, model='KW', guess=None):
    """camera/flatField/postprocessing/function.py over this restatement -> (result, params, S, calls)"""
    from imgprocessor_amd import ops
    from .fn2d_cases import first_guess
    img = np.asarray(img)
    if outgrid is not None or mask is None:
        replace_all = True
    if guess is None:
        guess = first_guess(model, img.shape)
    params, S, _, calls = ops.fn2d_fit(None, None, model, guess, normal=normal(img, mask, model))
    out, top = evaluate(model, params, img, None if replace_all else mask, outgrid)
    return divide(out, top), params, S, calls
