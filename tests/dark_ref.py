"""numpy restatement of what csrc/dark.hip computes and of the flow of
imgprocessor_amd/camera/DarkCurrentMap.py around it, for the shapes tests/golden/dark.npz does not
hold.  test_cpu_dark.py proves it equal to the fixture; the GPU tests compare the kernels with it.

Every sum runs in an explicit loop over the frames, in frame order: no np.ma, no sum(axis=...),
whose order is numpy's business.  The single-time-effect steps are those of test_cpu_ste.SteNumpy.
"""
import numpy as np

from .test_cpu_ste import SteNumpy

NLF_BOUNDED_SQRT, NLF_CLIPPED_POLY, NLF_CONSTANT = range(3)


def pair_min(f0, f1):
    """np.min((i1, i2), axis=0) in float64: NaN wins"""
    return np.min((np.asarray(f0).astype(np.float64), np.asarray(f1).astype(np.float64)), axis=0)


def nlf_threshold(x, kind, params, nstd):
    x = np.asarray(x, dtype=np.float64)
    if kind == NLF_BOUNDED_SQRT:
        min_y, ax, ay = params
        with np.errstate(invalid='ignore'):
            y = ay * np.sqrt(x - ax)
        n = np.maximum(np.nan_to_num(y), min_y)
    elif kind == NLF_CLIPPED_POLY:
        p2, p1, p0, x0, x1 = params
        c = np.clip(x, x0, x1)
        n = 0.0 * c + p2          # np.polyval's Horner loop
        n = n * c + p1
        n = n * c + p0
    elif kind == NLF_CONSTANT:
        n = np.full(x.shape, float(params[0]))
    else:
        raise ValueError('unknown kind %r' % (kind,))
    with np.errstate(over='ignore'):
        return n * nstd


def stack_linregress(times, stack, mx_intensity=65535, min_ascent=0.001):
    """the definition in include/imgproc_hip.h (ipa_stack_linregress_dev), frame by frame
    -> (offset, ascent, error)"""
    x = [float(t) for t in times]
    ys = [np.asarray(f).astype(np.float64) for f in stack]
    shape = ys[0].shape
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        valid = [~(y > mx_intensity) for y in ys]
        n, sx, sy = np.zeros(shape), np.zeros(shape), np.zeros(shape)
        for k in range(len(x)):
            v = valid[k]
            n[v] += 1.0
            sx[v] += x[k]
            sy[v] += ys[k][v]
        mx, my = sx / n, sy / n
        sxx, sxy = np.zeros(shape), np.zeros(shape)
        for k in range(len(x)):
            v = valid[k]
            dx = x[k] - mx
            sxx[v] += (dx * dx)[v]
            sxy[v] += (dx * (ys[k] - my))[v]
        ascent = sxy / sxx
        offset = my - ascent * mx
        se = np.zeros(shape)
        for k in range(len(x)):
            v = valid[k]
            r = ys[k] - (offset + ascent * x[k])
            se[v] += (r * r)[v]
        error = np.sqrt(se / n)
        # getLinearityFunction's own steps (camera/DarkCurrentMap.py:73-78)
        ascent[np.isnan(ascent)] = 0
        if min_ascent > 0:
            i = ascent < min_ascent
            offset[i] += (0.5 * (np.min(x) + np.max(x))) * ascent[i]
            ascent[i] = 0
    return offset, ascent, error


def dark_current_eval(offset, ascent, t, limit, dtype=np.float64):
    with np.errstate(invalid='ignore'):
        bg = np.asarray(offset, np.float64) + np.asarray(ascent, np.float64) * t
        bg = np.where(bg > limit, limit, bg)
    return bg.astype(dtype)


def cast_trunc(a, dtype):
    """`out[:] = a`, numpy's conversion on assignment"""
    out = np.empty(np.shape(a), dtype)
    with np.errstate(invalid='ignore'):
        out[:] = a
    return out


def sort_for_same_exp_time(times, imgs):
    d = {}
    for e, i in zip(times, imgs):
        d.setdefault(e, []).append(i)
    keys = sorted(d)
    return keys, [d[k] for k in keys]


def ste_average(frames, nlf=None, nstd=3, thr=None):
    """DarkCurrentMap(frames[:2], nlf) and addImg of the others -> the SteNumpy state.  nlf: any
    callable, evaluated on min(f0, f1); or thr: the threshold itself"""
    if thr is None:
        thr = np.asarray(nlf(pair_min(frames[0], frames[1])) * nstd, dtype=np.float64)
    return SteNumpy(frames, None, None, thr=np.broadcast_to(thr, np.shape(frames[0])).copy())


def averages(times, imgs, nlfs=None, thrs=None):
    """getDarkCurrentAverages -> (times, (T, h, w) stack in imgs[0].dtype).  nlfs: one callable per
    group of two or more frames, in ascending exposure time; or thrs: their thresholds"""
    x, groups = sort_for_same_exp_time(times, imgs)
    out = np.empty((len(x),) + tuple(imgs[0].shape), imgs[0].dtype)
    nlfs = [None] * len(thrs) if nlfs is None else list(nlfs)
    thrs = [None] * len(nlfs) if thrs is None else list(thrs)
    for n, g in enumerate(groups):
        if len(g) == 1:
            out[n] = g[0]
        else:
            out[n] = cast_trunc(ste_average(g, nlfs.pop(0), thr=thrs.pop(0)).avg, imgs[0].dtype)
    assert not nlfs and not thrs
    return x, out


def dark_current_function(times, imgs, nlfs=None, thrs=None, **kwargs):
    x, avg = averages(times, imgs, nlfs, thrs)
    return stack_linregress(x, avg, **kwargs)
