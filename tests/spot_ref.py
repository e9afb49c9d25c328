"""numpy restatement of what csrc/spot.hip and camera/flatField/vignettingFromSpotAverage.py
compute, written from the definitions (include/imgproc_hip.h, the reference's text): no tile, wave
or launch logic.  tests/test_cpu_spot.py pins it to the fixture the unchanged reference wrote
(tests/golden/spot.npz); the GPU tests compare the kernels with it.
"""
import numpy as np


def frame(img, bg):
    """`img = float64(frame); img -= avgBg`"""
    return np.asarray(img, dtype=np.float64) - bg


def average(frames):
    """transform/imgAverage.py: the float64 sum in frame order, divided by the count"""
    out = np.array(frames[0], dtype=np.float64)
    for f in frames[1:]:
        out += f
    out /= len(frames)
    return out


def background(bg):
    return bg if np.ndim(bg) == 0 else average(list(bg))


# ---------------------------------------------------------------- histogram, Otsu
def histogram(x, nbins=256):
    """np.histogram(x.ravel(), nbins) by its bin rule, element by element: the estimate, the clamp
    of the last edge, one correction down and one up against the edge table"""
    x = np.asarray(x, dtype=np.float64).ravel()
    if not np.isfinite(x).all():
        raise ValueError('autodetected range is not finite')
    lo, hi = x.min(), x.max()
    if lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    e = np.linspace(lo, hi, nbins + 1, endpoint=True)
    k = ((x - lo) * (nbins / (hi - lo))).astype(np.intp)
    k[k == nbins] -= 1
    k[x < e[k]] -= 1
    k[(x >= e[k + 1]) & (k != nbins - 1)] += 1
    assert ((e[k] <= x) & ((x < e[k + 1]) | (k == nbins - 1))).all()
    return np.bincount(k, minlength=nbins).astype(np.int64), e


def otsu(x, nbins=256):
    """skimage.filters.threshold_otsu (0.18) of a float image"""
    x = np.asarray(x, dtype=np.float64)
    first = x.ravel()[0]
    if np.all(x == first):
        return first
    counts, e = histogram(x, nbins)
    counts = counts.astype(float)
    centers = (e[:-1] + e[1:]) / 2.
    weight1 = np.cumsum(counts)
    weight2 = np.cumsum(counts[::-1])[::-1]
    mean1 = np.cumsum(counts * centers) / weight1
    mean2 = (np.cumsum((counts * centers)[::-1]) / weight2[::-1])[::-1]
    variance12 = weight1[:-1] * weight2[1:] * (mean1[:-1] - mean2[1:]) ** 2
    return centers[np.argmax(variance12)]


# ---------------------------------------------------------------- erosion
def erode(b):
    """minimum_filter(b, 3) of a bool image, `reflect` border: positions beyond the frame do not count"""
    b = np.asarray(b, dtype=bool)
    h, w = b.shape
    p = np.ones((h + 2, w + 2), bool)
    p[1:-1, 1:-1] = b
    out = np.ones((h, w), bool)
    for dy in range(3):
        for dx in range(3):
            out &= p[dy:dy + h, dx:dx + w]
    return out


def spot_mask(x, t):
    with np.errstate(invalid='ignore'):
        return erode(np.asarray(x, dtype=np.float64) > t).astype(np.uint8)


# ---------------------------------------------------------------- labelling
def label(mask, connectivity=2):
    """(labels int32, n): union-find over the foreground pixels whose roots are the smallest linear
    index of their component, numbered in the raster order of the roots"""
    m = np.asarray(mask) != 0
    h, w = m.shape
    par = np.where(m.ravel(), np.arange(h * w), -1)

    def find(i):
        r = i
        while par[r] != r:
            r = par[r]
        while par[i] != r:
            par[i], i = r, par[i]
        return r

    back = ((0, -1), (-1, 0)) + (((-1, -1), (-1, 1)) if connectivity == 2 else ())
    for i in np.flatnonzero(m.ravel()):
        y, x = divmod(int(i), w)
        for dy, dx in back:
            yy, xx = y + dy, x + dx
            if 0 <= yy and 0 <= xx < w and m[yy, xx]:
                a, b = find(i), find(yy * w + xx)
                if a != b:
                    par[max(a, b)] = min(a, b)
    labels = np.zeros(h * w, np.int32)
    number = {}
    for i in np.flatnonzero(m.ravel()):
        r = find(int(i))
        if r not in number:
            assert r == i, 'a root is the first pixel of its component'
            number[r] = len(number) + 1
        labels[i] = number[r]
    return labels.reshape(h, w), len(number)


def sizes(labels, n):
    return np.bincount(np.asarray(labels).ravel(), minlength=n + 1)[1:].astype(np.int64)


def largest(labels, n):
    """(label, size, (sum_y, sum_x)) of the largest component, the lowest label among equals; None for n = 0"""
    if n == 0:
        return None
    s = sizes(labels, n)
    k = int(np.argmax(s)) + 1
    y, x = np.nonzero(np.asarray(labels) == k)
    return k, int(s[k - 1]), (int(y.sum()), int(x.sum()))


# ---------------------------------------------------------------- the routine
def spot_average(images, bg, averageSpot=True, thresh=None):
    """vignettingFromSpotAverage.py:41-85 -> (fitimg, mask, info); info: per frame the threshold, the
    number of components, their sizes, the chosen label (0: none) and mx2, and the final mx.  Sums
    as numpy sums (the mean of a boolean selection)."""
    avg_bg = background(bg)
    fitimg, mask, mx = None, None, 0
    info = dict(t=[], n=[], sizes=[], label=[], mx2=[])
    for im in images:
        img = frame(im, avg_bg)
        if fitimg is None:
            fitimg = np.zeros_like(img)
            mask = np.zeros(img.shape, bool)
        t = otsu(img) if thresh is None else thresh
        spots, n = label(spot_mask(img, t), 2)
        info['t'].append(float(t))
        info['n'].append(n)
        info['sizes'].append(sizes(spots, n))
        big = largest(spots, n)
        if big is None:
            info['label'].append(0)
            info['mx2'].append(np.nan)
            continue
        k, size, (sy, sx) = big
        info['label'].append(k)
        if averageSpot:
            spot = np.rint([sy / float(size), sx / float(size)]).astype(int)
            mx2 = img[spot].max()       # rows spot[0] and spot[1]; IndexError for a column >= h
        else:
            spot = spots == k
            mx2 = img[spot].mean()
        fitimg[spot] = img[spot]
        mask[spot] = 1
        info['mx2'].append(float(mx2))
        if mx2 > mx:
            mx = mx2
    info['mx'] = mx
    with np.errstate(divide='ignore', invalid='ignore'):
        fitimg /= mx
    return fitimg, mask, info
