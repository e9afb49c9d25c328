"""numpy restatement of what csrc/nlf.hip computes - the frame passes of the reference's
camera/NoiseLevelFunction.py and measure/SNR/SNR.py - for shapes tests/golden/nlf.npz does not
hold.  test_cpu_nlf.py proves it equal to the fixture; the GPU tests compare the kernels with it.

`kernel_bins` is not the reference's loop but the kernel's own way to a pixel's bins (a guess
from a division, settled against the edge table), with the defects the boundary scenes are aimed
at as switches.
"""
import numpy as np

F_RMS2AAD = (2 / np.pi) ** -0.5
F_NOISE_WITH_MEDIAN = 1 + (1 / 3 ** 2)


def median3(a):
    """scipy.ndimage.median_filter(a, 3): rank 4 of the 9, the edge pixel repeated"""
    a = np.asarray(a, dtype=np.float64)
    p = np.pad(a, 1, mode='edge')
    h, w = a.shape
    st = np.stack([p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)])
    return np.sort(st, axis=0)[4]


def frames(img, img2=None, bg=None):
    """the frames as float64 after `img - bg` (SNR.py:33-40)"""
    a = np.asarray(img).astype(np.float64)
    b = None if img2 is None else np.asarray(img2).astype(np.float64)
    if bg is not None:
        a = a - bg
        b = None if b is None else b - bg
    return a, b


def signal_of(img, img2=None, bg=None):
    a, b = frames(img, img2, bg)
    return median3(a if b is None else 0.5 * (a + b))


def diff_of(img, signal, img2=None, bg=None, multiple=False):
    a, b = frames(img, img2, bg)
    if b is not None:
        return (a - b) / 2 ** 0.5
    return a - signal if multiple else (a - signal) * F_NOISE_WITH_MEDIAN


def moments(sig):
    return float(sig.min()), float(sig.max()), float(np.mean(sig)), float(np.std(sig))


def min_max(sig):
    mn, mx, av, std = moments(sig)
    return max(mn, av - 3 * std, 0), min(mx, av + 3 * std)


def edges_of(mn, step, nbins):
    e = np.empty(nbins + 1)
    m = mn
    for n in range(nbins + 1):
        e[n] = m
        m += step
    return e


def loop_bins(sig, val, e, upper_exclusive=False):
    """the reference's loop: bin n = e[n] <= signal <= e[n + 1] -> (counts, sums of val)"""
    nbins = len(e) - 1
    counts, sums = np.zeros(nbins, np.int64), np.zeros(nbins)
    with np.errstate(invalid='ignore'):
        for n in range(nbins):
            ind = (sig >= e[n]) & ((sig < e[n + 1]) if upper_exclusive else (sig <= e[n + 1]))
            counts[n] = ind.sum()
            sums[n] = val[ind].sum()
    return counts, sums


def kernel_bins(sig, val, e, step, fixup=True):
    """the kernel's way: k = floor((s - e[0]) / step), then membership of k - 1, k, k + 1 against
    the table.  fixup=False: bin k alone, trusted without a look at the table."""
    nbins = len(e) - 1
    counts, sums = np.zeros(nbins, np.int64), np.zeros(nbins)
    s, v = sig.ravel(), val.ravel()
    with np.errstate(invalid='ignore', divide='ignore'):
        kd = np.floor((s - e[0]) / step)
    kd = np.where(kd >= -1, kd, -1)
    k = np.minimum(kd, nbins).astype(np.int64)
    for off in ((-1, 0, 1) if fixup else (0,)):
        n = k + off
        ok = (n >= 0) & (n < nbins)
        nn = np.clip(n, 0, nbins - 1)
        if fixup:
            with np.errstate(invalid='ignore'):
                ok &= (e[nn] <= s) & (s <= e[nn + 1])
        np.add.at(counts, nn[ok], 1)
        np.add.at(sums, nn[ok], v[ok])
    return counts, sums


def calc_nlf(img, img2=None, signal=None, mn_mx_nbins=None, x=None, averageFn='AAD',
             signalFromMultipleImages=False, bg=None):
    """calcNLF -> (x, y, weights, signal); bins below min_len are NaN in x and y"""
    sig = signal_of(img, img2, bg) if signal is None else np.asarray(signal, dtype=np.float64)
    d = diff_of(img, sig, img2, bg, signalFromMultipleImages)
    if mn_mx_nbins is not None:
        mn, mx, nbins = mn_mx_nbins
        min_len = 0
    else:
        mn, mx = min_max(sig)
        min_len = int(sig.size * 1e-3) or 5
        nbins = 100 if mx - mn >= 100 else int(mx - mn)
    if nbins == 0:
        return np.empty(0), np.empty(0), np.zeros(0), sig
    step = (mx - mn) / nbins
    e = edges_of(mn, step, nbins)
    rms = averageFn != 'AAD'
    counts, sums = loop_bins(sig, d * d if rms else np.abs(d), e)
    keep = counts >= min_len
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = sums / counts
        y = np.where(keep, mean ** 0.5 if rms else mean * F_RMS2AAD, np.nan)
    if x is None:
        x = np.where(keep, e[1:] - 0.5 * step, np.nan)
    return x, y, np.where(keep, counts, 0).astype(np.float64), sig


def bounded_nlf(x, min_y, ax, ay):
    with np.errstate(invalid='ignore'):
        y = ay * np.sqrt(x - ax)
    return np.maximum(np.nan_to_num(y), min_y)


def background_level(img):
    """getBackgroundLevel: the 1 % point (utils/cdf.py) of the median of every 10th pixel"""
    arr = median3(np.asarray(img, dtype=np.float64)[10:-10:10, 10:-10:10])
    r = (arr.min(), arr.max())
    hist, bin_edges = np.histogram(arr, bins=2 * int(r[1] - r[0]), range=r)
    cdf = np.cumsum(hist.astype(np.float64) / hist.sum())
    return bin_edges[np.argmax(cdf > 0.01)]


def snr(img1, img2=None, bg=None, noise_level_function=None, constant_noise_level=False,
        imgs_to_be_averaged=False):
    """SNR.py:21-79; noise_level_function: a (minY, ax, ay) triple or a callable (the estimated
    NLF is the host side's work: pass what it returned)"""
    a, b = frames(img1, img2, bg)
    sig = median3(a if b is None else 0.5 * (a + b))
    if constant_noise_level:
        if b is not None:
            noise = 0.5 ** 0.5 * np.mean(np.abs(a - b)) * F_RMS2AAD
        else:
            noise = np.mean(np.abs((a - sig) * F_NOISE_WITH_MEDIAN)) * F_RMS2AAD
    else:
        f = noise_level_function
        noise = np.array(f(sig) if callable(f) else bounded_nlf(sig, *f), dtype=np.float64)
        noise[noise < 1] = 1
    if imgs_to_be_averaged:
        noise = noise * 0.5 ** 0.5
    if bg is None:
        sig = sig - background_level(a)
    with np.errstate(invalid='ignore'):
        out = np.asarray(sig / noise)
        out[out < 1] = 1
    return out
