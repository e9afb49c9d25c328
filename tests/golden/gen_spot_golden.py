#!/usr/bin/env python3
"""Generate tests/golden/spot.npz: the flat field from spot images as the reference computes it
(camera/flatField/vignettingFromSpotAverage.py over skimage's threshold_otsu and label, scipy's
minimum_filter and center_of_mass, utils/getBackground2.py, transform/imgAverage.py), and what
skimage.measure.label and scipy.ndimage.label give on the labelling patterns of
tests/spot_cases.py.  Runs only where the reference source, skimage and scipy exist.

The reference runs unchanged under the throw-away stand-ins of gen_golden.py / gen_ste_golden.py /
gen_flat_golden.py (numba shim, constants-only cv2, the running mean, the two import-only
fancytools stubs).  The generator only listens: the names the reference's module looks up -
imread, threshold_otsu, label - are wrapped to note the frame after the background left it, the
threshold, the 256 counts np.histogram gives skimage, the label image and its count; the wrapped
functions' results go back unchanged.  From those notes it repeats the rest of the loop with the
reference's own expressions and asserts that the result equals the reference's output to the bit.

Conditions of the tests, asserted here (conditions, not measurements):
  - in every averageSpot=False scene the two largest per-frame spot means differ by more than 1e-9
    relative: a last-digit difference in a sum cannot change which frame supplies mx;
  - the planted tie in spot size is an exact integer tie, and the first spot in raster order wins;
  - every kind of scene occurs: a frame without a spot, a given threshold, a scalar background,
    averaged background frames, an averageSpot=True scene that succeeds and one that raises
    IndexError;
  - skimage's and scipy's labels agree on every pattern at both connectivities.

The fixture holds arrays only.

    python tests/golden/gen_spot_golden.py [other/path/spot.npz]
"""
import contextlib
import io
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden import install_shim  # noqa: E402
from gen_ste_golden import install_standins  # noqa: E402
from gen_flat_golden import install_stubs  # noqa: E402
import spot_cases as sc  # noqa: E402

warnings.filterwarnings('ignore')


def run_scene(V, name, scene, out):
    notes = []      # one dict per frame
    cur = {}
    ref_imread, ref_otsu, ref_label = V.imread, V.threshold_otsu, V.label

    def imread(img, *a, **k):
        res = ref_imread(img, *a, **k)
        cur.clear()
        cur['img'] = res          # the reference subtracts the background in place
        notes.append(cur.copy())
        return res

    def threshold_otsu(img, *a, **k):
        t = ref_otsu(img, *a, **k)
        notes[-1]['t'] = float(t)
        notes[-1]['counts'] = np.histogram(img.ravel(), 256)[0]
        return t

    def label(mask, *a, **k):
        spots, n = ref_label(mask, *a, **k)
        notes[-1].update(img=cur['img'].copy(), mask=np.asarray(mask).copy(), spots=spots.copy(), n=n)
        return spots, n

    V.imread, V.threshold_otsu, V.label = imread, threshold_otsu, label
    images = [f.copy() for f in scene['images']]
    bg = scene['bg'] if np.ndim(scene['bg']) == 0 else [b.copy() for b in scene['bg']]
    text = io.StringIO()
    raised = None
    try:
        with contextlib.redirect_stdout(text):
            fitimg, mask = V.vignettingFromSpotAverage(images, bg, averageSpot=scene['averageSpot'],
                                                       thresh=scene['thresh'])
    except IndexError as e:
        raised = e
    finally:
        V.imread, V.threshold_otsu, V.label = ref_imread, ref_otsu, ref_label
    assert (raised is not None) == (scene['raises'] is IndexError), (name, raised)

    p = name + '_'
    frames = scene['images'] + ([] if np.ndim(scene['bg']) == 0 else scene['bg'])
    out[p + 'in_sum'] = np.array([np.asarray(f, np.float64).sum() for f in frames])
    out[p + 'printed'] = np.array(text.getvalue())
    out[p + 't'] = np.array([n.get('t', scene['thresh']) for n in notes], dtype=np.float64)
    if scene['thresh'] is None:
        out[p + 'counts'] = np.stack([n['counts'] for n in notes]).astype(np.int64)
    out[p + 'n'] = np.array([n['n'] for n in notes])
    out[p + 'spots'] = np.stack([n['spots'] for n in notes]).astype(np.uint8)
    assert all(n['spots'].max() < 256 for n in notes)
    # the rest of the loop from the notes, with the reference's expressions
    fit2, mask2, mx, mx2s, labels = None, None, 0, [], []
    sizes = []
    for k, n in enumerate(notes):
        img, spots = n['img'], n['spots']
        if fit2 is None:
            fit2, mask2 = np.zeros_like(img), np.zeros_like(img, dtype=bool)
        spot_sizes = [(spots == i).sum() for i in range(1, n['n'] + 1)]
        sizes.append(spot_sizes)
        if not spot_sizes:
            labels.append(0)
            mx2s.append(np.nan)
            continue
        labels.append(int(np.argmax(spot_sizes)) + 1)
        spot = spots == labels[-1]
        if scene['averageSpot']:
            from scipy.ndimage import center_of_mass
            spot = np.rint(center_of_mass(spot)).astype(int)
            if spot[1] >= img.shape[0]:
                assert raised is not None and k == len(notes) - 1
                labels[-1] = -labels[-1]
                mx2s.append(np.nan)
                break
            mx2 = img[spot].max()
        else:
            mx2 = img[spot].mean()
        fit2[spot] = img[spot]
        mask2[spot] = 1
        mx2s.append(float(mx2))
        if mx2 > mx:
            mx = mx2
    out[p + 'label'] = np.array(labels)
    out[p + 'mx2'] = np.array(mx2s)
    out[p + 'mx'] = np.array(float(mx))
    width = max([len(s) for s in sizes] + [1])
    out[p + 'sizes'] = np.array([list(s) + [0] * (width - len(s)) for s in sizes], dtype=np.int64)
    if raised is None:
        fit2 /= mx
        assert len(notes) == len(images)
        assert np.array_equal(fit2, fitimg, equal_nan=True) and np.array_equal(mask2, mask), name
        assert fitimg.dtype == np.float64 and mask.dtype == bool
        out[p + 'fitimg'] = fitimg
        out[p + 'mask'] = mask
    if not scene['averageSpot'] and np.isfinite(mx2s).sum() >= 2:
        top = np.sort(np.array(mx2s)[np.isfinite(mx2s)])[-2:]
        assert top[1] - top[0] > 1e-9 * top[1], 'the two largest spot means are too close: %r' % (top,)
    return notes, labels, sizes, raised


def main(path=os.path.join(HERE, 'spot.npz')):
    if not hasattr(np, 'asfarray'):
        np.asfarray = lambda a, dtype=np.float64: np.asarray(a, dtype=dtype)
    install_shim()
    mma_source = install_standins()
    stubs = install_stubs()
    from imgProcessor.camera.flatField import vignettingFromSpotAverage as V
    import skimage
    import scipy
    from skimage.measure import label as sk_label
    from scipy.ndimage import label as sp_label

    out = {'mma_source': np.array(mma_source), 'stubs': np.array(stubs),
           'versions': np.array('numpy %s, scipy %s, skimage %s' % (np.__version__, scipy.__version__,
                                                                    skimage.__version__))}
    kinds = set()
    for name, scene in sc.scenes().items():
        notes, labels, sizes, raised = run_scene(V, name, scene, out)
        kinds.add(('rows' if scene['averageSpot'] else 'spot') + ('_raises' if raised else ''))
        kinds.add('thresh' if scene['thresh'] is not None else 'otsu')
        kinds.add('scalar_bg' if np.ndim(scene['bg']) == 0 else 'bg_frames')
        if any(k == 0 for k in labels):
            kinds.add('no_spot')
            assert "couldn't find spot in image" in str(out[name + '_printed'])
        if name.startswith('a_'):
            # the planted tie: two components of the same size, the first one chosen
            s = sizes[2]
            assert len(s) == 2 and s[0] == s[1] == (sc.SPOT - 2) ** 2 and labels[2] == 1, s
    assert kinds == {'rows', 'rows_raises', 'spot', 'thresh', 'otsu', 'scalar_bg', 'bg_frames', 'no_spot'}, kinds

    for name, m in sc.golden_patterns().items():
        for conn in (1, 2):
            sk, n_sk = sk_label(m, background=0, return_num=True, connectivity=conn)
            sp, n_sp = sp_label(m, None if conn == 1 else np.ones((3, 3)))
            assert n_sk == n_sp and np.array_equal(sk, sp), (name, conn)
            assert n_sk < 65536
            out['label_%s_c%d' % (name, conn)] = sk.astype(np.uint16)
            out['label_%s_c%d_n' % (name, conn)] = np.array(n_sk)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= 100 * 1024, size
    print('wrote %s (%d bytes, %d arrays; %s; running mean: %s, stubs: %s)'
          % (path, size, len(out), out['versions'], mma_source, stubs))


if __name__ == '__main__':
    main(*sys.argv[1:2])
