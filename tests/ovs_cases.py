"""Scenes for the object / vignetting separation tests (tests/test_cpu_ovs.py, tests/test_gpu_ovs.py):
the shapes, frame counts and matrices of the kernel tests with their planted values, and the loop
scene - a vignetted object imaged at random positions.  Everything is generated, deterministic and
small; arrays handed out more than once are read-only."""
import numpy as np

ALL_DTYPES = (np.uint8, np.uint16, np.float32, np.float64)
MAX_FRAMES = 64
# (object shape, flat-field shape): one pixel; rows with a pitch; more than one 64 x 4 workgroup in
# both directions of both grids
SHAPES = (((1, 1), (1, 1)), ((3, 67), (5, 70)), ((33, 130), (41, 257)))
BIG = SHAPES[2]
N_VALUES = (1, 2, 5, 64)
# which of the five matrices a call of N frames uses: N = 1 is the fit that misses entirely
MATRIX_PICK = {1: (4,), 2: (2, 3), 5: (0, 1, 2, 3, 4)}
IDENTITY, TRANSLATION, ROTATION, PARTIAL, MISS = range(5)
DBL_MAX = np.finfo(np.float64).max


def top_of(dtype):
    return {np.dtype(np.uint8): 200.0, np.dtype(np.uint16): 3000.0}.get(np.dtype(dtype), 1.0)


def matrices(src_shape, dst_shape):
    """the five destination -> source matrices of the kernel tests for a destination of dst_shape
    sampled from a source of src_shape: the identity; an integer translation (weights exactly 0 and
    1); the rotation + perspective of test_vignetting_random_steps_warps; a placement that leaves
    part of the destination outside the source (border footprints, footprints wholly outside); a
    fit that misses the source entirely"""
    sh, sw = src_shape
    dh, dw = dst_shape
    a = np.deg2rad(3.0)
    rot = np.array([[np.cos(a), -np.sin(a), 6.0], [np.sin(a), np.cos(a), -4.0], [1e-4, -5e-5, 1.0]])
    part = np.array([[1.02, 0.0, sw - 0.5 * dw - 0.3], [0.01, 0.98, -2.25], [0.0, 0.0, 1.0]])
    miss = np.array([[1.0, 0.0, 5000.0], [0.0, 1.0, 7000.0], [0.0, 0.0, 1.0]])
    trans = np.array([[1.0, 0.0, 1.0 if sw > dw else -1.0], [0.0, 1.0, 1.0 if sh > dh else -1.0], [0.0, 0.0, 1.0]])
    return np.stack([np.eye(3), trans, rot, part, miss])


def pick(mats, n):
    idx = MATRIX_PICK.get(n) or tuple(i % 5 for i in range(n))
    return np.ascontiguousarray(mats[list(idx)])


def fit_stack(n, shape, dtype, seed):
    """n fitted images: values in (0.2, 1] of the type's range, a block of exact zeros, and for the
    float types a negative value"""
    rng = np.random.default_rng(seed)
    h, w = shape
    top = top_of(dtype)
    f = rng.uniform(0.2 * top, top, (n, h, w))
    if h * w > 40:
        f[:, h // 2, 4:8] = 0.0
        if np.dtype(dtype).kind == 'f':
            f[:, h // 2, 12] = -0.7
    return f.astype(dtype) if np.dtype(dtype).kind == 'f' else np.round(f).astype(dtype)


def mask_stack(n, shape, seed):
    """fit masks: a border (3 px where the image is large enough), a block inside, a few single
    pixels - masked pixels next to unmasked ones"""
    rng = np.random.default_rng(seed)
    h, w = shape
    m = np.zeros((n, h, w), np.uint8)
    if h > 8 and w > 8:
        m[:, :3, :] = m[:, -3:, :] = 1
        m[:, :, :3] = m[:, :, -3:] = 1
        m[:, h // 3:h // 3 + 2, w // 3:w // 3 + 5] = 1
    if h * w > 40:
        m[rng.random((n, h, w)) < 0.02] = 1
    if h > 8 and w > 24:
        # where the planted values of object_image and fit_stack lie, and one corner inside the border
        m[:, h // 2 - 1:h // 2 + 2, 3:24] = 0
        m[:, 3:6, 3:6] = 0
    return m


def flat_field(shape, seed):
    """a flat field for the object step: (0.3, 1), a block of exact zeros, a negative value, a NaN
    and an inf"""
    rng = np.random.default_rng(seed)
    h, w = shape
    ff = rng.uniform(0.3, 1.0, (h, w))
    if h * w > 40:
        ff[h // 2, 10:16] = 0.0
        if h > 2:
            ff[h // 2 + 1, 10:16] = 0.0
        ff[1, 20], ff[1, 30], ff[1, 40] = -0.4, np.nan, np.inf
    return ff


def object_image(shape, dtype, seed):
    """an object for the flat-field step in the units of the fits: zeros under positive fits, under
    the fits' zero block and (float types) under their negative value"""
    rng = np.random.default_rng(seed)
    h, w = shape
    obj = rng.uniform(0.4, 1.2, (h, w)) * top_of(dtype)
    if h * w > 40:
        obj[h // 2, 5] = 0.0      # fit 0 there: 0 / 0
        obj[h // 2, 12] = 0.0     # the negative fit value of the float types
        obj[h // 2 - 1, 20] = 0.0   # a positive fit
    return obj


# ------------------------------------------------------------------ the loop scene
def vignetting(shape):
    h, w = shape
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    r2 = ((y - 0.48 * h) / h) ** 2 + ((x - 0.53 * w) / w) ** 2
    return np.clip(1.0 - 1.6 * r2, 0.0, 1.0)


def _object_at(px, py):
    return 0.6 + 0.3 * np.sin(px / 5.0) * np.cos(py / 7.0)


_scenes = {}


def loop_scene(ff_shape=(60, 80), obj_shape=(30, 40), n=6, seed=1, dtype=np.float64):
    """-> dict: fits (n, oh, ow), masks (bool), Hs, imgs (n, fh, fw), img_masks (bool), ff0 (a start
    for the flat field).  Image k shows the object O at homography Hs[k] (object pixel -> image
    pixel: +-4 degrees, scale 0.95 - 1.05, small perspective terms) under the vignetting V:
    fit_k(p) = O(p) V(Hs[k] p); masks: a 3-px border and wherever the image does not show the
    object."""
    key = (ff_shape, obj_shape, n, seed, np.dtype(dtype).name)
    if key in _scenes:
        return _scenes[key]
    rng = np.random.default_rng(seed)
    fh, fw = ff_shape
    oh, ow = obj_shape
    V = vignetting(ff_shape)
    top = {np.dtype(np.uint8): 250.0, np.dtype(np.uint16): 4000.0}.get(np.dtype(dtype), 1.0)
    py, px = np.mgrid[0:oh, 0:ow].astype(np.float64)
    qy, qx = np.mgrid[0:fh, 0:fw].astype(np.float64)
    fits, masks, Hs, imgs, img_masks = [], [], [], [], []
    for _ in range(n):
        a = np.deg2rad(rng.uniform(-4, 4))
        s = rng.uniform(0.95, 1.05)
        cx, cy = 0.5 * (ow - 1), 0.5 * (oh - 1)
        tx = rng.uniform(3, fw - ow * 1.05 - 3) + cx
        ty = rng.uniform(3, fh - oh * 1.05 - 3) + cy
        c, si = s * np.cos(a), s * np.sin(a)
        H = np.array([[c, -si, tx - c * cx + si * cy], [si, c, ty - si * cx - c * cy],
                      [rng.uniform(-1e-4, 1e-4), rng.uniform(-1e-4, 1e-4), 1.0]])
        W = H[2, 0] * px + H[2, 1] * py + H[2, 2]
        ix = (H[0, 0] * px + H[0, 1] * py + H[0, 2]) / W
        iy = (H[1, 0] * px + H[1, 1] * py + H[1, 2]) / W
        r2 = ((iy - 0.48 * fh) / fh) ** 2 + ((ix - 0.53 * fw) / fw) ** 2
        inside = (ix >= 0) & (ix <= fw - 1) & (iy >= 0) & (iy <= fh - 1)
        fit = np.where(inside, _object_at(px, py) * np.clip(1.0 - 1.6 * r2, 0, 1), 0.0) * top
        mask = ~inside
        mask[:3, :] = mask[-3:, :] = True
        mask[:, :3] = mask[:, -3:] = True
        Hi = np.linalg.inv(H)
        Wq = Hi[2, 0] * qx + Hi[2, 1] * qy + Hi[2, 2]
        ox = (Hi[0, 0] * qx + Hi[0, 1] * qy + Hi[0, 2]) / Wq
        oy = (Hi[1, 0] * qx + Hi[1, 1] * qy + Hi[1, 2]) / Wq
        shown = (ox >= 0) & (ox <= ow - 1) & (oy >= 0) & (oy <= oh - 1)
        img = np.where(shown, _object_at(ox, oy) * V, 0.0) * top
        if np.dtype(dtype).kind != 'f':
            fit, img = np.round(fit), np.round(img)
        fits.append(fit.astype(dtype))
        imgs.append(img.astype(dtype))
        masks.append(mask)
        img_masks.append(shown & (ox >= 3) & (ox <= ow - 4) & (oy >= 3) & (oy <= oh - 4))
        Hs.append(H)
    y, x = np.mgrid[0:fh, 0:fw].astype(np.float64)
    ff0 = np.clip(1.0 - 0.8 * (((y - 0.5 * fh) / fh) ** 2 + ((x - 0.5 * fw) / fw) ** 2), 0, 1)
    out = dict(fits=np.stack(fits), masks=np.stack(masks), Hs=np.stack(Hs), imgs=np.stack(imgs),
               img_masks=np.stack(img_masks), ff0=ff0)
    for a in out.values():
        a.setflags(write=False)
    _scenes[key] = out
    return out
