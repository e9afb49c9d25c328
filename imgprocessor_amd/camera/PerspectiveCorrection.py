"""Perspective correction (homography warp) on MI355X behind the call surface of
the reference's ``imgProcessor.camera.PerspectiveCorrection.PerspectiveCorrection``
(reference: imgProcessor/camera/PerspectiveCorrection.py — __init__ :39-91,
setReference :97-131, homography :133-191, correctGrid :281-372, uncorrect :374-378,
correct :380-406, correctPoints :408-414).

On the hot path: the warp itself (``correct`` = cv2.warpPerspective with
INTER_LANCZOS4, ``uncorrect`` = INTER_CUBIC | WARP_INVERSE_MAP) runs as a HIP
gather kernel that evaluates the homography per pixel in float64 — no map
arrays, 8 B/px of HBM traffic for float32.  ``correctGrid`` — one
cv2.warpPerspective per lattice cell in the reference, 60 calls for a 6 x 10
module — is ONE launch of the same kernel: every output pixel looks up the cell
that owns it and evaluates that cell's homography (``ops.warp_grid``).

Outside the accelerated path (raises NotImplementedError when requested):
pose estimation (solvePnP), tilt-intensity correction, reference-image
homographies from feature matching.  ``new_size=(sy, sx)`` must be given
explicitly; the reference's None-size branch needs the pose code and is
ill-defined.
"""
from __future__ import print_function

import numpy as np

from .. import ops
from ..device import DeviceArray, default_context
from ..utils.geometry import (genericCameraMatrix, sortCorners, getPerspectiveTransform,
                              perspectiveTransform)

_CV_BORDER = {0: 'constant', 1: 'replicate', 2: 'reflect', 3: 'wrap', 4: 'reflect101'}


class PerspectiveCorrection(object):

    def __init__(self, img_shape, cameraMatrix=None, distCoeffs=np.zeros((5, 1)),
                 do_correctIntensity=False, px_per_phys_unit=None, new_size=(None, None),
                 in_plane=False, border=0, maxShear=0.05, material='EL_Si_module', cv2_opts={},
                 interpolation=None, ctx=None):
        if do_correctIntensity:
            raise NotImplementedError('tilt-intensity correction (pose + emissivity model) is '
                                      'outside the accelerated hot path')
        self.opts = {'distCoeffs': np.asarray(distCoeffs).astype(np.float32),
                     'do_correctIntensity': False, 'new_size': new_size, 'in_plane': in_plane,
                     'cv2_opts': dict(cv2_opts), 'border': border, 'material': material,
                     'maxShear': maxShear, 'shape': tuple(img_shape[:2])}
        if cameraMatrix is None:
            cameraMatrix = genericCameraMatrix(img_shape)
        self.opts['cameraMatrix'] = np.asarray(cameraMatrix).astype(np.float32)
        self.refQuad = None
        self.quad = None
        self.px_per_phys_unit = px_per_phys_unit
        self._newBorders = self.opts['new_size']
        self._homography = None
        self._homography_is_fixed = True
        self.interpolation = interpolation  # None = the reference's flags per method
        self._ctx = ctx
        self.img = None

    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = default_context()
        return self._ctx

    def setReferenceQuad(self, refQuad):
        self.refQuad = sortCorners(refQuad)

    def setReference(self, ref):
        """ref: 3x3 homography, or the four (x,y) corners of the quad to rectify"""
        self.quad = None
        self._homography = None
        self._homography_is_fixed = True
        if isinstance(ref, np.ndarray) and ref.shape == (3, 3):
            self._homography = ref.astype(np.float64)
        elif len(ref) == 4:
            self.quad = sortCorners(ref)
        else:
            raise NotImplementedError('reference IMAGES need feature matching '
                                      '(ORB + RANSAC), outside the accelerated hot path')

    def _size(self):
        sy, sx = self._newBorders
        if sy is None or sx is None:
            raise NotImplementedError('new_size=(sy, sx) must be given explicitly '
                                      '(the aspect-ratio-from-pose branch is not implemented)')
        return int(sy), int(sx)

    @property
    def homography(self):
        if self._homography is None:
            if self.quad is None:
                raise RuntimeError('call setReference(quad or 3x3 homography) first')
            b = self.opts['border']
            if self.refQuad is not None:
                dst = self.refQuad.astype(np.float32)
            else:
                sy, sx = self._size()
                dst = np.float32([[b, b], [sx - b, b], [sx - b, sy - b], [b, sy - b]])
            self._homography = getPerspectiveTransform(self.quad.astype(np.float32), dst)
        return self._homography

    # ------------------------------------------------------------------
    def _border_kw(self):
        o = self.opts['cv2_opts']
        mode = o.get('borderMode', 0)
        mode = _CV_BORDER.get(mode, mode)
        val = o.get('borderValue', 0)
        if np.ndim(val):
            val = np.ravel(val)[0]
        return mode, float(val)

    def _warp(self, img, M_dst2src, out_shape, interpolation, border=None):
        mode, val = self._border_kw() if border is None else border

        def run(d):
            return ops.warp_perspective(d, M_dst2src, out_shape, interpolation, mode, val)
        return self._on_device(img, run)

    def _on_device(self, img, run):
        if isinstance(img, DeviceArray):
            return run(img)
        img = np.asarray(img)
        if img.ndim == 3:   # (H, W, C): the layout copies both ways run on the device
            return ops.from_planes(run(ops.to_planes(img, ctx=self.ctx))).get()
        return run(self.ctx.to_device(img)).get()

    def correct(self, img):
        """perspective-rectify `img` into new_size=(sy,sx) — :380-406
        (cv2.warpPerspective(img, H, (sx,sy), flags=INTER_LANCZOS4))"""
        print("CORRECT PERSPECTIVE ...")
        self.img = img
        H = self.homography
        sy, sx = self._size()
        Minv = np.linalg.inv(np.asarray(H, dtype=np.float64))
        return self._warp(img, Minv, (sy, sx), self.interpolation or 'lanczos4')

    def _gridCells(self, grid):
        """the cells of correctGrid in the reference's paint order (:317-371), host only:
        -> (rects int32 (n, 4): x0, y0, w, h in the output; M float64 (n, 9): the cell's matrix from
        its LOCAL destination pixel to the source, inv(getPerspectiveTransform(quad, objP)))"""
        grid = np.asarray(grid)
        if grid.ndim != 3 or grid.shape[2] != 2 or grid.shape[0] < 2 or grid.shape[1] < 2:
            raise ValueError('grid must have shape (s0, s1, 2) with s0, s1 >= 2 (got %s)'
                             % (grid.shape,))
        n0, n1 = grid.shape[0] - 1, grid.shape[1] - 1
        W, H = self._size()   # read as (width, height) here, see correctGrid
        b = int(self.opts['border'])
        sx, sy = (W - 2 * b) // n0, (H - 2 * b) // n1
        if sx < 1 or sy < 1:
            raise ValueError('new_size %s with border %d leaves no room for %d x %d cells'
                             % ((W, H), b, n0, n1))
        rects, mats = [], []

        def cell(ix, iy, rows, cols, off):
            # the view out[rows, cols], clipped as a numpy slice is; the matrix acts on its pixels
            y0, y1, _ = slice(*rows).indices(H)
            x0, x1, _ = slice(*cols).indices(W)
            if y1 <= y0 or x1 <= x0:
                return
            quad = grid[ix:ix + 2, iy:iy + 2].reshape(4, 2)[[0, 2, 3, 1]].astype(np.float32)
            objP = np.float32([[0, 0], [sx, 0], [sx, sy], [0, sy]]) + np.float32(off)
            hcell = getPerspectiveTransform(quad, objP)
            rects.append((x0, y0, x1 - x0, y1 - y0))
            mats.append(np.linalg.inv(hcell).ravel())

        xr = (n0 - 1) * sx + b
        for ix in range(1, n0 - 1):                      # inner cells
            for iy in range(1, n1 - 1):
                cell(ix, iy, (iy * sy + b, (iy + 1) * sy + b), (ix * sx + b, (ix + 1) * sx + b), (0, 0))
        for ix in range(1, n0 - 1):                      # top
            cell(ix, 0, (None, sy + b), (ix * sx + b, (ix + 1) * sx + b), (0, b))
        for ix in range(1, n0 - 1):                      # bottom
            y, x = (n1 - 1) * sy + b, ix * sx + b
            cell(ix, n1 - 1, (y, y + sy + b), (x, x + sx), (0, 0))
        for iy in range(1, n1 - 1):                      # left
            y = iy * sy + b
            cell(0, iy, (y, y + sy), (None, sx + b), (b, 0))
        for iy in range(1, n1 - 1):                      # right
            y = iy * sy + b
            cell(n0 - 1, iy, (y, y + sy), (xr, xr + sx + b), (0, 0))
        # the corners; the -1 is the reference's (:361, :371): the two bottom ones start one row
        # early, their content sits one row lower
        cell(n0 - 1, n1 - 1, (-sy - b - 1, None), (xr, xr + sx + b), (0, 0))
        cell(0, 0, (0, sy + b), (0, sx + b), (b, b))
        cell(n0 - 1, 0, (None, sy + b), (xr, xr + sx + b), (0, b))
        cell(0, n1 - 1, (-sy - b - 1, None), (None, sx + b), (b, 0))
        return (np.array(rects, dtype=np.int32).reshape(-1, 4),
                np.array(mats, dtype=np.float64).reshape(-1, 9))

    def correctGrid(self, img, grid):
        """rectify an object whose cell lattice is known - :281-372.  grid: (s0, s1, 2) source
        points (x, y); every lattice cell is warped by its own homography into its own rectangle
        of the output (cv2.warpPerspective(img, hcell, ..., flags=INTER_LANCZOS4) per cell in the
        reference; here one launch, bit for bit the per-cell warps pasted in the same order).

        As in the reference, new_size is read as (width, height) in THIS method and grid axis 0
        runs along x: the output has shape new_size[::-1], the transpose of what correct()
        returns for a non-square new_size.  The reference's off-by-one in the two bottom corner
        cells is kept.  Pixels no cell covers (np.empty in the reference) receive the border
        value.  No setReference() is needed: new_size is explicit.  The tilt-intensity division
        is outside the accelerated path (do_correctIntensity raises in the constructor)."""
        self.img = img
        rects, M = self._gridCells(grid)
        W, H = self._size()
        mode, val = self._border_kw()
        interpolation = self.interpolation or 'lanczos4'

        def run(d):
            return ops.warp_grid(d, rects, M, (H, W), interpolation, mode, val)
        return self._on_device(img, run)

    def uncorrect(self, img):
        """inverse warp back into an image of img's own shape — :374-378
        (flags=INTER_CUBIC | WARP_INVERSE_MAP: H itself maps destination -> source)"""
        s = img.shape[-2:] if isinstance(img, DeviceArray) else np.shape(img)[:2]
        # the reference passes only `flags` here: cv2's default border (constant 0), not cv2_opts
        return self._warp(img, np.asarray(self.homography, dtype=np.float64), tuple(s),
                          self.interpolation or 'cubic_cv_q5', border=('constant', 0.0))

    def distort(self, img, rotX=0, rotY=0, quad=None):
        """apply a perspective distortion: rectify `img` (correct), warp the result into `quad`
        and paste it centred into a zero image of img's shape - :193-270, the warp at :241-242
        (cv2.warpPerspective(corr, H, (w, h), flags=INTER_CUBIC | WARP_INVERSE_MAP)).
        Only the explicit-quad form is on the accelerated path: without `quad` the reference
        projects the stored quad through a pose (rotX / rotY), which needs its 3-D point and
        solvePnP code."""
        if quad is None:
            raise NotImplementedError('distort() without quad needs the pose / 3-D projection '
                                      'code, outside the accelerated hot path')
        if isinstance(img, DeviceArray):
            img = img.get()
        img = np.asarray(img)
        self.img = img
        corr = self.correct(img)
        s = img.shape
        wquad = sortCorners(quad)
        wquad -= wquad.min(axis=0)
        lx, ly = corr.shape[1], corr.shape[0]
        objP = np.array([[0, 0], [lx, 0], [lx, ly], [0, ly]], dtype=np.float32)
        homography = getPerspectiveTransform(wquad.astype(np.float32), objP)
        w = wquad[:, 0].max() - wquad[:, 0].min()
        h = wquad[:, 1].max() - wquad[:, 1].min()
        # WARP_INVERSE_MAP: the matrix itself maps destination -> source
        dist = self._warp(corr, np.asarray(homography, dtype=np.float64), (int(h), int(w)),
                          self.interpolation or 'cubic_cv_q5', border=('constant', 0.0))
        # move the middle of dist to the middle of the image
        bg = np.zeros(shape=s)
        rmn = (bg.shape[0] / 2, bg.shape[1] / 2)
        ss = dist.shape
        mn = (ss[0] / 2, ss[1] / 2)
        ref = (int(rmn[0] - mn[0]), int(rmn[1] - mn[1]))
        bg[ref[0]:ss[0] + ref[0], ref[1]:ss[1] + ref[1]] = dist
        # finally move the quad into position (the reference re-estimates its pose here too;
        # that call is outside the accelerated path and is not made)
        self.quad = wquad
        self.quad += (ref[1], ref[0])
        self.img = bg
        self._homography = None
        return self.img

    def correctPoints(self, pts):
        """cv2.perspectiveTransform(pts, H) — :408-414"""
        pts = np.asarray(pts)
        if pts.ndim == 2:
            pts = pts.reshape(1, *pts.shape)
        return perspectiveTransform(pts.astype(np.float32), self.homography).astype(np.float32)
