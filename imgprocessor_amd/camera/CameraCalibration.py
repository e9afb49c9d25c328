"""``CameraCalibration`` — reference: imgProcessor/camera/CameraCalibration.py.

The calibration container (``coeffs`` dict, ``add*``, ``.cal`` pickle I/O,
date lookup) and the per-frame ``correct`` chain the lens-distortion hot path
sits in (reference :351-459):

    2. dark current   image -= bg                         (:476-505)
    3. flat field     image[ff != 0] /= ff[ff != 0]       (:521-528)
    4. artefacts      nan_to_num + medianThreshold(3x3)   (:561-568)
    5. lens           LensDistortion(coeffs).correct()    (:574-579)

Stages 2-4 run as ONE HIP kernel (``ipa_calib_prefilter_dev``), stage 5 as the
remap kernel on the same device buffer: a frame crosses PCIe once each way.

Kept as written in the reference:
  * ``calcDarkCurrent`` tests ``type(d) == tuple`` on the list entry
    ``[date, info, data, error]`` (:509), so the slope/intercept model is never
    evaluated and ``bg`` is ``data`` itself: an array works, a ``(slope,
    intercept)`` tuple makes ``image -= bg`` fail, which ``correct`` reports
    as ``Error: ...`` and skips (:418-422) — same here;
  * every stage's lookup errors are printed and the stage skipped (:416-447);
  * ``.cal`` files are plain pickles of ``coeffs`` (:305-322); files written by
    the reference load here and vice versa (lens entries are coefficient dicts).

Not on the GPU path (NotImplementedError, no CPU fallback): single-time-effect
removal for image stacks (:388-408) and ``deblur`` (:439-444).  ``denoise`` (:456-474)
runs on the device (ops.nl_means).
The reference always promotes the frame to float64 (:408-410); ``dtype=`` lets
a caller keep float32 frames (half the HBM traffic) — an extension.

A ``noise`` entry (``addNoise(nlf_coeff)``) is the (minY, ax, ay) triple of
NoiseLevelFunction.boundedFunction.  To obtain one from frames:
``NoiseLevelFunction.oneImageNLF(img)[0].triple`` (one frame, or two exposures
of the same scene), or ``estimateFromImages(imgs1, imgs2)[5]`` over several
pairs — the frame passes run on the device (csrc/nlf.hip).
"""
from __future__ import print_function

import pickle
import time

import numpy as np

from .. import ops
from ..device import DeviceArray
from .LensDistortion import LensDistortion

DATE_FORMAT = "%d %b %y - %H:%M"  # the reference's date strings, e.g. '30 Nov 15 - 13:20' (:16)

# light-dependent sections of `coeffs` ({light: history}) and the plain histories; a history is a
# list of entries [date, info, data(, error)] kept NEWEST FIRST (the order `.cal` files store)
_BY_LIGHT = ('flat field', 'lens', 'psf', 'balance')
_PLAIN = ('dark current', 'noise')


def _stamp(date):
    """time.struct_time of a date string in DATE_FORMAT; None = now"""
    return time.localtime() if date is None else time.strptime(date, DATE_FORMAT)


class _History(object):
    """view of one newest-first entry list of `coeffs` (the list itself stays what is pickled)"""

    def __init__(self, entries):
        self.entries = entries

    def slot(self, stamp):
        """position that keeps the order when an entry dated `stamp` is inserted (:29-34)"""
        pos = 0
        while pos < len(self.entries) and not self.entries[pos][0] < stamp:
            pos += 1
        return pos

    def add(self, stamp, *fields):
        self.entries.insert(self.slot(stamp), [stamp] + list(fields))

    def at(self, date):
        """the entry the reference picks for `date` (:37-49): the one in front of the insert
        position of `date` (the nearest calibration that is not older), the newest entry when
        `date` is None, unparsable or newer than everything stored"""
        try:
            pos = self.slot(time.strptime(date, DATE_FORMAT))
        except (ValueError, TypeError):
            return self.entries[0]
        return self.entries[pos - 1 if pos > 0 else 0]


class CameraCalibration(object):
    ftype = '.cal'

    def __init__(self, ctx=None):
        self._ctx = ctx
        self.noise_level_function = None
        self.coeffs = dict({'name': 'no camera', 'depth': 16, 'light spectra': [], 'shape': None},
                           **{k: [] for k in _PLAIN}, **{k: {} for k in _BY_LIGHT})
        self.temp = {}
        self._lens_cache = {}

    # ------------------------------------------------------------ bookkeeping --
    @staticmethod
    def currentTime():
        return time.strftime(DATE_FORMAT)

    def setCamera(self, camera_name, bit_depth=16):
        self.coeffs.update(name=camera_name, depth=bit_depth)

    def _history(self, typ, light=None, create=False):
        section = self.coeffs[typ]
        if isinstance(section, dict):
            assert light is not None, 'need light spectrum given to access [%s]' % typ
            if create:
                if light not in self.coeffs['light spectra']:
                    self.coeffs['light spectra'].append(light)
                section.setdefault(light, [])
            section = section[light]
        return _History(section)

    def dates(self, typ, light=None):
        try:
            return [time.strftime(DATE_FORMAT, e[0]) for e in self._history(typ, light).entries]
        except KeyError:
            return []

    def infos(self, typ, light=None, date=None):
        hist = self._history(typ, light)
        return [e[1] for e in hist.entries] if date is None else hist.at(date)[1]

    def _adopt_shape(self, *arrays):
        """the first array fixes the calibrated shape, every later one has to agree with it"""
        for a in arrays:
            if not isinstance(a, np.ndarray):
                continue
            known = self.coeffs['shape']
            if known is None:
                self.coeffs['shape'] = a.shape
            elif tuple(known[:2]) != a.shape[:2]:
                raise Exception('array shapes are different: stored(%s), given(%s)\n'
                                'if shapes are transposed, execute self.transpose() once '
                                % (known, a.shape))

    def addDarkCurrent(self, slope, intercept=None, date=None, info='', error=None):
        self._adopt_shape(slope, intercept)
        self._history('dark current').add(_stamp(date), info,
                                          slope if intercept is None else (slope, intercept), error)

    def addNoise(self, nlf_coeff, date=None, info='', error=None):
        self._history('noise').add(_stamp(date), info, nlf_coeff, error)

    def addDeconvolutionBalance(self, balance, date=None, info='', light_spectrum='visible'):
        self._history('balance', light_spectrum, create=True).add(_stamp(date), info, balance)

    def addPSF(self, psf, date=None, info='', light_spectrum='visible'):
        self._history('psf', light_spectrum, create=True).add(_stamp(date), info, psf)

    def addFlatField(self, arr, date=None, info='', error=None, light_spectrum='visible'):
        self._adopt_shape(arr)
        self._history('flat field', light_spectrum, create=True).add(_stamp(date), info, arr, error)

    def addLens(self, lens, date=None, info='', light_spectrum='visible'):
        """lens: a LensDistortion or the path of a saved one (:271-287); its coefficient dict is
        what the calibration keeps"""
        if not isinstance(lens, LensDistortion):
            path, lens = lens, LensDistortion(ctx=self._ctx)
            lens.readFromFile(path)
        self._history('lens', light_spectrum, create=True).add(_stamp(date), info, lens.coeffs)

    def clearOldCalibrations(self, date=None):
        """only the oldest entry of every history stays (:289-298)"""
        for k in _PLAIN:
            del self.coeffs[k][:-1]
        for k in ('flat field', 'lens'):
            for entries in self.coeffs[k].values():
                del entries[:-1]

    def _correctPath(self, path):
        return path if path.endswith(self.ftype) else path + self.ftype

    @staticmethod
    def loadFromFile(path, ctx=None):
        """a `.cal` file is the pickled `coeffs` dict (:305-316), python-2 pickles included"""
        cal = CameraCalibration(ctx=ctx)
        with open(cal._correctPath(path), 'rb') as f:
            blob = f.read()
        try:
            stored = pickle.loads(blob)
        except UnicodeDecodeError:
            stored = pickle.loads(blob, encoding='latin1')
        cal.coeffs.update(stored)
        return cal

    def saveToFile(self, path):
        path = self._correctPath(path)
        with open(path, 'wb') as f:
            f.write(pickle.dumps(dict(self.coeffs), protocol=pickle.HIGHEST_PROTOCOL))
        return path

    def transpose(self):
        """every stored array of the calibrated shape transposed, (slope, intercept) tuples turned
        into lists on the way, the shape reversed (:324-349)"""
        shape = self.coeffs['shape']
        pending = [v for v in self.coeffs.values() if type(v) == list]
        for section in self.coeffs.values():
            if type(section) == dict:
                pending.extend(section.values())
        while pending:
            seq = pending.pop()
            if type(seq) != list:
                continue
            for i, v in enumerate(seq):
                if type(v) == tuple:
                    v = seq[i] = list(v)
                if type(v) == list:
                    pending.append(v)
                elif isinstance(v, np.ndarray) and v.shape == shape:
                    seq[i] = v.T
        self.coeffs['shape'] = shape[::-1]

    def getCoeff(self, name, light=None, date=None):
        """the entry of `name` in force at `date` for `light` - for any other light (said so) when
        there is none for it, None when the section is empty (:583-604)"""
        section = self.coeffs[name]
        if isinstance(section, dict):
            if light not in section:
                if not section:
                    return None
                other = next(iter(section))
                if light is not None:
                    print('no calibration found for [%s] - using [%s] instead' % (light, other))
                light = other
            section = section[light]
        return _History(section).at(date)

    def calcDarkCurrent(self, exposuretime, date=None):
        entry = _History(self.coeffs['dark current']).at(date)
        if type(entry) != tuple:
            # what the reference's test on the ENTRY (:509) always yields for the lists
            # addDarkCurrent stores: the data as they are, the (slope, intercept) model never run
            return entry[2]
        offset, ascent = entry[2]
        limit = 2 ** self.coeffs['depth'] - 1
        with np.errstate(invalid='ignore'):
            return np.where(offset + ascent * exposuretime > limit, limit, offset + ascent * exposuretime)

    def getLens(self, light_spectrum, date):
        entry = self.getCoeff('lens', light_spectrum, date)
        if not entry:
            return None
        # one LensDistortion (and its device maps) per stored coefficient dict, kept between frames
        key = id(entry[2])
        if key not in self._lens_cache:
            self._lens_cache[key] = LensDistortion(entry[2], ctx=self._ctx)
        return self._lens_cache[key]

    # ----------------------------------------------------------------- correct --
    def correct(self, images, bgImages=None, exposure_time=None, light_spectrum=None,
                threshold=0.1, keep_size=True, date=None, deblur=False, denoise=False,
                dtype=np.float64, denoise_h=0.1):
        """denoise=True: after the lens stage NaN becomes 0 and the frame goes through non-local
        means with patch_size 7 and patch_distance 11 (:461-474), on the device.  denoise_h is
        the cut-off `h` of the weights in the frame's own units.  The reference always runs with
        skimage's default h = 0.1, under which a frame in camera counts comes back unchanged:
        every patch distance is beyond the cut-off and only the pixel itself keeps a weight.  Pass
        a denoise_h of the order of the noise level to denoise such a frame.  deblur=True is not
        part of the HIP path."""
        print('CORRECT CAMERA ...')
        if isinstance(date, str) or date is None:
            date = {k: date for k in ('dark current', 'flat field', 'lens', 'noise', 'psf')}
        if deblur:
            raise NotImplementedError('deblur is not part of the HIP path')
        if denoise:
            ops._nlm_args(7, 11, denoise_h, 0.0)
        if light_spectrum is None:
            try:
                light_spectrum = self.coeffs['light spectra'][0]
            except IndexError:
                pass

        dev_in = isinstance(images, DeviceArray)
        if not dev_in and (type(images) in (list, tuple) or
                           (isinstance(images, np.ndarray) and images.ndim == 3 and
                            images.shape[-1] not in (3, 4))):
            if len(images) > 1:
                raise NotImplementedError('single-time-effect removal of image stacks is not '
                                          'part of the HIP path: pass one frame')
            images = images[0]
        if dev_in:
            image = images
        else:
            image = np.asarray(images, dtype=dtype)
            if image.ndim != 2:
                raise ValueError('correct() takes one (H, W) frame')
        shape = tuple(image.shape)
        if self.coeffs['shape'] is None:
            self.coeffs['shape'] = shape
        elif tuple(self.coeffs['shape'][:2]) != shape[:2]:
            raise Exception('array shapes are different: stored(%s), given(%s)\n'
                            'if shapes are transposed, execute self.transpose() once '
                            % (self.coeffs['shape'], shape))
        self.last_light_spectrum = light_spectrum
        self.last_img = image
        fdtype = image.dtype

        def usable(a, what):
            a = np.asarray(a, dtype=fdtype)  # a (slope, intercept) tuple fails here or below
            np.broadcast_to(a, shape)
            return a

        # 2. dark current
        bg = None
        try:
            print('... remove dark current')
            if bgImages is not None:
                if type(bgImages) in (list, tuple) or (isinstance(bgImages, np.ndarray) and
                                                       bgImages.ndim == 3):
                    if len(bgImages) > 1:
                        raise NotImplementedError('single-time-effect removal of background '
                                                  'stacks is not part of the HIP path')
                    bgImages = bgImages[0]
                bg = bgImages
            else:
                bg = self.calcDarkCurrent(exposure_time, date['dark current'])
            self.temp['bg'] = bg
            bg = usable(bg, 'bg')
        except NotImplementedError:
            raise
        except Exception as errm:
            print('Error: %s' % errm)
            bg = None
        # 3. vignetting / sensitivity
        ff = None
        try:
            d = self.getCoeff('flat field', light_spectrum, date['flat field'])
            if d is not None:
                print('... remove vignetting and sensitivity')
                ff = usable(d[2], 'flat field')
        except Exception as errm:
            print('Error: %s' % errm)
            ff = None
        # 4. artefacts: fused with 2 and 3 in one kernel
        if threshold > 0:
            print('... remove artefacts')
        ctx = image.ctx if dev_in else (self._ctx or ops.default_context())
        d_img = image if dev_in else ctx.to_device(image)
        d_img = ops.calib_prefilter(d_img, bg, ff, threshold if threshold > 0 else 0.0, ctx=ctx)
        # 5. lens
        try:
            lens = self.getLens(light_spectrum, date['lens'])
        except Exception as errm:
            print('Error: %s' % errm)
            lens = None
        if lens:
            print('... correct lens distortion')
            d_img = lens.correct(d_img, keepSize=keep_size)
        # 7. denoise
        if denoise:
            print('... denoise ... this might take some time')
            d_img = ops.nl_means(ops.nan_to_zero(d_img), 7, 11, h=denoise_h)
        print('DONE')
        return d_img if dev_in else d_img.get()
