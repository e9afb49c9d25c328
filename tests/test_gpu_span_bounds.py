"""Where the calibration entry points draw the line between "next to" and "overlapping": an output
that starts on the first element after the input is served and gives the bits of a call on separate
buffers, one element earlier is IPA_ERR_BAD_ARG; frames one element closer than a frame is long
are refused for a stack and accepted for a single frame.  Through the C ABI, on 5 x 70 float64
frames, 3 to a stack, carved by offsets out of one allocation.  A refused call launches nothing."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, H, W = 3, 5, 70
FRAME = H * W          # elements of a frame, rows packed
STACK = N * FRAME      # the first element after a packed stack
NLF = (2.0, 0.0, 0.5)


@pytest.fixture(scope='module')
def ctx():
    import imgprocessor_amd
    return imgprocessor_amd.default_context(0)


class Arena(object):
    """one allocation of float64 elements that starts with `head` and is -1 behind it"""

    def __init__(self, ctx, head, total):
        host = np.full(total, -1.0)
        host[:head.size] = head.ravel()
        self.d = ctx.to_device(host)

    def at(self, i):
        return C.c_void_p(self.d.ptr.value + 8 * i)

    def get(self, i, shape):
        n = int(np.prod(shape))
        return self.d.get()[i:i + n].reshape(shape)


def frames(seed, n=N):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([100.0 + x + 3 * y + rng.normal(0, 2, (H, W)) for _ in range(n)])


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def test_ste(ctx):
    from imgprocessor_amd import DeviceArray, _lib as L
    st = frames(1)
    st[2, 2, 30:33] += 500.0
    a = Arena(ctx, st, STACK + FRAME)
    nlf = L.dbl(NLF, 3)

    def state():
        return DeviceArray(ctx, (H, W), np.float64), DeviceArray.counts(ctx, (H, W)), DeviceArray(ctx, (H, W), np.float64)

    def call(avg, cnt, thr, n=N, first=1, stride=FRAME):
        return ctx._lib.ipa_ste_dev(ctx.handle, a.at(0), L.F64, n, H, W, W, stride, first, nlf if first else None, 4.0,
                                    avg, cnt.ptr, thr.ptr, W, None, None, None, W)

    avg, cnt, thr = state()
    assert call(avg.ptr, cnt, thr) == L.OK
    want = avg.get(), cnt.get(), thr.get()
    assert np.count_nonzero(want[1] == 2) == 3 and np.count_nonzero(want[1] == 3) == FRAME - 3, 'the planted effect'
    _, cnt, thr = state()
    assert call(a.at(STACK - 1), cnt, thr) == L.ERR_BAD_ARG
    assert same(a.get(STACK, (H, W)), np.full((H, W), -1.0)), 'a refused call writes nothing'
    assert call(a.at(STACK), cnt, thr) == L.OK
    assert same(a.get(STACK, (H, W)), want[0]) and same(cnt.get(), want[1]) and same(thr.get(), want[2])
    assert same(a.get(0, st.shape), st)
    # frames one element closer than a frame is long
    avg, cnt, thr = state()
    assert call(avg.ptr, cnt, thr, stride=FRAME - 1) == L.ERR_BAD_ARG
    avg, cnt, thr = ctx.to_device(want[0]), DeviceArray.counts(ctx, (H, W)), ctx.to_device(want[2])
    cnt.set(want[1])
    assert call(avg.ptr, cnt, thr, n=1, first=0, stride=FRAME - 1) == L.OK
    ctx.synchronize()


def test_nl_means(ctx):
    from imgprocessor_amd import DeviceArray, _lib as L
    st = frames(2) / 200.0
    a = Arena(ctx, st, 2 * STACK)

    def call(dst, n=N, stride=FRAME):
        return ctx._lib.ipa_nl_means_dev(ctx.handle, a.at(0), L.F64, n, H, W, W, stride, 3, 2, 0.1, 0.0, dst, W, FRAME)

    out = DeviceArray(ctx, (N, H, W), np.float64)
    assert call(out.ptr) == L.OK
    want = out.get()
    assert call(a.at(STACK - 1)) == L.ERR_BAD_ARG
    assert same(a.get(STACK, st.shape), np.full(st.shape, -1.0)), 'a refused call writes nothing'
    assert call(a.at(STACK)) == L.OK
    assert same(a.get(STACK, st.shape), want) and same(a.get(0, st.shape), st)
    assert call(out.ptr, stride=FRAME - 1) == L.ERR_BAD_ARG
    assert call(out.ptr, n=1, stride=FRAME - 1) == L.OK
    assert same(out.get()[0], want[0])


def test_nlf_signal(ctx):
    from imgprocessor_amd import DeviceArray, _lib as L
    img = frames(3, 1)[0]
    a = Arena(ctx, img, 2 * FRAME)

    def call(sig):
        return ctx._lib.ipa_nlf_signal_dev(ctx.handle, a.at(0), L.F64, None, H, W, W, 0, None, 0, 1.5, sig, W)

    out = DeviceArray(ctx, (H, W), np.float64)
    assert call(out.ptr) == L.OK
    want = out.get()
    assert call(a.at(FRAME - 1)) == L.ERR_BAD_ARG
    assert same(a.get(FRAME, (H, W)), np.full((H, W), -1.0)), 'a refused call writes nothing'
    assert call(a.at(FRAME)) == L.OK
    assert same(a.get(FRAME, (H, W)), want) and same(a.get(0, (H, W)), img)


def test_snr_map(ctx):
    """the map may be the signal itself; the array it must stay clear of is the noise"""
    from imgprocessor_amd import DeviceArray, _lib as L
    sig, noise = frames(4, 1)[0], 1.0 + frames(5, 1)[0] / 50.0
    d_sig = ctx.to_device(sig)
    a = Arena(ctx, noise, 2 * FRAME)

    def call(snr):
        return ctx._lib.ipa_snr_map_dev(ctx.handle, d_sig.ptr, H, W, W, None, a.at(0), W, 0.0, 0.5 ** 0.5, 3.0, snr, W)

    out = DeviceArray(ctx, (H, W), np.float64)
    assert call(out.ptr) == L.OK
    want = out.get()
    assert call(a.at(FRAME - 1)) == L.ERR_BAD_ARG
    assert same(a.get(FRAME, (H, W)), np.full((H, W), -1.0)), 'a refused call writes nothing'
    assert call(a.at(FRAME)) == L.OK
    assert same(a.get(FRAME, (H, W)), want) and same(a.get(0, (H, W)), noise)


def test_stack_linregress(ctx):
    """a line needs two frames, so there is no single-frame call to accept"""
    from imgprocessor_amd import DeviceArray, _lib as L
    st = frames(6) + np.arange(N)[:, None, None] * 7.0
    a = Arena(ctx, st, STACK + FRAME)
    times = L.dbl([1.0, 2.0, 4.0], 3)

    def call(offset, ascent, error, stride=FRAME):
        return ctx._lib.ipa_stack_linregress_dev(ctx.handle, a.at(0), L.F64, N, H, W, W, stride, times, 1e6, 0.001,
                                                 offset, ascent.ptr, error.ptr, W)

    outs = [DeviceArray(ctx, (H, W), np.float64) for _ in range(3)]
    assert call(outs[0].ptr, outs[1], outs[2]) == L.OK
    want = [o.get() for o in outs]
    asc, err = DeviceArray(ctx, (H, W), np.float64), DeviceArray(ctx, (H, W), np.float64)
    assert call(a.at(STACK - 1), asc, err) == L.ERR_BAD_ARG
    assert same(a.get(STACK, (H, W)), np.full((H, W), -1.0)), 'a refused call writes nothing'
    assert call(a.at(STACK), asc, err) == L.OK
    assert same(a.get(STACK, (H, W)), want[0]) and same(asc.get(), want[1]) and same(err.get(), want[2])
    assert same(a.get(0, st.shape), st)
    assert call(outs[0].ptr, outs[1], outs[2], stride=FRAME - 1) == L.ERR_BAD_ARG
