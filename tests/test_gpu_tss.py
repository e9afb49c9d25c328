"""GPU: temporal signal stability (csrc/tss.hip, uncertainty/temporalSignalStability.py) against
the numpy / scipy restatement (tests/tss_ref.py) and the reference's outputs (tests/golden/tss.npz).

The event kernel runs through the C ABI over the whole case table of tests/tss_cases.py - one
pixel, images smaller than the window, more than one tile in both directions with partial last
tiles; 2 to 64 frames; all four element types; the lattice, plane, border and continuous scenes -
with pitched rows, frames further apart than a frame and guard-valued padding that must come back
untouched.  The event cube, the raw event length and the zero mask are compared bit for bit with
scipy's median (tss_ref.events_median); d_events = NULL and d_zero_mask = NULL give the same
length.  ipa_tss_finish_dev is compared bit for bit with scipy's filters (it only selects).

temporalSignalStability: error, ascent and offset bit for bit, the zero pattern of the final
event length exactly, its non-zero values within rtol 1e-13, atol 1e-15 - what
tests/test_cpu_stencil_refs.py grants masked_mean in float64; the maximum and the median after the
mean only select and are 1-Lipschitz, so the mean's error passes through unamplified.
"""
import numpy as np
import pytest

from .conftest import load_golden
from . import tss_cases as tc
from . import tss_ref as ref
from .test_cpu_dark import same
from .test_cpu_tss import unpack
from .test_gpu_dark import DT_ID, ERR_BAD_ARG, ERR_UNSUPPORTED, GUARD, dptr, padded, planes, unpad

pytestmark = pytest.mark.gpu

BYTE_GUARD = 7
PLANE_FILL = 1e30   # padding of the input planes: a kernel that reads it decides wrongly


@pytest.fixture(scope='module')
def ctx():
    import imgprocessor_amd
    return imgprocessor_amd.default_context(0)


@pytest.fixture(scope='module')
def g():
    return load_golden('tss.npz')


def _ops():
    from imgprocessor_amd import ops
    return ops


def byte_plane(ctx, shape):
    return ctx.to_device(np.full(shape, BYTE_GUARD, np.uint8))


def unpad_bytes(d, w):
    a = d.get()
    assert np.all(a[..., w:] == BYTE_GUARD), 'the padding was written'
    return a[..., :w]


def event_length_abi(ctx, sc, with_events=True, with_mask=True, gap=1, T=None, dtype_id=None):
    """-> (status, d_avlen, d_mask, d_events) of one call with pitched rows and padded frames"""
    st, times, offset, ascent, error = sc
    n, h, w = st.shape
    T = n if T is None else T
    pitch, ppitch, apitch, mpitch, epitch = w + 3, w + 1, w + 2, w + 5, w + 4
    host = np.concatenate([padded(st, pitch), np.zeros((n, gap, pitch), st.dtype)], axis=1)
    d_st = ctx.to_device(host)
    d_p = [ctx.to_device(padded(np.ascontiguousarray(a, dtype=np.float64), ppitch, PLANE_FILL))
           for a in (offset, ascent, error)]
    d_avlen, = planes(ctx, 1, h, apitch)
    d_mask = byte_plane(ctx, (h, mpitch))
    d_ev = byte_plane(ctx, (n, h + gap, epitch))
    t = np.ascontiguousarray(np.resize(np.asarray(times, dtype=np.float64), max(T, 1)))
    rc = ctx._lib.ipa_tss_event_length_dev(
        ctx.handle, d_st.ptr, DT_ID[st.dtype] if dtype_id is None else dtype_id, T, h, w, pitch, (h + gap) * pitch,
        dptr(t), d_p[0].ptr, d_p[1].ptr, d_p[2].ptr, ppitch, d_avlen.ptr, apitch,
        d_mask.ptr if with_mask else None, mpitch, d_ev.ptr if with_events else None, epitch, (h + gap) * epitch)
    return rc, d_avlen, d_mask, d_ev


# ------------------------------------------------------------------ the event kernel
@pytest.mark.parametrize('T', tc.T_VALUES)
def test_event_length_over_the_case_table(ctx, T):
    for i, (kind, shape, dt, v) in enumerate(tc.case_ids(T)):
        what = (kind, T, shape, np.dtype(dt).name, v)
        sc = tc.scene(kind, T, shape, dt, v)
        want_evt, want_raw = tc.reference(kind, T, shape, dt, v)
        h, w = shape
        rc, d_avlen, d_mask, d_ev = event_length_abi(ctx, sc, gap=1 + i % 2)
        ctx._check(rc, 'tss_event_length')
        ev = unpad_bytes(d_ev, w)
        assert np.all(ev[:, h:] == BYTE_GUARD), 'the gap between the event frames was written'
        got_evt = ev[:, :h]
        assert np.array_equal(got_evt, want_evt.astype(np.uint8)), \
            (what, 'events', int((got_evt != want_evt).sum()), np.argwhere(got_evt != want_evt)[:4].tolist())
        avlen = unpad(d_avlen, w)
        assert same(avlen, want_raw), (what, 'avlen')
        assert np.array_equal(unpad_bytes(d_mask, w), (want_raw == 0).astype(np.uint8)), (what, 'mask')
        # without the optional outputs: the same length, nothing else written
        rc, d_avlen, d_mask, d_ev = event_length_abi(ctx, sc, with_events=False, with_mask=False)
        ctx._check(rc, 'tss_event_length')
        assert same(unpad(d_avlen, w), want_raw), (what, 'avlen without events')
        assert np.all(d_mask.get() == BYTE_GUARD) and np.all(d_ev.get() == BYTE_GUARD)


def test_event_length_refusals(ctx):
    lib = ctx._lib
    sc = tc.scene('lattice', 4, (3, 4), np.float32, 0)
    st = sc[0]

    def untouched(outs):
        ctx.synchronize()
        d_avlen, d_mask, d_ev = outs
        return (np.all(d_avlen.get() == GUARD) and np.all(d_mask.get() == BYTE_GUARD) and
                np.all(d_ev.get() == BYTE_GUARD))

    rc, *outs = event_length_abi(ctx, sc, T=1)
    assert rc == ERR_BAD_ARG and untouched(outs)
    big = (np.zeros((65, 3, 4), np.float32),) + tuple(sc[1:])
    rc, *outs = event_length_abi(ctx, big, T=65)
    assert rc == ERR_UNSUPPORTED and untouched(outs)
    rc, *outs = event_length_abi(ctx, sc, dtype_id=7)
    assert rc == ERR_UNSUPPORTED and untouched(outs)
    # null pointers, an empty image, pitches, overlaps: straight through the ABI
    T, h, w = st.shape
    d_st = ctx.to_device(np.ascontiguousarray(st, np.float64))
    d_p = [ctx.to_device(np.ascontiguousarray(a, np.float64)) for a in sc[2:]]
    d_avlen, = planes(ctx, 1, h, w)
    d_mask, d_ev = byte_plane(ctx, (h, w)), byte_plane(ctx, (T, h, w))
    t = np.ascontiguousarray(sc[1], dtype=np.float64)

    def call(stack=d_st.ptr, off=d_p[0].ptr, asc=d_p[1].ptr, err=d_p[2].ptr, avlen=d_avlen.ptr, mask=d_mask.ptr,
             ev=d_ev.ptr, hh=h, ww=w, pitch=w, ppitch=w, apitch=w, mpitch=w, epitch=w, fstride=h * w,
             estride=h * w, times=dptr(t)):
        return lib.ipa_tss_event_length_dev(ctx.handle, stack, 3, T, hh, ww, pitch, fstride, times, off, asc, err,
                                            ppitch, avlen, apitch, mask, mpitch, ev, epitch, estride)
    for kw in (dict(stack=None), dict(off=None), dict(asc=None), dict(err=None), dict(avlen=None),
               dict(times=None), dict(hh=0), dict(ww=0), dict(pitch=w - 1), dict(ppitch=w - 1),
               dict(apitch=w - 1), dict(mpitch=w - 1), dict(epitch=w - 1), dict(fstride=h * w - 1),
               dict(estride=h * w - 1),
               dict(avlen=d_p[2].ptr), dict(avlen=d_st.ptr), dict(mask=d_ev.ptr), dict(ev=d_st.ptr),
               dict(mask=d_p[0].ptr)):
        assert call(**kw) == ERR_BAD_ARG, kw
    assert untouched((d_avlen, d_mask, d_ev))
    assert call() == 0
    want_evt = ref.events_median(*sc)
    assert np.array_equal(d_ev.get(), want_evt.astype(np.uint8))
    assert same(d_avlen.get(), ref.run_lengths(want_evt))


# ------------------------------------------------------------------ the 2-D tail
FIN_MULTI = (2 * tc.FIN_TILE_H + 3, 2 * tc.FIN_TILE_W + 5)
FIN_SHAPES = ((1, 1), (3, 4), (5, 37), FIN_MULTI)


def finish_masks(h, w):
    """all clear, all set, single pixels on the corners, the edges and both sides of every tile
    border, a random one"""
    yield 'clear', np.zeros((h, w), bool)
    yield 'set', np.ones((h, w), bool)
    ys = sorted({0, h // 2, h - 1} | {y for b in range(tc.FIN_TILE_H, h, tc.FIN_TILE_H) for y in (b - 1, b)})
    xs = sorted({0, w // 2, w - 1} | {x for b in range(tc.FIN_TILE_W, w, tc.FIN_TILE_W) for x in (b - 1, b)})
    for n, (y, x) in enumerate([(y, x) for y in ys for x in xs]):
        m = np.zeros((h, w), bool)
        m[y, x] = True
        if n % 3 == 0 or (y in (0, h - 1) and x in (0, w - 1)):
            yield 'single (%d, %d)' % (y, x), m
    yield 'random', np.random.default_rng(h * w).random((h, w)) < 0.08


@pytest.mark.parametrize('shape', FIN_SHAPES)
def test_finish_against_scipy(ctx, shape):
    h, w = shape
    rng = np.random.default_rng(60 + w)
    raw = rng.integers(1, 9, (h, w)) / rng.integers(1, 5, (h, w))
    pitch, mpitch, opitch = (w + 3, w + 1, w + 2) if w % 2 else (w, w, w)
    n_zero = n_pos = 0
    for name, m0 in finish_masks(h, w):
        mean = ref.stencil_ref.masked_mean(np.where(m0, 0.0, raw), m0, 7, fill_mask=False)
        want = ref.finish(mean, m0)
        d_out, = planes(ctx, 1, h, opitch)
        d_mean = ctx.to_device(padded(mean, pitch, PLANE_FILL))
        d_m = ctx.to_device(padded(m0.astype(np.uint8), mpitch, 1))
        ctx._check(ctx._lib.ipa_tss_finish_dev(ctx.handle, d_mean.ptr, d_m.ptr, h, w, pitch, mpitch, d_out.ptr,
                                               opitch), 'tss_finish')
        got = unpad(d_out, w)
        assert same(got, want), (shape, name, np.argwhere(got != want)[:4].tolist())
        n_zero += int((want == 0).sum())
        n_pos += int((want > 0).sum())
        if name in ('random', 'clear'):
            assert same(_ops().tss_finish(mean, m0), want)
            d = _ops().tss_finish(ctx.to_device(mean), ctx.to_device(m0.astype(np.uint8)))
            assert same(d.get(), want)
    assert n_zero and (n_pos or shape == (1, 1))


def test_finish_refusals(ctx):
    h, w = 5, 9
    d_mean, d_m = ctx.to_device(np.ones((h, w))), ctx.to_device(np.zeros((h, w), np.uint8))
    d_out, = planes(ctx, 1, h, w)

    def call(mean=d_mean.ptr, m=d_m.ptr, out=d_out.ptr, hh=h, ww=w, pitch=w, mpitch=w, opitch=w):
        return ctx._lib.ipa_tss_finish_dev(ctx.handle, mean, m, hh, ww, pitch, mpitch, out, opitch)
    for kw in (dict(mean=None), dict(m=None), dict(out=None), dict(hh=0), dict(ww=0), dict(pitch=w - 1),
               dict(mpitch=w - 1), dict(opitch=w - 1), dict(out=d_mean.ptr)):
        assert call(**kw) == ERR_BAD_ARG, kw
    ctx.synchronize()
    assert np.all(d_out.get() == GUARD) and np.all(d_mean.get() == 1.0)
    assert call() == 0 and np.all(d_out.get() == 1.0)


# ------------------------------------------------------------------ the ops wrappers
def test_ops_event_length_host_and_device(ctx):
    from imgprocessor_amd import DeviceArray
    ops = _ops()
    T, shape = 9, tc.MULTI
    st, times, off, asc, err = tc.scene('continuous', T, shape, np.uint16, 0)
    want_evt, want_raw = tc.reference('continuous', T, shape, np.uint16, 0)
    got = ops.tss_event_length(st, times, off, asc, err)
    assert isinstance(got, np.ndarray) and same(got, want_raw)
    avlen, ev = ops.tss_event_length(list(st), list(times), off, asc, err, events=True)
    assert same(avlen, want_raw) and ev.dtype == np.uint8 and np.array_equal(ev, want_evt)
    d = [ctx.to_device(np.ascontiguousarray(a)) for a in (off, asc, err)]
    avlen, ev, zero = ops.tss_event_length(ctx.to_device(st), times, *d, events=True, zero_mask=True)
    assert all(isinstance(a, DeviceArray) for a in (avlen, ev, zero))
    assert same(avlen.get(), want_raw) and np.array_equal(ev.get(), want_evt)
    assert np.array_equal(zero.get(), (want_raw == 0).astype(np.uint8))
    avlen = ops.tss_event_length([ctx.to_device(f) for f in st], times, *d)
    assert same(avlen.get(), want_raw)
    with pytest.raises(ValueError):
        ops.tss_event_length(st, times, off[:-1], asc, err)


# ------------------------------------------------------------------ end to end
_restated = {}


def restated(name):
    if name not in _restated:
        times, frames = getattr(tc, name)()
        _restated[name] = (times, frames, ref.temporal_signal_stability(frames, times))
    return _restated[name]


@pytest.mark.parametrize('given', ('host stack', 'host list', 'device stack', 'device list'))
@pytest.mark.parametrize('name', ('demo', 'demo16'))
def test_temporal_signal_stability(ctx, g, name, given):
    from imgprocessor_amd import DeviceArray
    from imgprocessor_amd.uncertainty import temporalSignalStability
    times, frames, want = restated(name)
    dev = given.startswith('device')
    imgs = {'host stack': lambda: frames, 'host list': lambda: list(frames),
            'device stack': lambda: ctx.to_device(frames),
            'device list': lambda: [ctx.to_device(f) for f in frames]}[given]()
    out = temporalSignalStability(imgs, list(times) if 'list' in given else times)
    assert len(out) == 4 and all(isinstance(a, DeviceArray if dev else np.ndarray) for a in out)
    error, avlen, ascent, offset = [a.get() if dev else a for a in out]
    p = name + '_'
    for k, a in (('error', error), ('ascent', ascent), ('offset', offset)):
        assert same(a, want[k]) and same(a, g[p + k]), (name, given, k)
    for src, b in (('restatement', want['avlen']), ('fixture', g[p + 'avlen'])):
        assert np.array_equal(avlen == 0, b == 0), (name, given, src, 'zero pattern')
        nz = b != 0
        err = np.max(np.abs(avlen[nz] - b[nz]) / b[nz]) if nz.any() else 0.0
        print('%s, %s: event length against the %s: rel err %.1e' % (name, given, src, err))
        np.testing.assert_allclose(avlen, b, rtol=1e-13, atol=1e-15)
    assert (avlen > 0).any() and (avlen == 0).any()
    if given == 'device stack':   # the steps in between, against the fixture
        ops = _ops()
        d_off, d_asc, d_err = out[3], out[2], out[0]
        raw, ev = ops.tss_event_length(imgs, times, d_off, d_asc, d_err, events=True)
        assert str(g['linreg_source']) != 'restatement' or (
            np.array_equal(ev.get(), unpack(g[p + 'events'], frames.shape)) and same(raw.get(), g[p + 'raw']))
        assert np.array_equal(ev.get(), want['events']) and same(raw.get(), want['raw'])
