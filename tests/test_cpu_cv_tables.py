"""CPU-only: the cv2 interpolation tables the library uploads (csrc/cv_tables.hpp, read back through
ipa_cv_table: no context, no device) against the oracle's own tables - bit for bit, no tolerance."""
import ctypes as C

import numpy as np


def _table(which, dtype):
    from imgprocessor_amd import _lib
    lib = _lib.lib()
    n = lib.ipa_cv_table(which, None, 0)
    assert n > 0 and n % np.dtype(dtype).itemsize == 0
    out = np.zeros(n // np.dtype(dtype).itemsize, dtype)
    assert lib.ipa_cv_table(which, out.ctypes.data_as(C.c_void_p), n) == n
    return out


def test_rows_table_is_the_oracles(oracle):
    from imgprocessor_amd import _lib
    rows = _table(_lib.CV_TABLE_ROWS, np.float32)
    assert rows.size == 256 + 128
    want = []
    for which, ks in ((1, 8), (0, 4)):          # Lanczos4 first, then bicubic
        t = np.zeros((32, ks), np.float32)
        oracle.lib().orc_fixed_tab1d(which, t.ctypes.data_as(C.c_void_p))
        want.append(t.ravel())
    want = np.concatenate(want)
    bad = np.flatnonzero(rows.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, 'rows table differs from the oracle at %s' % bad.tolist()


def _unpack(table, ks):
    """the documented layout (include/imgproc_hip.h) -> (32, 32, ks, ks) int16 weights"""
    d = table.view(np.uint32).reshape(32, 32, ks, ks // 2)
    lo, hi = (d & 0xffff).astype(np.uint16).view(np.int16), (d >> 16).astype(np.uint16).view(np.int16)
    w = np.zeros((32, 32, ks, ks), np.int16)
    for q in range(ks // 2):
        if ks == 4:     # {w0 | w2 << 16, w1 | w3 << 16}
            w[..., q], w[..., q + 2] = lo[..., q], hi[..., q]
        else:           # {w0 | w1 << 16, w2 | w3 << 16, w4 | w5 << 16, w6 | w7 << 16}
            w[..., 2 * q], w[..., 2 * q + 1] = lo[..., q], hi[..., q]
    return w.astype(np.int32)


def test_u8_fixed_point_tables_are_the_oracles(oracle):
    from imgprocessor_amd import _lib
    for which, ks in ((_lib.CV_TABLE_U8_CUBIC, 4), (_lib.CV_TABLE_U8_LANCZOS4, 8)):
        tab = _table(which, np.int32)
        assert tab.size == 1024 * ks * ks // 2
        got = _unpack(tab, ks)
        it = np.zeros(ks * ks, np.int32)
        bad = []
        for fy in range(32):
            for fx in range(32):
                oracle.lib().orc_fixed_weights_2d(ks, fy, fx, it.ctypes.data_as(C.c_void_p))
                assert int(got[fy, fx].sum()) == 32768, (ks, fy, fx)
                if not np.array_equal(got[fy, fx], it.reshape(ks, ks)):
                    bad.append((fy, fx))
        assert not bad, 'ks %d: fraction pairs that differ from the oracle: %s' % (ks, bad)


def test_size_query_short_buffer_unknown_table():
    from imgprocessor_amd import _lib
    lib = _lib.lib()
    sizes = {_lib.CV_TABLE_ROWS: 384 * 4, _lib.CV_TABLE_U8_CUBIC: 1024 * 8 * 4,
             _lib.CV_TABLE_U8_LANCZOS4: 1024 * 32 * 4}
    for which, n in sizes.items():
        assert lib.ipa_cv_table(which, None, 0) == n
        assert lib.ipa_cv_table(which, None, n) == n
        buf = np.full(n, 0xA5, np.uint8)
        assert lib.ipa_cv_table(which, buf.ctypes.data_as(C.c_void_p), n - 1) == n
        assert (buf == 0xA5).all(), 'a buffer one byte short must stay untouched'
        assert lib.ipa_cv_table(which, buf.ctypes.data_as(C.c_void_p), n) == n
        assert (buf != 0xA5).any()
    for which in (-1, 3, 99):
        assert lib.ipa_cv_table(which, None, 0) == -1
