"""CPU: the table of tests/chain_cases.py itself - the bits it restates are those of imgprocessor_amd/_lib.py and
include/imgproc_hip.h, every bit is expected somewhere, every boundary has a case on either side, every routing
knob flips an expectation, the geometry has the strips the docstring promises (the kernels' `fast` predicates
restated), every case's inputs and reference build and repeat, no filter is symmetric, and the reference alone
tells every filter from the same filter with its taps turned round - in an interior strip and in a rim strip."""
import os
import re

import numpy as np
import pytest

from . import chain_cases as cc
from .conftest import ROOT

EDGES = ['dense_k7_streams', 'dense_k11_last', 'dense_square_odd', 'stream_k', 'big_fused', 'dense_cubic_k7',
         'dense_taps', 'dense_k9_by_value', 'lens_cache_dense', 'shared7_frames', 'pipe7', 'u16_k7_last', 'u16_coords',
         'u8_coords', 'sep_taps9', 'sep_equal_taps', 'sep_taps', 'sep_u16_coords', 'sep_u8_coords', 'sep_u16',
         'rank1_exact', 'rank1_taps9', 'rank1_sep', 'rank1_taps', 'rank1_u16_lens', 'plan_frames4', 'plan_split7',
         'streamed_frames4', 'frames_wg', 'pipe', 'frames_inner', 'plan_apart', 'stored4', 'stored_coords']
KNOBS = ('big_fused', 'stream_k', 'pipe7', 'sep_u16', 'rank1_sep', 'stored_coords', 'lens_cache', 'frames_wg', 'pipe',
         'frames_inner')
GROUPS = 'DCSRBTG'


def test_bits_match_the_binding_and_the_header():
    from imgprocessor_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'imgproc_hip.h')).read()
    in_header = {m.group(1): 1 << int(m.group(2)) for m in re.finditer(r'IPA_CHAIN_PATH_(\w+) = 1 << (\d+)', hdr)}
    assert sorted(in_header) == sorted(cc.BIT_NAMES)
    for k, name in enumerate(cc.BIT_NAMES):
        assert getattr(cc, name) == 1 << k == in_header[name] == getattr(_lib, 'CHAIN_PATH_' + name), name
    assert cc.path_names(cc.RESIDENT | cc.PER_FRAME) == 'RESIDENT|PER_FRAME' and cc.path_names(0) == '0'


def test_every_bit_is_expected_by_some_case():
    for k, name in enumerate(cc.BIT_NAMES):
        if name == 'ROTATED':
            # rotated_warp_in_two_launches answers yes from 8 frames and 64e6 result pixels on: no case of a few MB can
            # turn it; test_gpu_tile_warp.py::test_rotated_fused_chains_in_two_launches_have_the_same_bits asserts it
            assert not any(c.expect & cc.ROTATED for c in cc.CASES)
            continue
        assert any(c.expect >> k & 1 for c in cc.CASES), name
    kernels = cc.RESIDENT | cc.STREAMED | cc.SEP
    for c in cc.CASES:
        assert 0 < c.expect < 1 << len(cc.BIT_NAMES), c.id
        own = c.expect & kernels
        # one route per call: one of the chain's kernels with the shape of its launches, or the two launches with none
        assert bin(own).count('1') + bool(c.expect & cc.TWO_LAUNCHES) == 1, c.id
        assert bool(own) == bool(c.expect & (cc.FRAMES_WG | cc.PER_FRAME)), c.id
        assert not (c.expect & cc.FRAMES_WG and c.expect & cc.PER_FRAME), c.id
        assert not c.expect & cc.RANK1 or c.expect & cc.SEP, c.id
        assert not c.expect & (cc.SPLIT | cc.STORED) or c.expect & cc.FRAMES_WG, c.id
    # the routes alone, too: not only behind a second bit
    for alone in (cc.RESIDENT | cc.PER_FRAME, cc.RESIDENT | cc.FRAMES_WG, cc.STREAMED | cc.PER_FRAME,
                  cc.STREAMED | cc.FRAMES_WG, cc.SEP | cc.PER_FRAME, cc.SEP | cc.FRAMES_WG, cc.TWO_LAUNCHES):
        assert any(c.expect == alone for c in cc.CASES), cc.path_names(alone)


def test_every_boundary_has_a_case_on_either_side():
    sides = {}
    for c in cc.CASES:
        for name, side in c.edge:
            assert side in ('below', 'at', 'above'), c.id
            sides.setdefault(name, {}).setdefault(side, set()).add(c.expect)
    assert sorted(sides) == sorted(EDGES)
    for name, s in sides.items():
        assert len(s) >= 2, (name, sorted(s))
        # ... and the sides do not expect the same thing
        assert len(set.union(*s.values())) >= 2, name
    assert sorted(set(c.group for c in cc.CASES)) == sorted(GROUPS)


def _but_for(c, knob):
    return (c.sdt, c.interp, c.coords, c.n, c.shape, c.filt, c.overlap, tuple(sorted((k, v) for k, v in c.knobs.items()
                                                                                      if k != knob)))


@pytest.mark.parametrize('knob', KNOBS)
def test_every_routing_knob_flips_an_expectation(knob):
    """two cases that differ in that knob alone and expect different records"""
    seen = {}
    for c in cc.CASES:
        seen.setdefault(_but_for(c, knob), {})[c.knobs.get(knob)] = c.expect
    assert any(len(set(v.values())) > 1 for v in seen.values() if len(v) > 1), knob


def test_the_table_covers_what_it_must():
    by = lambda **kw: [c for c in cc.CASES if all(getattr(c, k) == v for k, v in kw.items())]
    for filt in (('dense', 5, 5), ('sep', 5, 5), ('dense', 9, 9)):
        assert {c.n for c in by(group='B', filt=filt, knobs={}, overlap=False)} >= {1, 3, 4, 5, 6, 7, 8, 9}, filt
    assert len(by(overlap=True)) == 2 and all(c.n == 7 and not c.expect & cc.SPLIT and c.expect & cc.PER_FRAME
                                              for c in by(overlap=True))
    # one case per kernel family on each of the two other geometries
    for shape in ('odd', 'ragged'):
        got = {c.expect & (cc.RESIDENT | cc.STREAMED | cc.SEP | cc.TWO_LAUNCHES | cc.RANK1) for c in by(shape=shape)}
        assert got >= {cc.RESIDENT, cc.STREAMED, cc.SEP, cc.TWO_LAUNCHES, cc.RANK1 | cc.SEP}, shape
    # the boundary that guards fused_sep_interp: uint16 frames under the lens model by value never reach wave_sep_kernel
    guard = by(sdt=cc.U16, coords='lens', knobs=dict(lens_cache=0))
    assert {c.filt[0] for c in guard} >= {'sep', 'rank1', 'dense'}
    assert all(not c.expect & cc.SEP for c in guard)
    # nothing large
    assert all(c.n <= 9 for c in cc.CASES)
    sh, sw = cc.SRC_HW
    assert 9 * sh * sw * 4 + 9 * 52 * 760 * 4 < 4e6


def test_geometry_has_every_kind_of_strip(oracle):
    """wave_geom / sep_geom and the `fast` predicates of wave_stencil_body and wave_sep_kernel, restated in
    chain_cases.fast_strips, on the three result shapes"""
    geoms = {('dense', 3): (240, 2), ('dense', 5): (240, 2), ('dense', 7): (248, 1), ('dense', 9): (240, 2),
             ('dense', 11): (240, 2), ('sep', 3): (240, 2), ('sep', 5): (240, 2), ('sep', 7): (240, 2), ('sep', 9): (240, 2)}
    for (kind, K), (ow, hl) in geoms.items():
        assert cc.strip_geometry((kind, K, K))[2:] == (ow, hl), (kind, K)
        for depth in (1, 2):
            fx, fy, xs = cc.fast_strips(K, ow, hl, *cc.SHAPES['main'], depth)
            assert fx == [False, True, True, False], (kind, K, xs)
            assert fy[0] is False and fy[1] is True and fy[3] is False and len(fy) == 4, (kind, K, fy)
            assert fy[2] == (K <= 9), (kind, K)
            ox, oy, _ = cc.fast_strips(K, ow, hl, *cc.SHAPES['odd'], depth)
            assert (ox, oy) == (fx, fy), (kind, K)
            rx, ry, rxs = cc.fast_strips(K, ow, hl, *cc.SHAPES['ragged'], depth)
            assert not any(rx) and len(rx) >= 2 and any(ry), (kind, K, rxs)
    assert cc.fast_strips(5, 240, 2, 52, 760, 1)[2] == [-8, 232, 472, 712]
    assert cc.fast_strips(7, 248, 1, 52, 760, 1)[2] == [-4, 244, 492, 740]
    dh, dw = cc.SHAPES['main']
    assert dw % 4 == 0 and cc.SHAPES['odd'][1] % 4 and cc.SHAPES['ragged'][1] % 4
    # footprints outside the source in interior and in rim strips, for every coordinate source
    sh, sw = cc.SRC_HW
    for shape in ('main', 'odd'):
        dh, dw = cc.SHAPES[shape]
        v, u = np.mgrid[0:dh, 0:dw].astype(np.float64)
        M = cc.homography(shape)
        w = M[2, 0] * u + M[2, 1] * v + M[2, 2]
        lx, ly = oracle.build_undistort_map(*cc.lens(shape), dh, dw)
        for name, (sx, sy) in (('maps', cc.maps(shape)), ('lens', (lx, ly)),
                               ('hom', ((M[0, 0] * u + M[0, 1] * v + M[0, 2]) / w, (M[1, 0] * u + M[1, 1] * v + M[1, 2]) / w))):
            sx, sy = np.asarray(sx, np.float64), np.asarray(sy, np.float64)
            assert sy.min() > 2 and sy.max() < sh - 3, (name, shape)            # rows: always inside
            assert np.abs(np.diff(sy, axis=1)).max() < 0.01, name                # a few pixels of drift over the frame
            out = (sx < -1) | (sx > sw)
            for filt in (('dense', 5, 5), ('dense', 7, 7), ('dense', 11, 11), ('sep', 9, 9)):
                m = cc.interior_mask(filt, shape)
                assert m.any() and (~m).any()
                assert (out & m).sum() >= 16 and (~out & m).sum() > m.sum() // 2, (name, shape, filt)
                assert (out & ~m & (u < 100)).any() and (out & ~m & (u > 700)).any(), (name, shape, filt)
    assert not cc.interior_mask(('dense', 5, 5), 'ragged').any()


def test_no_filter_is_symmetric():
    for c in cc.CASES:
        f = cc.kernel(c)
        again = cc.kernel(c)
        if isinstance(f, tuple):
            ky, kx = f
            assert np.array_equal(ky, again[0]) and np.array_equal(kx, again[1])
            assert (len(ky), len(kx)) == c.filt[1:]
            assert not np.allclose(ky, ky[::-1], rtol=0.05) and not np.allclose(kx, kx[::-1], rtol=0.05), c.id
            assert len(ky) != len(kx) or not np.allclose(ky, kx, rtol=0.05), c.id
            assert abs(ky.sum() - 1) < 1e-12 and abs(kx.sum() - 1) < 1e-12 and ky.min() > 0 and kx.min() > 0
        else:
            assert np.array_equal(f, again)
            assert f.shape == (c.filt[1], c.filt[-1])
            for name, t in cc.turned(f).items():
                assert t.shape != f.shape or not np.allclose(t, f, rtol=0.05), (c.id, name)
            rank = np.linalg.matrix_rank(f, tol=1e-6)
            assert rank == (1 if c.filt[0] in ('rank1', 'near1') else min(f.shape)), c.id
            if c.filt[0] == 'near1':      # not an outer product by the library's 1e-12 of the largest entry
                ky, kx = f[:, 1] / f[:, 1].sum(), f[1] / f[1].sum()
                assert abs(f[0, 0] - np.outer(ky, kx)[0, 0] * f.sum()) > 1e-10 * f.max(), c.id


@pytest.mark.parametrize('group', list(GROUPS))
def test_inputs_and_references_build_and_repeat(oracle, group):
    """... and the reference with the taps turned round is told apart from the expected one: by at least 100
    tolerances somewhere in an interior strip and somewhere in a rim strip"""
    for c in cc.CASES:
        if c.group != group:
            continue
        inp, again = cc.inputs(c, oracle), cc.inputs(c, oracle)
        assert sorted(inp) == sorted(again)
        for k in inp:
            if k != 'filt':
                assert np.array_equal(inp[k], again[k]), (c.id, k)
        assert inp['src'].shape == (c.n,) + cc.SRC_HW and inp['src'].dtype == np.dtype(c.sdt)
        assert float(inp['src'].max()) <= cc.VALUE_RANGE[c.sdt] and float(inp['src'].max()) > 0.9 * cc.VALUE_RANGE[c.sdt]
        f = c.n - 1
        want, twice = cc.expected(c, inp, oracle, f), cc.expected(c, inp, oracle, f)
        assert want.shape == cc.SHAPES[c.shape] and want.dtype == np.float64 and np.isfinite(want).all(), c.id
        assert np.array_equal(want, twice), c.id
        assert np.unique(want).size > want.size // 2, c.id
        rtol, atol = cc.tolerance(c)
        tol = atol + rtol * np.abs(want)
        assert (cc.rounding_bound(c, inp, oracle, f) < tol).all(), c.id      # the tolerance is no tighter than rounding
        inside = cc.interior_mask(c.filt, c.shape)
        assert inside.any() == (c.shape != 'ragged'), c.id
        mid = cc.remapped(c, inp, oracle, f)
        for name, t in cc.turned(inp['filt']).items():
            far = np.abs(cc.filtered(mid, t) - want) >= 100 * tol
            assert (far & ~inside).any(), '%s: %s passes on the rim strips' % (c.id, name)
            assert (far & inside).any() or c.shape == 'ragged', '%s: %s passes on the interior strips' % (c.id, name)
