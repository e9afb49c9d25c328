"""CPU: the table of tests/remap_cases.py itself - every path bit is expected somewhere, every boundary
the table names has a case on each side, every case's inputs and oracle call build and repeat, and the
bits the table restates are those of imgprocessor_amd/_lib.py and include/imgproc_hip.h."""
import os
import re

import numpy as np
import pytest

from . import remap_cases as rc
from .conftest import ROOT

# the boundaries the issue names; 'sides': what must be present on either side of each
EDGES = ['tile256x4', 'u8cubic64rows', 'u8lz128x256', 'ring_rows32', 'ring_cols128', 'ring_waves_linear',
         'ring_waves_cubic', 'ring_waves_lanczos4', 'ring_from_maps_linear', 'ring_from_maps_cubic',
         'ring_from_maps_lanczos4', 'ring_from_lens_linear', 'ring_from_lens_cubic', 'ring_from_hom_cubic',
         'ring_from_lens_lanczos4', 'ring_from_hom_lanczos4', 'stored4_lens_cubic', 'stored4_lens_cubic_cv',
         'stored4_lens_lanczos4', 'stored4_hom_cubic', 'stored4_hom_cubic_cv', 'stored4_hom_lanczos4',
         'tile64x32', 'tile_frames8', 'tile_box_fits', 'tile_u16_2e6', 'tile_cubic_16e6', 'tilemap64x32',
         'tilemap_frames8', 'tilemap_lz_8e6', 'lens_map4_u8_f32', 'lens_map4_u8_u8']


def test_bits_match_the_binding_and_the_header():
    from imgprocessor_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'imgproc_hip.h')).read()
    in_header = {m.group(1): 1 << int(m.group(2))
                 for m in re.finditer(r'IPA_REMAP_PATH_(\w+) = 1 << (\d+)', hdr)}
    assert sorted(in_header) == sorted(rc.BIT_NAMES)
    for k, name in enumerate(rc.BIT_NAMES):
        assert getattr(rc, name) == 1 << k == in_header[name] == getattr(_lib, 'REMAP_PATH_' + name), name


def test_every_bit_is_expected_by_some_case():
    for k, name in enumerate(rc.BIT_NAMES):
        if name in ('STRIP',):
            assert any(c.expect == rc.STRIP for c in rc.CASES)      # ... and alone, not only behind LENS_MAP
        assert any(c.expect >> k & 1 for c in rc.CASES), name
    # plain gather runs need no second run: at least one case per alternative forces one
    assert all(c.expect < 1 << len(rc.BIT_NAMES) and c.expect > 0 for c in rc.CASES)


def test_every_boundary_has_a_case_on_each_side():
    sides = {}
    for c in rc.CASES:
        for name, side in c.edge:
            assert side in ('below', 'at', 'above'), c.id
            sides.setdefault(name, set()).add(side)
    assert sorted(sides) == sorted(EDGES)
    for name, s in sides.items():
        assert 'below' in s and ('at' in s or 'above' in s), (name, s)
    for name in ('tile256x4', 'u8cubic64rows', 'u8lz128x256', 'ring_rows32', 'ring_cols128', 'tile64x32',
                 'tilemap64x32', 'ring_waves_linear', 'ring_waves_cubic', 'ring_waves_lanczos4', 'tile_frames8',
                 'tilemap_frames8'):
        assert sides[name] == {'below', 'at', 'above'}, name      # sizes one short of, at and one past


def test_groups_cover_what_the_issue_lists():
    by = {}
    for c in rc.CASES:
        by.setdefault(c.group, []).append(c)
    assert sorted(by) == list('ABCDEFG')
    a = by['A']
    for pair in rc.DTYPE_PAIRS:        # the instantiation matrix: pair x source x bilinear / Lanczos4
        for kind in ('maps', 'lens', 'hom'):
            for interp in ('linear', 'lanczos4'):
                got = {c.border for c in a if (c.sdt, c.ddt) == pair and c.coords[0] == kind and c.interp == interp
                       and c.dst_hw == (41, 77) and c.src_hw == (37, 70)}
                assert got >= ({'constant', 'reflect'} if pair != (rc.F32, rc.F32) else set(rc.BORDERS)), (pair, kind)
    assert {c.sdt for c in a if c.coords[0] == 'grid'} >= {rc.F32, rc.U8, rc.F64}
    assert {c.interp for c in a if (c.sdt, c.ddt) == (rc.U16, rc.U16)} >= {'linear_cv_q5', 'cubic_cv_q5'}
    assert all(c.knobs == rc.GATHER_ONLY for c in a)
    assert all(c.expect == rc.U8_LZ_LDS or c.coords[0] == 'grid' for c in by['B']) and any(c.pad for c in by['B'])
    assert {c.coords[0] for c in by['B']} == {'maps', 'lens', 'hom', 'grid'}
    assert all(c.knobs == {} for c in by['B'] + by['F'])
    assert all(c.expect == rc.GATHER and c.coords[0] == 'grid' for c in by['G'])
    # consecutive ring cases never share a result shape: no case can inherit the hint of the one before
    ring = [c for c in by['C'] if c.knobs == rc.RING_ALWAYS]
    assert all(x.dst_hw != y.dst_hw for x, y in zip(ring, ring[1:]))
    # the arrays stay small: the 64 MB of the bicubic rule are the largest
    for c in rc.CASES:
        assert c.n * c.src_hw[0] * c.src_hw[1] * np.dtype(c.sdt).itemsize <= 64e6, c.id
        assert c.n * c.dst_hw[0] * c.dst_hw[1] * np.dtype(c.ddt).itemsize <= 64e6, c.id


@pytest.mark.parametrize('group', list('ABCDEFG'))
def test_inputs_and_oracle_calls_build_and_repeat(oracle, group):
    for c in rc.CASES:
        if c.group != group:
            continue
        inp, again = rc.inputs(c, oracle), rc.inputs(c, oracle)
        assert sorted(inp) == sorted(again)
        for k in inp:
            assert np.array_equal(inp[k], again[k], equal_nan=True), (c.id, k)
        assert inp['src'].shape == (c.n,) + c.src_hw and inp['src'].dtype == np.dtype(c.sdt)
        f = c.n - 1 if c.oracle_frames is None else c.oracle_frames[-1]
        want, twice = rc.oracle_frame(c, inp, oracle, f), rc.oracle_frame(c, inp, oracle, f)
        assert want.shape == c.dst_hw and want.dtype == np.dtype(c.ddt), c.id
        assert np.array_equal(want, twice, equal_nan=want.dtype.kind == 'f'), c.id
        if want.dtype.kind == 'f':
            assert np.isfinite(want).mean() > 0.5, c.id
        # the picture is in sight: a case whose result is one flat value checks nothing
        assert np.unique(want[np.isfinite(want)] if want.dtype.kind == 'f' else want).size > 16, c.id


def test_ring_cases_put_pixels_through_the_ring_kernel(oracle):
    """RING in the mask only says that ring_remap_kernel was launched; it writes the clean strip pairs alone
    (remap_cases.ring_clean_pairs restates the planning rule).  Every ring case whose width has a pair of
    whole strips has a clean pair - so the bit-for-bit comparison with the gather kernel is ring against
    gather -, the widths that pair a whole strip with a partial one (or have none) have no clean pair, and
    wherever a strip row has more than one pair the rest launch has work too; with 65 rows and in the cases of the
    default rule a WHOLE pair is dirty because its footprints leave the source."""
    ring = [c for c in rc.CASES if c.expect & rc.RING]
    assert len(ring) == 80 and all(c.group == 'C' for c in ring)
    seen = {}
    for c in ring:
        pairs = rc.ring_clean_pairs(c, rc.inputs(c, oracle), oracle)
        whole = c.dst_hw[1] in rc.RING_WHOLE_PAIR_COLS or c.dst_hw[1] % 256 == 0
        assert pairs.any() == whole, (c.id, pairs)
        if pairs.shape[1] > 1:                       # (33 x 128: both strip rows clean, the second of one row)
            assert not pairs.all(), c.id
        if whole and (c.dst_hw[0] == 65 or c.id.endswith('-rule')):
            assert pairs[0, 0] and not pairs[1, 0], (c.id, pairs)       # a rim of footprints outside the source
        if pairs.any():
            for name, side in c.edge:
                seen.setdefault((name, c.coords[0], c.interp), set()).add(side)
    # ... on every side of the row count and the frame count, for every source and tap count
    for kind in ('maps', 'lens', 'hom'):
        for interp in ('linear', 'cubic', 'lanczos4'):
            assert seen[('ring_rows32', kind, interp)] == {'below', 'at', 'above'}, (kind, interp)
            assert seen[('ring_waves_' + interp, kind, interp)] == {'below', 'at', 'above'}, (kind, interp)
            assert seen[('ring_cols128', kind, interp)] == {'at', 'above'}, (kind, interp)   # 128 and 257


def test_the_clean_rule_sees_what_makes_a_strip_dirty(oracle):
    """the restatement itself: a case with a clean pair loses it when the source is one row or column too
    small for the pair's footprints, and when a coordinate of the pair is not finite"""
    c = rc.BY_ID['C-f32_f32-lanczos4-reflect-maps-inset-n2-32x257']
    inp = rc.inputs(c, oracle)
    assert rc.ring_clean_pairs(c, inp, oracle).tolist() == [[True, False]]
    need_h = int(np.floor(np.rint(inp['my'][:, :256].max() * 32.0) / 32)) + 5   # Lanczos4 (at 1/32 px): rows floor(y) - 3 ... + 4
    need_w = int(np.floor(np.rint(inp['mx'][:, :256].max() * 32.0) / 32)) + 5
    assert rc.ring_clean_pairs(c._replace(src_hw=(need_h, need_w)), inp, oracle)[0, 0]
    assert not rc.ring_clean_pairs(c._replace(src_hw=(need_h - 1, need_w)), inp, oracle).any()
    assert not rc.ring_clean_pairs(c._replace(src_hw=(need_h, need_w - 1)), inp, oracle).any()
    bad = dict(inp, mx=inp['mx'].copy())
    bad['mx'][7, 200] = np.nan
    assert not rc.ring_clean_pairs(c, bad, oracle).any()
