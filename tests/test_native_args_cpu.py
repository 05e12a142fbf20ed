"""The argument checkers of native.py, one per kind of argument: they read shapes, strides and addresses only, so host
tensors serve and neither a device nor the shared object is needed."""
import types

import numpy as np
import pytest
import torch

from image_stitcher_amd import native


def _t():
    return torch.zeros((3, 8, 8), dtype=torch.uint16)


def _b():
    return torch.zeros((2, 4, 8, 8), dtype=torch.uint8)


@pytest.mark.parametrize('make,want', [
    (lambda: _t(), (3, 8, 8, 64, 8)),
    (lambda: _t()[::2], (2, 8, 8, 128, 8)),
    (lambda: torch.zeros((3, 8, 12))[:, :, :8], (3, 8, 8, 96, 12)),
    (lambda: _b(), (8, 8, 8, 64, 8)),
    (lambda: _b()[:, ::2], (4, 8, 8, 128, 8)),
    (lambda: torch.zeros((1, 1, 5))[0], (1, 1, 5, 5, 5)),
    (lambda: torch.zeros((8, 8)), (1, 8, 8, 64, 8)),
])
def test_plane_layout(make, want):
    assert native._plane_layout(make(), 'x') == want


@pytest.mark.parametrize('make', [
    lambda: _t().permute(0, 2, 1),
    lambda: _t()[:1].expand(3, 8, 8),
    lambda: _b()[:, :3],
    lambda: _t()[:, :, :0],
    lambda: torch.zeros((3, 8, 16))[:, :, ::2],
])
def test_plane_layout_refuses(make):
    with pytest.raises(ValueError):
        native._plane_layout(make(), 'x')


def test_byte_extents():
    t = _t()
    extent = lambda v: native._byte_extent(v, native._plane_layout(v, 'x'))
    assert extent(t) == (t.data_ptr(), t.data_ptr() + 3 * 64 * 2)
    assert extent(t[::2]) == (t.data_ptr(), t.data_ptr() + (128 + 64) * 2)
    assert native._overlap(extent(t[:2]), extent(t[1:]))
    assert not native._overlap(extent(t[:1]), extent(t[2:]))
    assert native._overlap(extent(t[::2]), extent(t[1::2]))      # interleaved views share no element, their ranges do


def test_projected_planes():
    plan = lambda n: types.SimpleNamespace(n_tiles=n)
    assert native._projected_planes(plan(4), torch.zeros((3, 4, 8, 8)), None, None) == 3
    assert native._projected_planes(plan(4), torch.zeros((4, 8, 8)), None, None) == 1
    assert native._projected_planes(plan(4), None, torch.zeros(12, dtype=torch.int64), None) == 3
    assert native._projected_planes(plan(0), None, torch.zeros(0, dtype=torch.int64), [None, None]) == 2
    with pytest.raises(ValueError):
        native._projected_planes(plan(4), None, None, None)


def test_z_level_words():
    words = native._z_level_words([0, 2 ** 32 - 1], False)
    assert words.dtype == np.int32 and words.tolist() == [0, -1]
    for bad in (-1, 2 ** 32):
        with pytest.raises(ValueError, match='z levels'):
            native._z_level_words([0, bad], False)
    assert native._z_level_words([5, 5], False).tolist() == [5, 5]
    with pytest.raises(ValueError, match='distinct'):
        native._z_level_words([5, 5], True)


def test_int_in():
    lo, hi = 1, 127
    for bad in (True, 3.0, lo - 1, hi + 1):
        with pytest.raises(ValueError, match='radius'):
            native._int_in(bad, lo, hi, 'radius')
    assert native._int_in(np.int64(lo), lo, hi, 'radius') == lo
    assert native._int_in(hi, lo, hi, 'radius') == hi


PAIR_N_TILES, PAIR_H, PAIR_W, PAIR_N0, PAIR_N1 = 4, 160, 96, 128, 44
PAIR_ORIGINS = {'ref_y0': (PAIR_N0, PAIR_H), 'ref_x0': (PAIR_N1, PAIR_W), 'mov_y0': (PAIR_N0, PAIR_H), 'mov_x0': (PAIR_N1, PAIR_W)}


def _pairs(**fields):
    """Three good pairs, the middle one with `fields` set."""
    pairs = np.zeros(3, dtype=native.PAIR_DTYPE)
    pairs['mov_tile'] = 1
    for name, value in fields.items():
        pairs[name][1] = value
    return pairs


def _check_pairs(pairs):
    return native._check_pairs(pairs, PAIR_N_TILES, PAIR_H, PAIR_W, PAIR_N0, PAIR_N1)


@pytest.mark.parametrize('field', sorted(PAIR_ORIGINS))
def test_check_pairs_refuses_an_origin_that_leaves_its_tile(field):
    """... in int64: an int32 origin near 2^31 plus the crop side wraps to a negative sum, which is inside every tile."""
    side, limit = PAIR_ORIGINS[field]
    assert (np.array([2 ** 31 - side], dtype=np.int32) + np.int32(side))[0] < 0      # what the check must not compute
    for bad in (2 ** 31 - 1, 2 ** 31 - side, 2 ** 31 - 16, limit - side + 1, limit, -1, -2 ** 31):
        with pytest.raises(ValueError, match='crop reaches outside its tile'):
            _check_pairs(_pairs(**{field: bad}))
    for good in (0, 1, limit - side):
        got = _check_pairs(_pairs(**{field: good}))
        assert got.dtype == native.PAIR_DTYPE and got[field].tolist() == [0, good, 0]


def test_check_pairs_accepts_every_origin_at_its_limit_and_an_empty_table():
    edge = dict(ref_y0=PAIR_H - PAIR_N0, mov_y0=PAIR_H - PAIR_N0, ref_x0=PAIR_W - PAIR_N1, mov_x0=PAIR_W - PAIR_N1)
    pairs = _pairs(ref_tile=PAIR_N_TILES - 1, **edge)
    got = _check_pairs(pairs)
    assert got.tobytes() == pairs.tobytes() and got.flags.c_contiguous
    assert len(_check_pairs(np.zeros(0, dtype=native.PAIR_DTYPE))) == 0
    assert _check_pairs(pairs[::2]).flags.c_contiguous


@pytest.mark.parametrize('field', ['ref_tile', 'mov_tile'])
def test_check_pairs_refuses_a_tile_outside_the_table(field):
    for bad in (-1, PAIR_N_TILES, 2 ** 31 - 1, -2 ** 31):
        with pytest.raises(ValueError, match='pair refers to a tile outside the table'):
            _check_pairs(_pairs(**{field: bad}))
    assert _check_pairs(_pairs(**{field: PAIR_N_TILES - 1}))[field][1] == PAIR_N_TILES - 1


def test_register_pairs_checks_its_table_before_it_needs_the_library(monkeypatch):
    """Host tensors and no shared object: the refusal comes from the checker, ahead of lib()."""
    def no_library():
        raise AssertionError('lib() was reached before the pair table was checked')
    monkeypatch.setattr(native, 'lib', no_library)
    tiles = torch.zeros((PAIR_N_TILES, PAIR_H, PAIR_W), dtype=torch.uint16)
    minmax = torch.zeros((PAIR_N_TILES, 2), dtype=torch.int32)
    with pytest.raises(ValueError, match='crop reaches outside its tile'):
        native.register_pairs_async(tiles, minmax, _pairs(ref_y0=2 ** 31 - 16), PAIR_N0, PAIR_N1)
    with pytest.raises(ValueError, match='pair refers to a tile outside the table'):
        native.register_pairs(tiles, minmax, _pairs(mov_tile=PAIR_N_TILES), PAIR_N0, PAIR_N1)
    assert len(native.register_pairs(tiles, minmax, np.zeros(0, dtype=native.PAIR_DTYPE), PAIR_N0, PAIR_N1)) == 0


def test_device_checks_sit_in_the_helpers():
    for integer_only in (False, True):
        with pytest.raises(ValueError):
            native._plane_stack(_t(), 'planes', integer_only)
    with pytest.raises(ValueError):
        native._check_plane('out', torch.zeros((8, 8)), (8, 8))
