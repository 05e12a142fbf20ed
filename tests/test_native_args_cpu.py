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


SHIFT = (-16384, 16384, 'shift')
COEFF = (-50000, 50000, 'coefficient')


def _table(values, tiles, ranges=(SHIFT, SHIFT)):
    table, n = native._tuple_table(values, tiles, ranges, 'params', 'a tuple')
    return list(table), n


def test_tuple_table_one_for_all_or_one_per_leading_index():
    assert _table((3, -4), _t()) == ([3, -4], 1)
    assert _table([np.int64(3), np.int32(-4)], torch.zeros((8, 8))) == ([3, -4], 1)      # one tuple suits a single plane too
    assert _table([(1, 2), [3, 4], np.array([5, 6])], _t()) == ([1, 2, 3, 4, 5, 6], 3)
    assert _table([(1, 2), (3, 4)], _b()) == ([1, 2, 3, 4], 2)                           # per index of the FIRST dimension
    assert _table([(1, 2), (3, 4)], torch.zeros((2, 8, 8))) == ([1, 2, 3, 4], 2)         # two pairs, not one pair of pairs
    six = (1, 2, 3, 4, 5, 6)
    assert _table(six, _t(), (SHIFT, SHIFT) + (COEFF,) * 4) == (list(six), 1)
    assert _table([six] * 3, _t(), (SHIFT, SHIFT) + (COEFF,) * 4) == (list(six) * 3, 3)
    table, n = native._tuple_table((3, -4), _t(), (SHIFT, SHIFT), 'params', 'a tuple')
    assert np.ctypeslib.as_array(table).dtype == np.int32 and n == 1


@pytest.mark.parametrize('values,tiles', [
    (5, _t),                                        # no sequence at all
    ([(1, 2), (3, 4)], _t),                         # wrong count: two for three leading indices
    ([(1, 2)] * 4, _t),
    ([], _t),
    ((1, 2, 3), _t),                                # wrong width: three integers are three entries, none a pair
    ([(1, 2), (3, 4), (5, 6, 7)], _t),              # ... and an entry of another width
    ([(1, 2), (3, 4), 5], _t),
    ([(1, 2), (3, 4), 'ab'], _t),
    ((1.0, 2), _t),                                 # a non-integer
    ((True, 2), _t),
    ([(1, 2), (3, 4), (5, 6.5)], _t),
    ([(1, 2)], lambda: torch.zeros((8, 8))),        # a 2-d tensor has no leading index to give a sequence to
    ([(1, 2), (3, 4)], lambda: torch.zeros((8, 8))),
])
def test_tuple_table_refuses(values, tiles):
    with pytest.raises(ValueError):
        _table(values, tiles())


def test_tuple_table_holds_every_position_to_its_own_range():
    ranges = ((-1, 1, 'frame index'), (0, 255, 'constant'))
    for good in ((-1, 0), (1, 255)):
        assert _table(good, _t(), ranges) == (list(good), 1)
    for bad, noun in (((-2, 0), 'frame index'), ((2, 0), 'frame index'), ((0, -1), 'constant'), ((0, 256), 'constant')):
        with pytest.raises(ValueError, match=noun):
            _table(bad, _t(), ranges)
        with pytest.raises(ValueError, match=noun):
            _table([(0, 0), (0, 0), bad], _t(), ranges)


def test_batch_and_output_checks_sit_in_the_helpers():
    """Host tensors and no shared object: what can be refused without a device is refused by the helpers, by name."""
    for bad in (_t(), np.zeros((3, 8, 8), np.uint16), None):
        with pytest.raises(ValueError, match='left must be a .* device tensor'):
            native._plane_batch(bad, 'left')
    with pytest.raises(ValueError, match=r'\[n, H, W\] or \[b, n, H, W\] device tensor'):
        native._plane_batch(_t(), 'tiles', '[n, H, W] or [b, n, H, W]', (3, 4))
    t = _t()
    src = native._plane_layout(t, 'tiles')
    for bad in (torch.zeros((3, 8, 8), dtype=torch.float32),        # a float tensor
                torch.zeros((3, 8, 9), dtype=torch.uint16),         # another shape
                torch.zeros((3, 8, 8), dtype=torch.uint16).numpy()):
        with pytest.raises(ValueError, match='out must be'):
            native._out_of_place(bad, (3, 8, 8), t, src, 'filter', None)
    with pytest.raises(ValueError):                                   # a permuted view: its rows are not contiguous
        native._out_of_place(torch.zeros((3, 8, 8), dtype=torch.uint16).permute(0, 2, 1), (3, 8, 8), t, src, 'filter', None)
    whole = torch.zeros((4, 8, 8), dtype=torch.uint16)
    src = native._plane_layout(whole[:3], 'tiles')
    for noun in ('filter', 'binning', 'correction', 'shift', 'map'):
        with pytest.raises(ValueError, match=f'shares memory with tiles: the {noun} is out of place'):
            native._out_of_place(whole[1:], (3, 8, 8), whole[:3], src, noun, None)
    good = torch.zeros((3, 8, 12), dtype=torch.uint16)[:, :, :8]
    out, dst = native._out_of_place(good, (3, 8, 8), t, native._plane_layout(t, 'tiles'), 'filter', None)
    assert out is good and dst == (3, 8, 8, 96, 12)
    made, dst = native._out_of_place(None, (3, 4, 4), t, native._plane_layout(t, 'tiles'), 'binning', None)
    assert made.shape == (3, 4, 4) and made.dtype == t.dtype and dst == (3, 4, 4, 16, 4)
    empty = torch.zeros((0, 8, 8), dtype=torch.uint16)               # no plane: nothing to overlap with
    assert native._out_of_place(empty, (0, 8, 8), empty, native._plane_layout(empty, 'tiles'), 'filter', None)[0] is empty


@pytest.mark.parametrize('call', [
    lambda t: native.tophat_tiles(t, 3), lambda t: native.despeckle_tiles(t, 5), lambda t: native.tile_stats(t),
    lambda t: native.dpc_tiles(t, t), lambda t: native.bin_tiles(t, 2), lambda t: native.warp_tiles(t, 100),
    lambda t: native.shift_tiles(t, (1, 2)), lambda t: native.affine_tiles(t, (0,) * 6), lambda t: native.dark_tiles(t, (-1, 1)),
])
def test_every_per_tile_wrapper_refuses_a_host_tensor_by_the_batch_checker(monkeypatch, call):
    def no_library():
        raise AssertionError('lib() was reached before the batch was checked')
    monkeypatch.setattr(native, 'lib', no_library)
    with pytest.raises(ValueError, match='device tensor'):
        call(_t())
