"""tests/tile_layouts.py itself: the padded buffers hold the tiles they were made of, everything around the tiles holds both
fill values, and the layouts tests/test_register_inputs_gpu.py runs have rows at every alignment phase of a 16-byte line --
a layout that quietly degenerated to aligned rows fails here, without a device."""
import numpy as np
import pytest

import tile_layouts as T


def _stack(dtype, shape, seed=0):
    # pixels strictly between the two fill values, so that a fill value found inside a tile's view is a wrong view
    return np.random.default_rng(seed).integers(1, np.iinfo(dtype).max, shape).astype(dtype)


def _assert_layout(layout, stack):
    n, h, w = stack.shape
    top = np.iinfo(stack.dtype).max
    assert layout.shape == (n, h, w) and layout.buffer.dtype == stack.dtype and layout.buffer.ndim == 1
    np.testing.assert_array_equal(T.tiles_of(layout), stack)
    flat = layout.buffer
    for t in (0, n - 1):
        for y in (0, h - 1):
            start = layout.base_offset + t * layout.tile_stride + y * layout.pitch
            np.testing.assert_array_equal(flat[start:start + w], stack[t, y])
    # whatever is no pixel of a tile is fill: 0 at even indices of the buffer, the maximum at odd ones
    outside = np.ones(flat.size, dtype=bool)
    index = (layout.base_offset + np.arange(n)[:, None, None] * layout.tile_stride + np.arange(h)[None, :, None] * layout.pitch
             + np.arange(w)[None, None, :]).ravel()
    assert len(np.unique(index)) == n * h * w and index.max() < flat.size       # the tiles neither overlap nor leave the buffer
    outside[index] = False
    where = np.flatnonzero(outside)
    np.testing.assert_array_equal(flat[where], (where & 1) * top)
    pad = T.padding_of(layout)
    assert pad.shape == (n, h, layout.pitch - w)
    if pad.shape[2] >= 2:
        assert ((pad == 0).any(axis=2) & (pad == top).any(axis=2)).all()        # every row's padding holds both values
    if layout.base_offset >= 2:
        assert set(flat[:layout.base_offset].tolist()) == {0, top}
    tail = flat[layout.base_offset + (n - 1) * layout.tile_stride + (h - 1) * layout.pitch + w:]
    assert len(tail) >= T.LINE and set(tail.tolist()) == {0, top}


@pytest.mark.parametrize('dtype', ['uint16', 'uint8'])
@pytest.mark.parametrize('pad,base_offset,gap', [(0, 0, 0), (1, 0, 0), (3, 1, 0), (2, 5, 7), (8, 16, 1)])
def test_padded_buffer_holds_the_stack_and_fill_around_it(dtype, pad, base_offset, gap):
    stack = _stack(dtype, (4, 6, 11))
    layout = T.padded(stack, pad, base_offset, gap)
    assert (layout.base_offset, layout.pitch, layout.tile_stride) == (base_offset, 11 + pad, 6 * (11 + pad) + gap)
    _assert_layout(layout, stack)
    T.tiles_of(layout)[...] = 0          # the view is the buffer, not a copy
    assert not layout.buffer[base_offset:base_offset + 11].any()


@pytest.mark.parametrize('dtype', ['uint16', 'uint8'])
def test_separate_tiles_are_buffers_of_their_own_at_offsets_of_their_own(dtype):
    stack = _stack(dtype, (7, 5, 9), seed=1)
    singles = T.separate(stack, 3)
    assert len(singles) == 7
    for t, single in enumerate(singles):
        _assert_layout(single, stack[t:t + 1])
        assert single.pitch == 12
        assert all(not np.shares_memory(single.buffer, other.buffer) for other in singles[:t])
    offsets = [s.base_offset for s in singles]
    assert offsets == [1, 4, 7, 10, 13, 0, 3]
    assert len({o % T.vec(dtype) for o in offsets}) >= 5       # the tiles differ in alignment
    assert [s.base_offset for s in T.separate(stack[:2], 3, offsets=[9, 2])] == [9, 2]


def test_row_phases():
    layout = T.padded(_stack('uint16', (3, 4, 5)), 3, base_offset=1, gap=2)      # pitch 8: every row of a tile at one phase
    assert T.row_phases(layout).tolist() == [[1] * 4, [3] * 4, [5] * 4]
    layout = T.padded(_stack('uint8', (2, 3, 5)), 2, base_offset=15)
    assert T.row_phases(layout).tolist() == [[15, 6, 13], [4, 11, 2]]
    assert T.row_phases(layout, tiles=1, rows=2).tolist() == [[15, 6]]


@pytest.mark.parametrize('dtype,w', [(d, w) for d in ('uint16', 'uint8') for w in T.MINMAX_WIDTHS[d]])
def test_minmax_case_plants_strict_extremes_at_every_position_and_phase(dtype, w):
    stack, max_at, min_at, base_offset, gap = T.minmax_case(dtype, w)
    n = len(stack)
    assert stack.shape == (n, T.MINMAX_H, w) and n >= max(16, 3 * w) and base_offset in T.MINMAX_BASES
    lo, hi = T.MINMAX_INTERIOR[dtype]
    flat = stack.reshape(n, -1).astype(np.int64)
    for at, value, inner in ((max_at, flat.max(axis=1), hi), (min_at, flat.min(axis=1), lo)):
        planted = stack[np.arange(n), at[:, 0], at[:, 1]]
        np.testing.assert_array_equal(planted, value)
        assert ((flat == value[:, None]).sum(axis=1) == 1).all()                # strict
        assert (np.abs(value - inner) >= 1).all() and len(set(value.tolist())) > 1
        assert 0 < value.min() and value.max() < np.iinfo(dtype).max            # not a fill value
        # every position of the planted rows, once or (a narrow tile) equally often
        counts = {}
        for y, x in at.tolist():
            counts[(y, x)] = counts.get((y, x), 0) + 1
        assert set(counts) == {(y, x) for y in T.MINMAX_ROWS for x in range(w)} and len(set(counts.values())) == 1
    layout = T.minmax_layout(dtype, w)
    assert layout.pitch == w + T.MINMAX_PAD and layout.tile_stride % 2 == 1
    assert T.first_rows_phases(layout) == set(range(T.vec(dtype)))
    assert len(set(T.row_phases(layout, tiles=1, rows=2).ravel().tolist())) == 2      # consecutive rows change phase
    if stack.size <= 1 << 20:            # (the two widest are the same code at a size that takes seconds to index)
        _assert_layout(layout, stack)
    else:
        np.testing.assert_array_equal(T.tiles_of(layout), stack)


@pytest.mark.parametrize('name', sorted(T.NAMED))
def test_named_layouts_meet_every_phase_in_their_first_rows(name):
    dtype, shape, pad, base_offset, gap = T.NAMED[name]
    stack = _stack(dtype, shape, seed=2)
    layout = T.named(name, stack)
    np.testing.assert_array_equal(T.tiles_of(layout), stack)
    assert pad >= 2 and base_offset >= 1
    if name in T.ONE_PHASE:
        assert set(T.row_phases(layout).ravel().tolist()) == {T.ONE_PHASE[name]} and T.ONE_PHASE[name] != 0
    else:
        assert T.first_rows_phases(layout) == set(range(T.vec(dtype)))
    singles = T.named_separate(name, stack)
    assert len({s.base_offset % T.vec(dtype) for s in singles}) == min(len(singles), T.vec(dtype))
    for t, single in enumerate(singles):
        np.testing.assert_array_equal(T.tiles_of(single)[0], stack[t])
