"""Tiles as a C caller may hand them to the registration entry points (include/squidstitch.h: tile_pitch, tile_stride, a base
pointer or a pointer table): padded rows, a gap between tiles, a lead-in before the first tile and a tail after the last, and
tiles that are allocations of their own at offsets of their own.  Nothing here needs a device.

All offsets are in ELEMENTS: row y of tile t starts at  base_offset + t * tile_stride + y * pitch  of the flat buffer.
Everything that is no pixel of a tile -- row padding, gaps, lead-in, tail -- holds 0 and the dtype's maximum alternately (by
the parity of its index in the buffer), so a read outside a tile's W columns moves a minimum, a maximum, a moment or a
normalised crop.

The second half names the layouts tests/test_register_inputs_gpu.py runs, so that tests/test_tile_layouts_cpu.py can hold them
to what they are there for (rows at every alignment phase of a 16-byte line) without a device."""
from collections import namedtuple

import numpy as np

LINE = 16      # bytes of the vector loads of minmax_kernel and rows_forward_block

Layout = namedtuple('Layout', 'buffer base_offset tile_stride pitch shape')      # shape = (n, h, w)


def vec(dtype) -> int:
    """Pixels per 16-byte line = alignment phases a row can start at."""
    return LINE // np.dtype(dtype).itemsize


def padded(stack, pad, base_offset=0, gap=0, tail=LINE) -> Layout:
    """The dense [N, H, W] uint8 / uint16 `stack` with rows `pad` elements apart, tiles `gap` more than H rows apart, behind
    `base_offset` elements and before `tail` more."""
    stack = np.asarray(stack)
    assert stack.ndim == 3 and stack.dtype in (np.uint8, np.uint16) and min(pad, base_offset, gap, tail) >= 0
    n, h, w = stack.shape
    pitch = w + pad
    tile_stride = h * pitch + gap
    total = base_offset + n * tile_stride + tail
    buffer = ((np.arange(total) & 1) * np.iinfo(stack.dtype).max).astype(stack.dtype)
    layout = Layout(buffer, base_offset, tile_stride, pitch, (n, h, w))
    tiles_of(layout)[...] = stack
    return layout


def _strided(layout, first_column, columns):
    n, h, _ = layout.shape
    size = layout.buffer.itemsize
    return np.lib.stride_tricks.as_strided(layout.buffer[layout.base_offset + first_column:], shape=(n, h, columns),
                                           strides=(layout.tile_stride * size, layout.pitch * size, size))


def tiles_of(layout):
    """The [N, H, W] view of the tiles in the buffer."""
    return _strided(layout, 0, layout.shape[2])


def padding_of(layout):
    """The [N, H, pitch - W] view of what lies behind every row."""
    return _strided(layout, layout.shape[2], layout.pitch - layout.shape[2])


def separate(stack, pad, offsets=None):
    """One single-tile Layout per tile, for a pointer table: a buffer of its own each, its tile behind offsets[t] elements
    (by default 1, 4, 7, ... modulo 16, so that the tiles differ in alignment and tile 5 is an aligned one)."""
    stack = np.asarray(stack)
    if offsets is None:
        offsets = [(1 + 3 * t) % LINE for t in range(len(stack))]
    return [padded(stack[t:t + 1], pad, base_offset=int(off)) for t, off in enumerate(offsets)]


def row_phases(layout, tiles=None, rows=None):
    """Alignment phase, in elements of a 16-byte line, of the given rows of the given tiles (all by default) -- of a buffer that
    itself starts on a line, which a test on the device asserts of its allocation."""
    n, h, _ = layout.shape
    t = np.arange(n if tiles is None else min(n, tiles))[:, None]
    y = np.arange(h if rows is None else min(h, rows))[None, :]
    return (layout.base_offset + t * layout.tile_stride + y * layout.pitch) % vec(layout.buffer.dtype)


def first_rows_phases(layout):
    """The phases the first rows meet: of the first vec rows of tile 0 when those can differ in all of them (an odd pitch and a
    tile that high), else of every row of the first vec tiles."""
    v = vec(layout.buffer.dtype)
    if layout.pitch % 2 == 1 and layout.shape[1] >= v:
        return set(row_phases(layout, tiles=1, rows=v).ravel().tolist())
    return set(row_phases(layout, tiles=v).ravel().tolist())


# ---- sq_tile_minmax: one tile per pixel position ---------------------------------------------------------------------------
MINMAX_H = 9                     # 2 blocks, 8 waves: row 8 is a wave's second row
MINMAX_ROWS = (0, 4, 8)
MINMAX_WIDTHS = {                # every shape of the head / vector / tail split; the last has more than 64 vectors a row
    'uint16': (1, 7, 8, 9, 23, 523),
    'uint8': (1, 15, 16, 17, 47, 1043),
}
MINMAX_PAD = 3                   # consecutive rows change phase
MINMAX_BASES = (0, 1, 5)
MINMAX_INTERIOR = {'uint16': (1000, 2000), 'uint8': (100, 150)}


def minmax_case(dtype, w):
    """(stack [N, 9, w], max_at, min_at, base_offset, gap): for every position (row in MINMAX_ROWS, column) one tile whose
    interior is mid-range, whose only maximum sits at that position (max_at[t] = (y, x)) and whose only minimum sits
    w // 2 + 1 columns further on, wrapping within the row -- in a one-column tile, where that is the same pixel, one planted
    row further on instead.  Every position is a maximum once and a minimum once.  A width with fewer than 16 positions
    repeats them until there are 16 tiles, so that with the odd tile stride every row meets every phase.  The planted values
    differ from tile to tile."""
    dtype = np.dtype(dtype)
    lo, hi = MINMAX_INTERIOR[dtype.name]
    positions = [(y, x) for y in MINMAX_ROWS for x in range(w)]
    positions = positions * -(-LINE // len(positions))
    n = len(positions)
    rng = np.random.default_rng(1000 + w)
    stack = rng.integers(lo, hi + 1, (n, MINMAX_H, w)).astype(dtype)
    max_at = np.array(positions)
    min_at = max_at.copy()
    if w == 1:
        min_at[:, 0] = [MINMAX_ROWS[(MINMAX_ROWS.index(y) + 1) % len(MINMAX_ROWS)] for y in max_at[:, 0]]
    else:
        min_at[:, 1] = (max_at[:, 1] + w // 2 + 1) % w
    t = np.arange(n)
    room = min(lo, np.iinfo(dtype).max - hi) - 1
    stack[t, max_at[:, 0], max_at[:, 1]] = hi + 1 + t % room
    stack[t, min_at[:, 0], min_at[:, 1]] = lo - 1 - (t * 7) % room
    widths = MINMAX_WIDTHS[dtype.name]
    base_offset = MINMAX_BASES[widths.index(w) % len(MINMAX_BASES)]
    gap = 2 if (MINMAX_H * (w + MINMAX_PAD)) % 2 else 3        # an odd tile stride: consecutive tiles change phase too
    return stack, max_at, min_at, base_offset, gap


def minmax_layout(dtype, w) -> Layout:
    stack, _, _, base_offset, gap = minmax_case(dtype, w)
    return padded(stack, MINMAX_PAD, base_offset, gap)


# ---- the other layouts, by name: (dtype, (n, h, w), pad, base_offset, gap) ---------------------------------------------------
def _moments_shape(w):
    """Three tiles that hold a w-wide window three rows higher than a band of sq_pair_overlap_moments (16384 // w rows) at
    origins of up to (4, 3); of an even width, so that the pitch 3 wider is odd."""
    return (3, 16384 // w + 3 + 5, w + 6 + w % 2)


MOMENTS_WIDTHS = (1, 63, 64, 65, 300)
NAMED = {
    'normalize': ('uint16', (5, 37, 61), 4, 3, 5),
    'normalize-u8': ('uint8', (5, 37, 61), 4, 3, 5),
    'register-pitch99': ('uint16', (12, 160, 96), 3, 1, 7),
    'register-pitch104': ('uint16', (12, 160, 96), 8, 1, 8),      # every row ONE element behind a line: the same phase
    'register-u8': ('uint8', (10, 48, 48), 5, 1, 3),
    'register-long': ('uint16', (2, 8, 12288), 3, 1, 2),
}
for _dtype in ('uint16', 'uint8'):
    for _w in MOMENTS_WIDTHS:
        NAMED[f'moments-{_dtype}-w{_w}'] = (_dtype, _moments_shape(_w), 3, 1, 2)
ONE_PHASE = {'register-pitch104': 1}      # the layouts whose rows are meant to share one phase, and which phase that is


def named(name, stack) -> Layout:
    dtype, shape, pad, base_offset, gap = NAMED[name]
    stack = np.asarray(stack)
    assert stack.dtype == np.dtype(dtype) and stack.shape == shape, f'{name}: a {stack.dtype} stack of {stack.shape}'
    return padded(stack, pad, base_offset, gap)


def named_separate(name, stack):
    dtype, shape, pad, _, _ = NAMED[name]
    stack = np.asarray(stack)
    assert stack.dtype == np.dtype(dtype) and stack.shape == shape, f'{name}: a {stack.dtype} stack of {stack.shape}'
    return separate(stack, pad)
