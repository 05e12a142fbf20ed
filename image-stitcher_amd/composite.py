"""--composite: one colour quick-look PNG (and a JSON sidecar) per (timepoint, region).

The reference's dormant ``_save_debug_slice`` (stitcher.py:861-885) writes the first three channels as RGB, min/max normalised,
from a host copy of the whole stack.  Here the source planes -- the projection a run writes, or one z plane of the stack -- are
reduced where they are final on the device (``native.block_mean``, csrc/composite.hip) to block means of at most
``max_side`` pixels a side; their windows are ``omezarr.contrast_window`` of the exact value counts of the source
(``native.histogram_planes``), and ``native.composite_render`` adds the windowed planes in their channel colours.  Integers
only; the definition is the numpy restatement in tests/composite_ref.py ("Composite").
"""
from __future__ import annotations

import json
import os
from typing import List, Optional, Sequence

import numpy as np

from . import omezarr, png

MAX_K = 8                       # a 256 x 256 block sum of uint16 values fits 32 bits
MAX_SIDE_RANGE = (16, 16384)
MAX_CHANNELS = 16               # planes one sq_composite_render call adds


def check_options(composite, max_side, z, channels) -> tuple:
    """-> (composite, max_side, z, channels) validated at construction: max_side an integer in 16..16384, z None or an integer
    >= 0 (its upper bound is known once the metadata is parsed), channels None or 1..16 distinct names."""
    if isinstance(max_side, bool) or not isinstance(max_side, (int, np.integer)) or \
            not MAX_SIDE_RANGE[0] <= int(max_side) <= MAX_SIDE_RANGE[1]:
        raise ValueError(f"composite_max_side must be an integer in {MAX_SIDE_RANGE[0]}..{MAX_SIDE_RANGE[1]}, got {max_side!r}")
    if z is not None and (isinstance(z, bool) or not isinstance(z, (int, np.integer)) or int(z) < 0):
        raise ValueError(f"composite_z must be a z level (an integer >= 0), got {z!r}")
    if channels is not None:
        if isinstance(channels, str) or not all(isinstance(c, str) for c in channels):
            raise ValueError(f"composite_channels must be a list of channel names, got {channels!r}")
        channels = list(channels)
        if not 1 <= len(channels) <= MAX_CHANNELS or len(set(channels)) != len(channels):
            raise ValueError(f"composite_channels must be 1..{MAX_CHANNELS} distinct channel names, got {channels!r}")
    return bool(composite), int(max_side), (None if z is None else int(z)), channels


def choose_level(height: int, width: int, max_side: int) -> int:
    """The smallest k >= 0 with max(ceil(H / 2^k), ceil(W / 2^k)) <= max_side; k <= 8 or a ValueError that names the smallest
    max_side that works."""
    height, width, max_side = int(height), int(width), int(max_side)
    if height < 1 or width < 1 or max_side < 1:
        raise ValueError(f"choose_level: bad sizes {height} x {width}, max_side {max_side}")
    k = 0
    while max(-(-height // (1 << k)), -(-width // (1 << k))) > max_side:
        k += 1
    if k > MAX_K:
        need = -(-max(height, width) // (1 << MAX_K))
        raise ValueError(f"a {height} x {width} image needs blocks of {1 << k} pixels a side to fit composite_max_side = {max_side}; "
                         f"blocks go up to {1 << MAX_K} (their sums are kept in 32 bits): the smallest composite_max_side that "
                         f"works is {need}")
    return k


def sidecar(*, store: str, kind: str, z: Optional[int], level: int, shape: Sequence[int], source_shape: Sequence[int],
            labels: Sequence[str], colors: Sequence[int], windows: Sequence[tuple], percentiles: Sequence[float]) -> dict:
    """What ``<stem>_composite.json`` records."""
    return {'source': {'store': store, 'kind': kind, 'z': None if z is None else int(z)},
            'level': int(level), 'factor': 1 << int(level), 'shape': [int(v) for v in shape],
            'source_shape': [int(v) for v in source_shape],
            'channels': [{'label': str(n), 'color': f'{int(c) & 0xFFFFFF:06X}', 'window': {'start': int(a), 'end': int(b)}}
                         for n, c, (a, b) in zip(labels, colors, windows)],
            'percentiles': [float(percentiles[0]), float(percentiles[1])]}


def write_outputs(stem: str, rgb, meta: dict) -> tuple:
    """``<stem>.png`` and ``<stem>.json``."""
    png.write_rgb8(stem + '.png', rgb)
    with open(stem + '.json', 'w') as fh:
        json.dump(meta, fh, indent=1)
    return stem + '.png', stem + '.json'


class CompositeTarget:
    """The device state of one region's composite: ``means`` [n, h, w] (zero-initialised: what no rank or batch writes is the
    canvas' zero) and the value counts of the source planes.  ``add`` is called where a source plane (or a row band of it) is
    final on the device, on the stream that writes it to its store.

    ``channels``: indices into the run's output channels, in composite order.  ``z``: the stack's z level the source is, or None
    when the source is a projection store (Z = 1).  ``shared_hist``: the projection store's own [C, bins] histogram target
    (--contrast-limits percentile): it holds the same counts, so nothing is counted twice."""

    def __init__(self, stem: str, *, store: str, kind: str, z: Optional[int], channels: Sequence[int], labels: Sequence[str],
                 colors: Sequence[int], height: int, width: int, max_side: int, dtype, percentiles, device, shared_hist=None):
        import torch
        from . import native
        self.stem, self.store, self.kind, self.z = stem, store, kind, z
        self.channels = [int(c) for c in channels]
        self.labels, self.colors = list(labels), [int(c) for c in colors]
        self.height, self.width = int(height), int(width)
        self.level = choose_level(height, width, max_side)
        self.factor = 1 << self.level
        self.shape = (-(-self.height // self.factor), -(-self.width // self.factor))
        self.dtype = np.dtype(dtype)
        self.percentiles = (float(percentiles[0]), float(percentiles[1]))
        self._index = {c: i for i, c in enumerate(self.channels)}
        self.means = torch.zeros((len(self.channels),) + self.shape, dtype=native.torch_dtype_of(self.dtype), device=device)
        self.counts_own = shared_hist is None
        self.hist = shared_hist if shared_hist is not None else \
            torch.zeros((len(self.channels), native.histogram_bins(self.dtype)), dtype=torch.int64, device=device)

    def add(self, planes, coords, row_offset: int = 0) -> None:
        """``planes`` [m, rows, W]: the planes ``coords`` = [(t, c, z)] as written to level 0 of the store, rows
        ``row_offset`` ... of them.  Planes that are not a source of the composite are skipped."""
        from . import native
        f = self.factor
        rows = int(planes.shape[1])
        if row_offset % f or (rows % f and row_offset + rows != self.height) or int(planes.shape[2]) != self.width:
            raise ValueError(f"composite: rows {row_offset} + {rows} x {int(planes.shape[2])} of a {self.height} x {self.width} "
                             f"source do not fall on blocks of {f}")
        y = row_offset // f
        for i, (_, c, z) in enumerate(coords):
            j = self._index.get(int(c))
            if j is None or (self.z is not None and int(z) != self.z):
                continue
            native.block_mean(planes[i:i + 1], self.level, out=self.means[j:j + 1, y:y + -(-rows // f)])
            if self.counts_own:
                native.histogram_planes(planes[i:i + 1], [j], hist=self.hist)

    def counts(self, hist_host) -> np.ndarray:
        """[n, bins] counts in composite order from the host copy of ``hist``."""
        h = np.asarray(hist_host)
        return h if self.counts_own else h[self.channels]

    def windows(self, counts) -> List[tuple]:
        lo, hi = self.percentiles
        top = int(np.iinfo(self.dtype).max)
        return [omezarr.contrast_window(row, lo, hi, top) for row in np.asarray(counts)]

    def render(self, windows, means=None):
        """-> RGB8 [h, w, 3] numpy (waits for the current stream)."""
        from . import native
        return native.composite_render(self.means if means is None else means, windows, self.colors).cpu().numpy()

    def meta(self, windows) -> dict:
        return sidecar(store=self.store, kind=self.kind, z=self.z, level=self.level, shape=self.shape,
                       source_shape=(self.height, self.width), labels=self.labels, colors=self.colors, windows=windows,
                       percentiles=self.percentiles)
