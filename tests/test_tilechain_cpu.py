"""The byte accounting of the staged-tile filter chain (image_stitcher_amd/tilechain.py): integers only, no device.  The per-plane
count the batch budget is divided by and the stream writer's smaller count, against the plain sum of the chain's buffers, over
every combination of the options that allocate one.  The arithmetic is exact."""
import itertools

import numpy as np
import pytest

from image_stitcher_amd.tilechain import TileChain

FH, FW = 97, 131      # no multiple of 2 or 3: the binned tiles drop rows and columns
NUM_Z = 2
DPC_PLANES = range(2 * NUM_Z, 3 * NUM_Z)      # the derived channel is the third of four
GRID = list(itertools.product((0, 20000), (1, 2, 3), ('none', 'hot'), (False, True), (False, True), ('uint8', 'uint16')))


def _chain(ppm, k, despeckle, tophat, dpc, dtype):
    return TileChain(distortion_ppm=ppm, binning=k, binning_method='mean', dpc_planes=DPC_PLANES if dpc else (), dpc_gain=1,
                     despeckle=despeckle, despeckle_threshold=40, tophat_radius=5 if tophat else None, seam_qc_radius=2,
                     file_shape=(FH, FW), tile_shape=(FH // k, FW // k), dtype=dtype)


def _oracle(n, ppm, k, despeckle, tophat, derived, dtype):
    """(bytes per staged plane of n tiles, the stream writer's count of one): buffer by buffer."""
    b = np.dtype(dtype).itemsize
    raw, tile = n * FH * FW * b, n * (FH // k) * (FW // k) * b
    total = writer = raw                  # the staged planes as they are in their files (the ingest slot's device mirror)
    if derived:
        total += raw                      # the right halves, counted as one more copy though only the derived planes have one
    if ppm:
        total += raw                      # the corrected copy of the staged planes
        writer += raw
        if derived:
            total += raw                  # ... and of the right halves
    if k > 1:
        total += tile                     # the binned copy of the staged planes
        writer += tile
        if derived:
            total += tile                 # ... and of the right halves
    if despeckle != 'none':
        total += tile                     # the despeckle's destination
    if tophat:
        total += tile                     # the top-hat's scratch: the erosion, as many bytes as the tiles
    return total, writer


@pytest.mark.parametrize('n', [1, 6])
def test_counts_equal_the_sum_of_the_buffers(n):
    seen = set()
    for ppm, k, despeckle, tophat, dpc, dtype in GRID:
        chain = _chain(ppm, k, despeckle, tophat, dpc, dtype)
        for plist in ([0, 1, 2, 3], [3, 4, 5, 6], [4], [6, 7]):      # without, with, only and behind the derived planes
            positions = chain.derived(plist)
            assert positions == ([i for i, p in enumerate(plist) if p in DPC_PLANES] if dpc else [])
            derived = bool(positions)
            want, want_writer = _oracle(n, ppm, k, despeckle, tophat, derived, dtype)
            assert chain.plane_bytes(n, derived) == want, (ppm, k, despeckle, tophat, dpc, dtype, plist)
            assert chain.writer_plane_bytes(n) == want_writer, (ppm, k, despeckle, tophat, dpc, dtype, plist)
            seen.add((bool(ppm), k, despeckle, tophat, derived))
    assert len(seen) == 2 * 3 * 2 * 2 * 2      # the whole grid, with and without derived planes


def test_cache_keys():
    chain = _chain(20000, 2, 'hot', True, True, 'uint16')
    th, tw = FH // 2, FW // 2
    assert chain.key('ingest', 3, 6, 2) == ('ingest', 3, 6, FH, FW, 2, '<u2')
    assert chain.key('dpc', 2, 6, 2) == ('dpc', 2, 6, FH, FW, 2, '<u2')
    assert chain.key('distortion', 3, 6) == ('distortion', 3, 6, FH, FW, '<u2')
    assert chain.key('distortion-dpc', 2, 6) == ('distortion-dpc', 2, 6, FH, FW, '<u2')
    for name in ('binning', 'despeckle', 'tophat'):
        assert chain.key(name, 3, 6) == (name, 3, 6, th, tw, '<u2')
    assert chain.key('binning-dpc', 2, 6) == ('binning-dpc', 2, 6, th, tw, '<u2')
    assert _chain(0, 1, 'none', False, False, 'uint8').key('ingest', 1, 4, 1) == ('ingest', 1, 4, FH, FW, 1, '|u1')
