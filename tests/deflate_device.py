"""What the device tile-encoder tests share (tests/test_deflate_gpu.py, tests/test_deflate_edges_gpu.py): plane stacks on the device,
dense or padded, one encode through the binding, and the checks of every stream against tests/deflate_ref.py -- it inflates to its
tile's predicted bytes; it is as long as the restated rules make it."""
import zlib

import numpy as np

import deflate_ref as R
import tile_layouts
from image_stitcher_amd import native


def _dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def device_planes(planes_np, padded: bool):
    """The stack on the device: dense, or with a padded pitch and plane stride behind a lead-in (tile_layouts.padded)."""
    import torch
    if not padded:
        return torch.from_numpy(planes_np).to(_dev())
    lay = tile_layouts.padded(planes_np, pad=5, base_offset=16, gap=11)
    n, h, w = lay.shape
    buf = torch.from_numpy(lay.buffer).to(_dev())
    return torch.as_strided(buf, (n, h, w), (lay.tile_stride, lay.pitch, 1), lay.base_offset)


def streams_of(buf):
    """The stream of every tile (b'' for an all-zero one) of buffers whose stream has run."""
    offsets, out = buf.offsets.cpu().numpy(), buf.out.cpu().numpy()
    assert offsets[0] == 0 and np.all(np.diff(offsets) >= 0) and offsets[-1] <= buf.bound == len(out)
    assert len(offsets) == buf.n_chunks + 1
    return [out[offsets[i]:offsets[i + 1]].tobytes() for i in range(len(offsets) - 1)]


def encode(planes_np, th, tw, predictor, padded=False):
    """-> (the stream of every tile, b'' for an all-zero one; the buffers)."""
    import torch
    buf = native.deflate_encode_planes(device_planes(planes_np, padded), th, tw, predictor)
    torch.cuda.synchronize()
    assert int(buf.status.item()) == 0
    return streams_of(buf), buf


def check_streams(streams, planes_np, th, tw, predictor):
    """Every stream inflates to its tile's predicted bytes, to the last block and the checksum."""
    want = R.expected_tiles(planes_np, th, tw, predictor)
    assert len(streams) == len(want)
    for i, (s, w) in enumerate(zip(streams, want)):
        if not w:
            assert s == b'', f'tile {i} is all zero and has a stream of {len(s)} bytes'
            continue
        assert s[:2] == b'\x78\x01', f'tile {i}: zlib header {s[:2].hex()}'
        d = zlib.decompressobj()
        got = d.decompress(s)
        assert d.eof and d.unused_data == b'', f'tile {i}: the stream does not end with its last block and checksum'
        assert got == w, f'tile {i}: inflated bytes differ'
    return want


def check_exact(planes_np, th, tw, predictor, padded=False):
    """Every stream inflates to its tile's predicted bytes; -> (total stream bytes, raw bytes of all tiles, streams)."""
    streams, _ = encode(planes_np, th, tw, predictor, padded)
    want = check_streams(streams, planes_np, th, tw, predictor)
    raw = len(want) * th * tw * planes_np.dtype.itemsize
    return sum(len(s) for s in streams), raw, streams


def check_sizes(streams, planes_np, th, tw, predictor, label=''):
    """Every stream is exactly as long as the stream of tests/deflate_ref.py: its length follows from the rules alone (runs, their
    pieces, a minimum-redundancy code under the limit, the header, the flush, stored or dynamic), whatever the order of ties.  The
    bytes may differ: how many tiles are identical is printed, not asserted.  (Pure Python: tiles of a few segments only.)"""
    assert th * tw * planes_np.dtype.itemsize <= 8 * R.SEG
    ref = R.encode_planes(planes_np, th, tw, predictor)
    assert len(ref) == len(streams)
    same = sum(a == b for a, b in zip(streams, ref))
    print(f'{label}: {len(ref)} tiles, {sum(map(len, streams))} device / {sum(map(len, ref))} reference bytes, '
          f'{same} streams byte-identical')
    wrong = [(i, len(s), len(r)) for i, (s, r) in enumerate(zip(streams, ref)) if len(s) != len(r)]
    assert not wrong, f'{label}: (tile, device bytes, reference bytes) {wrong[:8]} -- {len(wrong)} of {len(ref)} tiles differ'
    return same
