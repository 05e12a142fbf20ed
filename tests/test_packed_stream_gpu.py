"""The scaffold the three device encoders share (csrc/packed_stream.h): the empty geometry, the refusal of a negative capacity,
and the one scan kernel under the encoder whose own tests did not walk around its width (Blosc does in test_blosc_edges_gpu,
JPEG at 1024 / 1025 / 2625 tiles in test_jpeg_edges_gpu)."""
import numpy as np
import pytest

import deflate_ref
from image_stitcher_amd import native

pytestmark = pytest.mark.gpu

ENCODERS = {'blosc': (), 'deflate': (2,), 'jpeg': (90,)}      # the codec's own arguments behind the tile shape


def _call(codec, n_planes, capacity=None, status_preset=1):
    """sq_<codec>_encode_planes of ``n_planes`` 16 x 16 uint8 planes, one 16 x 16 tile each -> (rc, message, offsets, status)."""
    import torch
    dev = torch.device('cuda:0')
    L = native.lib()
    geo = (n_planes, 16, 16, native.SQ_U8, 16, 16)
    need, bound = int(getattr(L, f'sq_{codec}_scratch_bytes')(*geo)), int(getattr(L, f'sq_{codec}_out_bound')(*geo))
    assert need >= 256 and bound >= 0
    planes = torch.full((max(n_planes, 1), 16, 16), 7, dtype=torch.uint8, device=dev)
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    offsets = torch.full((n_planes + 1,), 77, dtype=torch.int64, device=dev)
    out = torch.empty(max(bound, 1), dtype=torch.uint8, device=dev)
    status = torch.full((1,), status_preset, dtype=torch.int32, device=dev)
    rc = getattr(L, f'sq_{codec}_encode_planes')(planes.data_ptr(), 256, 16, *geo, *ENCODERS[codec], scratch.data_ptr(), need,
                                                offsets.data_ptr(), out.data_ptr(), bound if capacity is None else capacity,
                                                status.data_ptr(), native._stream_ptr())
    torch.cuda.synchronize()
    return rc, L.sq_last_error().decode(), offsets.cpu().numpy(), int(status.item())


@pytest.mark.parametrize('codec', list(ENCODERS))
def test_empty_geometry_clears_the_status(codec):
    rc, _, offsets, status = _call(codec, 0)
    assert rc == 0 and status == 0 and offsets[0] == 0


@pytest.mark.parametrize('codec', list(ENCODERS))
def test_negative_capacity_is_refused(codec):
    rc, message, offsets, status = _call(codec, 1, capacity=-1)
    assert rc == native.SQ_ERR_INVALID and message == f'sq_{codec}_encode_planes: negative out_capacity'
    assert status == 1 and offsets[0] == 77                              # nothing ran


@pytest.mark.parametrize('count', [1023, 1024, 1025, 2049])
def test_deflate_tile_counts_around_the_scan_width(count):
    """The scan gives each of its 1024 threads (n + 1023) / 1024 consecutive sizes: one per thread up to 1024 tiles, two from 1025
    (the last threads idle), three at 2049.  Tiles of 1 x 16 bytes, all zero but the first, the 1024th and the last."""
    import torch
    plane = np.zeros((1, count, 16), np.uint8)
    rows = sorted({0, min(1023, count - 1), count - 1})
    plane[0, rows] = np.random.default_rng(count).integers(1, 256, (len(rows), 16), dtype=np.uint8)
    want = np.array([len(s) for s in deflate_ref.encode_planes(plane, 1, 16, 2)])
    assert [int(i) for i in np.nonzero(want)[0]] == rows
    buf = native.deflate_encode_planes(torch.from_numpy(plane).to('cuda:0'), 1, 16, 2)
    torch.cuda.synchronize()
    assert int(buf.status.item()) == 0 and buf.n_chunks == count
    assert np.array_equal(buf.offsets.cpu().numpy(), np.concatenate([[0], np.cumsum(want)]))
