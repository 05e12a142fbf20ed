"""What the device JPEG-encoder tests share (tests/test_jpeg_gpu.py, tests/test_jpeg_edges_gpu.py): the streams out of a call's
buffers, and one encode through the binding held byte for byte to ``jpegtile.encode_tile`` of every zero-padded tile."""
import numpy as np

import jpeg_cases as K
from deflate_device import _dev, device_planes
from image_stitcher_amd import native


def device_streams(buf):
    offsets, out = buf.offsets.cpu().numpy(), buf.out.cpu().numpy()
    assert offsets[0] == 0 and np.all(np.diff(offsets) >= 0) and offsets[-1] <= buf.bound
    assert len(offsets) == buf.n_chunks + 1
    return [out[offsets[i]:offsets[i + 1]].tobytes() for i in range(len(offsets) - 1)]


def first_difference(got: bytes, want: bytes) -> str:
    n = min(len(got), len(want))
    at = next((i for i in range(n) if got[i] != want[i]), n)
    return f'{len(got)} device / {len(want)} host bytes, first difference at {at}: {got[at:at + 8].hex()} / {want[at:at + 8].hex()}'


def guarded_planes(planes_np, layout):
    """The stack on the device inside a buffer of K.GUARD bytes (K.guarded): pitch, plane stride and the base's offset behind a
    256-byte boundary as `layout` says."""
    import torch
    pitch, stride, _ = layout
    host, at = K.guarded(planes_np, layout)
    buf = torch.from_numpy(host).to(_dev())
    assert buf.data_ptr() % 256 == 0, 'the allocation is not on a 256-byte boundary: the layouts would not be what they say'
    return torch.as_strided(buf, planes_np.shape, (stride, pitch, 1), at)


def check_equal(planes, th, tw, quality, padded, label):
    """`padded`: False dense, True deflate_device's odd pitch, or a K.guarded layout.  -> the device's streams."""
    import torch
    n, h, w = planes.shape
    worst = int(native.lib().sq_jpeg_out_bound(n, h, w, native.SQ_U8, th, tw))
    dev = guarded_planes(planes, padded) if isinstance(padded, tuple) else device_planes(planes, padded)
    buf = native.jpeg_encode_planes(dev, th, tw, quality, capacity=worst)
    torch.cuda.synchronize()
    assert int(buf.status.item()) == 0, label
    got, want = device_streams(buf), K.expected_streams(planes, th, tw, quality)
    assert len(got) == len(want)
    for i, (g, w_) in enumerate(zip(got, want)):
        assert g == w_, f'{label}, tile {i}: {first_difference(g, w_)}'
    return got
