"""Device JPEG tile encoder (csrc/jpeg.hip) through the binding: the packed bytes of every tile equal
``jpegtile.encode_tile`` of the zero-padded tile BYTE FOR BYTE -- offsets included, tiles of zeros of size 0.  Inputs and what each
is there for: tests/jpeg_cases.py (tests/test_jpeg_cpu.py holds the host definition to Pillow and the contents to their purpose).
No decoder is needed here."""
import numpy as np
import pytest

import jpeg_cases as K
import stream_cases as SC
from deflate_device import _dev, device_planes
from image_stitcher_amd import jpegtile as J
from image_stitcher_amd import native
from jpeg_device import check_equal, device_streams

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('quality', K.QUALITIES)
@pytest.mark.parametrize('shape_name', [s[0] for s in K.SHAPES])
def test_streams_equal_the_host_definition(shape_name, quality):
    _, shape, (th, tw), padded = next(s for s in K.SHAPES if s[0] == shape_name)
    for name in K.CONTENTS:
        planes = K.content(name, shape, seed=len(name) + quality)
        streams = check_equal(planes, th, tw, quality, padded, f'{shape_name} {name} q{quality}')
        if name == 'zero':
            assert all(s == b'' for s in streams)
        if name == 'pixel':
            assert sum(s != b'' for s in streams) == 1
        if name == 'uniform':
            assert any(b'\xFF\x00' in K.entropy_data(s) for s in streams)


def test_the_default_tile():
    _, shape, (th, tw), padded = K.DEFAULT_SHAPE
    (s,) = check_equal(K.content('image', shape, seed=3), th, tw, 90, padded, 'default image q90')
    assert len(s) < shape[1] * shape[2] // 3


def test_too_small_a_capacity_sets_status_and_writes_nothing_past_it():
    """Noise at quality 100 does not shrink below raw.  With out_capacity = the raw size, inside a larger buffer of canaries, the
    status is set and not one byte from out_capacity on is touched (the contract promises: none at all); with
    sq_jpeg_out_bound's capacity the same call succeeds and equals the host."""
    import torch
    h, w, th, tw = 48, 80, 16, 80
    planes = K.content('uniform', (1, h, w), seed=11)
    dev = device_planes(planes, False)
    L = native.lib()
    worst = int(L.sq_jpeg_out_bound(1, h, w, native.SQ_U8, th, tw))
    assert worst == 3 * (J.HEADER_BYTES + 2 * (2 * ((10 * (20 + 63 * 26) + 7) // 8) + 2))
    buf = native.JpegBuffers(1, h, w, th, tw, _dev(), capacity=worst)
    raw = h * w
    want = K.expected_streams(planes, th, tw, 100)
    assert raw < sum(map(len, want)) <= worst
    for capacity in (raw, worst):
        buf.out.fill_(0xAB)
        rc = L.sq_jpeg_encode_planes(dev.data_ptr(), h * w, w, 1, h, w, native.SQ_U8, th, tw, 100, buf.scratch.data_ptr(),
                                     buf.scratch.numel(), buf.offsets.data_ptr(), buf.out.data_ptr(), capacity, buf.status.data_ptr(),
                                     native._stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0
        if capacity == raw:
            assert int(buf.status.item()) != 0
            assert bool((buf.out[capacity:] == 0xAB).all()), 'bytes were written at or beyond out_capacity'
            assert bool((buf.out == 0xAB).all()), 'bytes were written although the capacity was too small'
            assert int(buf.offsets[-1].item()) == sum(map(len, want))      # the size that would have been needed
        else:
            assert int(buf.status.item()) == 0
            assert device_streams(buf) == want


def test_the_default_capacity_is_raw_plus_headers():
    import torch
    planes = K.content('image', (2, 40, 72), seed=2)
    buf = native.jpeg_encode_planes(torch.from_numpy(planes).to(_dev()), 16, 16, 75)
    torch.cuda.synchronize()
    assert buf.bound == buf.n_chunks * (16 * 16 + J.HEADER_BYTES + 2) == buf.out.numel() and buf.bound < buf.worst_case
    assert int(buf.status.item()) == 0 and device_streams(buf) == K.expected_streams(planes, 16, 16, 75)


def test_uint16_and_bad_arguments_are_refused():
    import torch
    L = native.lib()
    with pytest.raises(native.NativeError) as e:
        native.jpeg_encode_planes(torch.zeros((1, 32, 32), dtype=torch.uint16, device=_dev()), 16, 16)
    assert e.value.status == native.SQ_ERR_UNSUPPORTED
    planes = torch.zeros((1, 32, 32), dtype=torch.uint8, device=_dev())
    for q in (0, 101):
        with pytest.raises(ValueError):
            native.jpeg_encode_planes(planes, 16, 16, q)
    with pytest.raises(native.NativeError) as e:
        native.jpeg_encode_planes(planes, 16, 12)
    assert e.value.status == native.SQ_ERR_INVALID
    buf = native.JpegBuffers(1, 32, 32, 16, 16, _dev())
    args = lambda q: (planes.data_ptr(), 32 * 32, 32, 1, 32, 32, native.SQ_U8, 16, 16, q, buf.scratch.data_ptr(), buf.scratch.numel(),
                      buf.offsets.data_ptr(), buf.out.data_ptr(), buf.bound, buf.status.data_ptr(), native._stream_ptr())
    assert L.sq_jpeg_encode_planes(*args(0)) == native.SQ_ERR_INVALID
    assert L.sq_jpeg_encode_planes(*args(101)) == native.SQ_ERR_INVALID


def test_buffers_are_reused_for_the_same_geometry():
    import torch
    a = K.content('image', (1, 40, 72), seed=1)
    b = K.content('gaps', (1, 40, 72))
    buf = native.jpeg_encode_planes(torch.from_numpy(a).to(_dev()), 16, 16, 50)
    again = native.jpeg_encode_planes(torch.from_numpy(b).to(_dev()), 16, 16, 50, buffers=buf)
    torch.cuda.synchronize()
    assert again is buf and int(buf.status.item()) == 0
    assert device_streams(buf) == K.expected_streams(b, 16, 16, 50)


# ---------------------------------------------------------------------------------------------------- off the default stream
DH, DW, DT = 100, 130, 64


def _planes(seed):
    return {'planes': K.content('image', (2, DH, DW), seed=seed)}


def _call(ctx, inp, out, stream):
    buf = native.jpeg_encode_planes(inp['planes'], DT, DT, 90, stream=stream)
    return {'offsets': buf.offsets, 'streams': buf.out, 'status': buf.status}


def _finish(host):
    """The streams as a fixed-size array (zero behind each stream's end): compared exactly."""
    off, data = host['offsets'], host['streams']
    assert int(host['status'][0]) == 0, f"the encoder's status word is {host['status']}"
    tiles = np.zeros((len(off) - 1, DT * DT + J.HEADER_BYTES + 2), np.uint8)
    for i in range(len(off) - 1):
        s = data[off[i]:off[i + 1]][:tiles.shape[1]]
        tiles[i, :len(s)] = s
    return {'tiles': tiles, 'sizes': np.diff(off)}


def _reference(a, strict):
    want = K.expected_streams(a['planes'], DT, DT, 90)
    tiles = np.zeros((len(want), DT * DT + J.HEADER_BYTES + 2), np.uint8)
    for i, s in enumerate(want):
        tiles[i, :len(s)] = np.frombuffer(s, np.uint8)
    return {'tiles': tiles, 'sizes': np.array([len(s) for s in want], np.int64)}


STREAM_CASE = SC.Case('jpeg-encode-planes', _planes(300), _planes(310), {}, _call, _reference, finish=_finish)


@pytest.fixture(scope='module')
def streams():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    st = SC.Streams.open(torch.device('cuda:0'))
    if st.S is None:
        pytest.fail(f'no two of {SC.MAX_DRAWS} torch streams make progress while the other, the copy stream or the default '
                    'stream is lagged: they share hardware queues, and every stream race would stay hidden')
    return st


@pytest.fixture(scope='module')
def prepared(streams):
    return SC.Prepared(STREAM_CASE, streams)


@pytest.mark.parametrize('mode', ['A', 'B'])
def test_waits_for_its_stream(streams, prepared, mode):
    r = SC.experiment_e1(prepared.case, prepared.ctx, prepared.want, streams, mode)
    assert r.probe_full, 'the probe did not read the poison in full: the lag had ended when the call began'
    assert r.mismatch is None, f'E1-{mode} {r.mismatch}'


def test_touches_no_other_stream(streams, prepared):
    r = SC.experiment_e2(prepared.case, prepared.ctx, prepared.want, streams)
    assert r.event_pending, (f"the other stream's event was complete when the outputs had been read (the call took "
                             f'{r.host_ms:.2f} ms on the host): the call waited for that stream, or its lag is too short')
    assert r.first is None, f'E2, the other stream still lagged: {r.first}'
    assert r.after is None, f'E2, after the other stream has drained: {r.after}'
