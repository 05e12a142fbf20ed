"""Device tile encoder (csrc/deflate.hip) through the C-ABI binding: every tile's stream is inflated by ``zlib.decompress`` and
compared exactly with the bytes tests/deflate_ref.py says it encodes (the tile, zero past the plane's edge, predicted).  Inputs:
tests/deflate_cases.py.  What the ratios below are held to comes from the format, not from the encoder: Huffman coding alone
spends at least one bit per byte, so a total under 1/16 of the raw size proves that runs are coded; on the cumulative-sum planes
fixed Huffman gives 0.88 and zlib's Z_RLE 0.685 of the raw size (measured on the CPU), so 0.80 needs a dynamic code."""
import zlib

import numpy as np
import pytest

import deflate_cases as K
import deflate_ref as R
import stream_cases as SC
from deflate_device import _dev, check_exact, device_planes
from image_stitcher_amd import native

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('predictor', [1, 2])
@pytest.mark.parametrize('dtype', [np.uint8, np.uint16])
@pytest.mark.parametrize('content', K.CONTENTS)
@pytest.mark.parametrize('shape_name', [s[0] for s in K.SHAPES])
def test_streams_inflate_to_the_tiles(shape_name, content, dtype, predictor):
    _, shape, t = next(s for s in K.SHAPES if s[0] == shape_name)
    planes = K.content(content, shape, dtype, seed=len(shape_name))
    padded = shape[0] > 1
    total, raw, streams = check_exact(planes, t, t, predictor, padded)
    seg_per_tile = -(-t * t * np.dtype(dtype).itemsize // K.SEG)
    print(f'{shape_name} {content} {np.dtype(dtype).name} predictor {predictor}: {total} of {raw} bytes = {total / raw:.4f}')
    if content == 'zero':
        assert all(s == b'' for s in streams)
    if content == 'uniform':      # nothing to gain: stored blocks, inside the bound
        n_tiles = len(streams)
        assert total <= n_tiles * (t * t * np.dtype(dtype).itemsize + 6 + 5 * seg_per_tile)
        if t * t * np.dtype(dtype).itemsize >= 4096:
            assert total > raw
    if t >= 128:                  # tiles of whole segments: the header of a segment is small beside it
        if content == 'constant':
            assert total < raw / 16
        if content == 'cumsum' and np.dtype(dtype) == np.uint16 and predictor == 2:
            zr = 0
            for p in range(shape[0]):
                c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
                zr += len(c.compress(R.tile_bytes(planes[p], 0, 0, t, t, 2)) + c.flush())
            print(f'    zlib Z_RLE on the same bytes: {zr} = {zr / raw:.4f}; encoder / Z_RLE = {total / zr:.4f}')
            assert total < 0.80 * raw


@pytest.mark.parametrize('predictor', [1, 2])
@pytest.mark.parametrize('dtype', [np.uint8, np.uint16])
def test_runs_of_every_length(dtype, predictor):
    """1..300 elements, 258..261 among them, across segment boundaries, three planes with a padded pitch and plane stride."""
    planes = K.every_run_length(dtype)
    side = planes.shape[1]
    total, raw, _ = check_exact(planes, side, side, predictor, padded=True)
    if predictor == 1:
        assert total < raw / 8      # (runs of 150 elements on average: far below what literals alone can reach)


def test_code_length_limit_acts():
    """Fibonacci value counts: the unlimited code is deeper than 15 (tests/test_deflate_cpu.py), the stream has to be valid all the
    same -- and dynamic: the counts' entropy is 2.4 bits per byte, a stored block would be 16389 bytes."""
    planes = K.fibonacci_segment()
    total, raw, _ = check_exact(planes, 128, 128, 1)
    assert total < raw / 2


def test_too_small_a_capacity_sets_status_and_writes_nothing():
    import torch
    planes = K.content('uniform', (1, 144, 144), np.uint16, seed=5)
    dev = device_planes(planes, False)
    buf = native.DeflateBuffers(1, 144, 144, np.uint16, 144, 144, _dev())
    buf.out.fill_(0xAB)
    capacity = 1000
    L = native.lib()
    rc = L.sq_deflate_encode_planes(dev.data_ptr(), 144 * 144, 144, 1, 144, 144, native.SQ_U16, 144, 144, 2, buf.scratch.data_ptr(),
                                    buf.scratch.numel(), buf.offsets.data_ptr(), buf.out.data_ptr(), capacity, buf.status.data_ptr(),
                                    native._stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert int(buf.status.item()) != 0
    assert bool((buf.out == 0xAB).all()), 'bytes were written although the capacity was too small'
    assert int(buf.offsets[-1].item()) > capacity      # the size that would have been needed


def test_two_config_3_planes_offsets_past_2_31():
    """Two planes of 36 428 x 29 108 uint16 in 512 x 512 tiles: 262 656 segments, so the second plane and its segments' slots lie past
    2^31 bytes, and so do the packed streams of its lower half; sampled tiles of it, the last one among them, inflate to what the
    plane holds."""
    import torch
    h, w, t = 36428, 29108, 512
    planes = torch.empty((2, h, w), dtype=torch.uint16, device=_dev())
    planes.view(torch.int16).random_(0, 3000)
    planes[:, :t, :t] = 0
    buf = native.deflate_encode_planes(planes, t, t, 2)
    torch.cuda.synchronize()
    assert int(buf.status.item()) == 0
    off = buf.offsets.cpu().numpy()
    gy, gx = -(-h // t), -(-w // t)
    per = gy * gx
    assert len(off) == 2 * per + 1 and off[per + per // 2] > 2 ** 31 and np.all(np.diff(off) >= 0)
    assert off[1] == 0 and off[per + 1] == off[per]      # the first tile of either plane is zero
    for i in [1, gx + 3, per // 2, (gy - 1) * gx - 1, per - gx, per - 1]:
        iy, ix = divmod(i, gx)
        tile = np.zeros((t, t), np.uint16)
        part = planes[1, iy * t:(iy + 1) * t, ix * t:(ix + 1) * t].cpu().numpy()
        tile[:part.shape[0], :part.shape[1]] = part
        s = buf.out[int(off[per + i]):int(off[per + i + 1])].cpu().numpy().tobytes()
        assert zlib.decompress(s) == R.predict(tile, 2).tobytes(), f'tile {i} of plane 1'


def test_float32_and_bad_arguments_are_refused():
    import torch
    with pytest.raises(native.NativeError) as e:
        native.deflate_encode_planes(torch.zeros((1, 32, 32), dtype=torch.float32, device=_dev()), 16, 16)
    assert e.value.status == native.SQ_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        native.deflate_encode_planes(torch.zeros((1, 32, 32), dtype=torch.uint16, device=_dev()), 16, 16, predictor=3)
    assert native.lib().sq_deflate_out_bound(1, 32, 32, native.SQ_F32, 16, 16) == native.SQ_ERR_UNSUPPORTED


def test_buffers_are_reused_for_the_same_geometry():
    import torch
    a = K.content('cumsum', (1, 40, 72), np.uint16, seed=1)
    b = K.content('runs', (1, 40, 72), np.uint16)
    buf = native.deflate_encode_planes(torch.from_numpy(a).to(_dev()), 16, 16, 2)
    again = native.deflate_encode_planes(torch.from_numpy(b).to(_dev()), 16, 16, 2, buffers=buf)
    torch.cuda.synchronize()
    assert again is buf
    off, out = buf.offsets.cpu().numpy(), buf.out.cpu().numpy()
    for i, w in enumerate(R.expected_tiles(b, 16, 16, 2)):
        assert zlib.decompress(out[off[i]:off[i + 1]].tobytes()) == w


# ---------------------------------------------------------------------------------------------------- off the default stream
DH, DW, DT = 100, 130, 64


def _planes(seed):
    return {'planes': K.content('cumsum', (2, DH, DW), np.uint16, seed=seed)}


def _call(ctx, inp, out, stream):
    buf = native.deflate_encode_planes(inp['planes'], DT, DT, 2, stream=stream)
    return {'offsets': buf.offsets, 'streams': buf.out, 'status': buf.status}


def _finish(host):
    off, data = host['offsets'], host['streams']
    assert int(host['status'][0]) == 0, f"the encoder's status word is {host['status']}"
    tiles = np.zeros((len(off) - 1, DT * DT), np.uint16)
    for i in range(len(off) - 1):
        s = data[off[i]:off[i + 1]].tobytes()
        if s:
            try:
                tiles[i] = np.frombuffer(zlib.decompress(s), '<u2')
            except (zlib.error, ValueError):
                tiles[i] = 0xDEAD        # (a stream cut short by a race: reported as a mismatch, not as an exception)
    return {'tiles': tiles}


def _reference(a, strict):
    return {'tiles': np.stack([np.frombuffer(w, '<u2') if w else np.zeros(DT * DT, np.uint16)
                               for w in R.expected_tiles(a['planes'], DT, DT, 2)])}


STREAM_CASE = SC.Case('deflate-encode-planes', _planes(200), _planes(210), {}, _call, _reference, finish=_finish)


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
