"""Device tile encoder (csrc/deflate.hip) at deflate's edges.  tests/test_deflate_gpu.py holds every stream to "it inflates to its
tile"; a stream that is valid but worse -- fewer runs found, a code that is not minimum-redundancy, stored where dynamic would
shrink -- passes that.  Here every stream is also held to the LENGTH of the stream tests/deflate_ref.py makes of the same tile:
that length depends only on the rules both state (tie order among equal counts moves lengths between symbols of one count, not
their sum), so it is compared exactly.  Further: tiles whose segments are no multiple of a wave's 64-element round (the C ABI
takes any tile shape), tiles that mix stored and dynamic segments, the 15-bit limit on the uint16 path (two codes in one emit),
tiles of 128 and of the permitted 2048 segments, the capacity at its exact edge, reused buffers, and every refusal of
sq_deflate_encode_planes.  All comparisons are exact."""
import zlib

import numpy as np
import pytest

import deflate_cases as K
import deflate_ref as R
from deflate_device import _dev, check_sizes, check_streams, device_planes, encode, streams_of
from image_stitcher_amd import native

pytestmark = pytest.mark.gpu


def _both(planes, th, tw, predictor, padded=False, label=''):
    streams, _ = encode(planes, th, tw, predictor, padded)
    check_streams(streams, planes, th, tw, predictor)
    check_sizes(streams, planes, th, tw, predictor, label)
    return streams


# ---------------------------------------------------------------------------------------------------- sizes equal the reference's
@pytest.mark.parametrize('predictor', [1, 2])
@pytest.mark.parametrize('dtype', [np.uint8, np.uint16])
@pytest.mark.parametrize('content', K.CONTENTS)
@pytest.mark.parametrize('shape_name', [s[0] for s in K.SHAPES])
def test_stream_sizes_equal_the_references(shape_name, content, dtype, predictor):
    _, shape, t = next(s for s in K.SHAPES if s[0] == shape_name)
    planes = K.content(content, shape, dtype, seed=len(shape_name))
    _both(planes, t, t, predictor, shape[0] > 1, f'{shape_name} {content} {np.dtype(dtype).name} predictor {predictor}')


@pytest.mark.parametrize('predictor', [1, 2])
@pytest.mark.parametrize('dtype', [np.uint8, np.uint16])
def test_sizes_with_runs_of_every_length(dtype, predictor):
    """Runs of 1..300 elements across segment boundaries: one run missed, one piece cut elsewhere, and a size differs."""
    planes = K.every_run_length(dtype)
    side = planes.shape[1]
    _both(planes, side, side, predictor, True, f'every run length {np.dtype(dtype).name} predictor {predictor}')


def test_size_under_the_code_length_limit_uint8():
    _both(K.fibonacci_segment(), 128, 128, 1, label='fibonacci uint8')


def test_size_under_the_code_length_limit_uint16():
    """The uint16 path sends the two codes of an element in one emit: here both are of up to the limit's 15 bits.  The unlimited code
    is 16 deep (tests/test_deflate_cpu.py); the stream is dynamic all the same, and as long as the restated limit makes it."""
    planes = K.fibonacci_segment_u16()
    streams = _both(planes, 64, 128, 1, label='fibonacci uint16')
    assert len(streams) == 1 and len(streams[0]) < 64 * 128 * 2 / 2
    assert (streams[0][2] >> 1) & 3 == 2      # BTYPE 10


@pytest.mark.parametrize('predictor', [1, 2])
@pytest.mark.parametrize('dtype', [np.uint8, np.uint16])
def test_size_of_all_ones(dtype, predictor):
    """Every byte 0xFF, in 100 x 100 tiles of a 150 x 130 plane (edge tiles, a partial last round)."""
    _both(K.all_ones((1, 150, 130), dtype), 100, 100, predictor, label=f'all ones {np.dtype(dtype).name} predictor {predictor}')


# ---------------------------------------------------------------------------------------------------- mixed tiles
def _segment_starts(tile: bytes, esz: int):
    """Byte positions in a tile's stream of its segments' blocks (and of the checksum), from the restated rules."""
    at, out = 2, []
    for a in range(0, len(tile), R.SEG):
        seg, final = tile[a:a + R.SEG], a + R.SEG >= len(tile)
        out.append(at)
        blk = R.dynamic_block(seg, esz, final)
        at += len(blk) if len(blk) < len(seg) + 5 else len(seg) + 5
    return out + [at]


@pytest.mark.parametrize('predictor', [1, 2])
@pytest.mark.parametrize('dtype', [np.uint8, np.uint16])
def test_stored_and_dynamic_segments_in_one_tile(dtype, predictor):
    """A stored block behind a dynamic segment's sync flush, a final stored block after a dynamic one, a final dynamic one after a
    stored one: the block-type bits at every segment's start are the kinds the restated rule gives, a stored segment starts on a
    byte boundary with LEN / ~LEN, and every segment's bytes inflate on their own to that segment."""
    planes = K.mixed_segments(dtype)
    side, esz = planes.shape[1], planes.dtype.itemsize
    streams = _both(planes, side, side, predictor, label=f'mixed {planes.dtype.name} predictor {predictor}')
    for p, want_kinds in enumerate(K.MIXED_KINDS[planes.dtype.name]):
        tile = R.tile_bytes(planes[p], 0, 0, side, side, predictor)
        assert R.block_kinds(tile, esz) == want_kinds
        s = streams[p]
        starts = _segment_starts(tile, esz)
        assert starts[-1] + 4 == len(s)
        for k, kind in enumerate(want_kinds):
            at, final = starts[k], k == len(want_kinds) - 1
            seg = tile[k * R.SEG:(k + 1) * R.SEG]
            assert s[at] & 1 == (1 if final else 0), f'plane {p} segment {k}: BFINAL'
            assert (s[at] >> 1) & 3 == (0 if kind == 'S' else 2), f'plane {p} segment {k}: BTYPE of a {kind} segment'
            if kind == 'S':
                n = len(seg)
                assert s[at] == (1 if final else 0)
                assert s[at + 1:at + 5] == bytes([n & 0xFF, n >> 8, ~n & 0xFF, (~n >> 8) & 0xFF])
                assert s[at + 5:at + 5 + n] == seg
            elif not final:
                assert s[starts[k + 1] - 4:starts[k + 1]] == b'\x00\x00\xff\xff'      # the sync flush that ends it
            assert zlib.decompressobj(-15).decompress(s[at:starts[k + 1]]) == seg, f'plane {p} segment {k} on its own'


# ---------------------------------------------------------------------------------------------------- off-grid tiles
@pytest.mark.parametrize('predictor', [1, 2])
@pytest.mark.parametrize('padded', [False, True], ids=['dense', 'padded'])
@pytest.mark.parametrize('dtype', [np.uint8, np.uint16])
@pytest.mark.parametrize('name', [c[0] for c in K.OFF_GRID])
def test_tiles_that_are_no_multiple_of_a_round(name, dtype, padded, predictor):
    planes, th, tw = K.off_grid(name, dtype)
    _both(planes, th, tw, predictor, padded, f'{name} {np.dtype(dtype).name} {"padded" if padded else "dense"} predictor {predictor}')


# ---------------------------------------------------------------------------------------------------- many segments
def _big(content, side):
    if content == 'all-ones':
        return K.all_ones((1, side, side), np.uint16)
    return K.content('cumsum', (1, side, side), np.uint16, seed=side)


def _one_tile(planes, predictor):
    import torch
    side = planes.shape[1]
    buf = native.deflate_encode_planes(torch.from_numpy(planes).to(_dev()), side, side, predictor)
    torch.cuda.synchronize()
    assert int(buf.status.item()) == 0 and buf.n_chunks == 1
    off = buf.offsets.cpu().numpy()
    s = buf.out[:int(off[1])].cpu().numpy().tobytes()
    assert off[0] == 0 and 0 < len(s) <= buf.bound
    want = R.predict(planes[0], predictor).astype('<u2').tobytes()
    d = zlib.decompressobj()
    got = d.decompress(s)      # (checks the Adler-32 combined over all segments)
    assert d.eof and d.unused_data == b''
    assert got == want
    return len(s)


@pytest.mark.parametrize('predictor', [1, 2])
@pytest.mark.parametrize('content', ['all-ones', 'cumsum'])
def test_a_tile_of_128_segments(content, predictor):
    """More segments than tile_size_kernel has lanes; all bytes 0xFF: the largest Adler partial sums."""
    size = _one_tile(_big(content, 1024), predictor)
    print(f'1024 x 1024 uint16 {content} predictor {predictor}: {size} of {2 * 1024 * 1024} bytes')


@pytest.fixture(scope='module')
def cumsum_4096():
    return _big('cumsum', 4096)


def test_a_tile_of_2048_segments_all_ones():
    """The largest tile the encoder takes: 32 MiB, every one of deflate_assemble_kernel's 2048 segment starts in use."""
    assert native.lib().sq_deflate_out_bound(1, 4096, 4096, native.SQ_U16, 4096, 4096) == 2 + 4 + 5 * 2048 + 2 * 4096 * 4096
    size = _one_tile(_big('all-ones', 4096), 1)
    assert size < 2 * 4096 * 4096 / 16      # runs of 0xFFFF


def test_a_tile_of_2048_segments_cumsum(cumsum_4096):
    size = _one_tile(cumsum_4096, 2)
    assert size < 0.80 * 2 * 4096 * 4096      # (the bound of tests/test_deflate_gpu.py for these planes: a dynamic code)


def test_the_4096_plane_in_512_tiles(cumsum_4096):
    import torch
    t = 512
    buf = native.deflate_encode_planes(torch.from_numpy(cumsum_4096).to(_dev()), t, t, 2)
    torch.cuda.synchronize()
    assert int(buf.status.item()) == 0
    streams = streams_of(buf)
    assert len(streams) == 64
    got = np.empty((4096, 4096), np.uint16)
    for i, s in enumerate(streams):
        iy, ix = divmod(i, 8)
        tile = np.frombuffer(zlib.decompress(s), '<u2').reshape(t, t)
        got[iy * t:(iy + 1) * t, ix * t:(ix + 1) * t] = R.unpredict(tile, 2)
    assert np.array_equal(got, cumsum_4096[0])


# ---------------------------------------------------------------------------------------------------- through the C ABI
SQ_OK = 0
OUT_CANARY, OFF_CANARY, STATUS_CANARY = 0xAB, 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A


class Call:
    """One geometry's buffers with canaries, and sq_deflate_encode_planes called on them with single arguments replaced."""

    def __init__(self, planes_np, th, tw, predictor=2, extra_scratch=0):
        import torch
        self.planes_np, self.th, self.tw = planes_np, th, tw
        n, h, w = planes_np.shape
        self.dev = device_planes(planes_np, False)
        self.buf = native.DeflateBuffers(n, h, w, planes_np.dtype, th, tw, _dev())
        L = native.lib()
        self.need = int(L.sq_deflate_scratch_bytes(*self.buf.geometry))
        if extra_scratch:
            self.buf.scratch = torch.empty(self.need + extra_scratch, dtype=torch.uint8, device=_dev())
        self.args = dict(planes=self.dev.data_ptr(), plane_stride=h * w, pitch=w, n_planes=n, h=h, w=w,
                         dtype=native.sq_dtype_of(planes_np.dtype), tile_h=th, tile_w=tw, predictor=predictor,
                         scratch=self.buf.scratch.data_ptr(), scratch_bytes=self.buf.scratch.numel(),
                         offsets=self.buf.offsets.data_ptr(), out=self.buf.out.data_ptr(), out_capacity=self.buf.out.numel(),
                         status=self.buf.status.data_ptr())
        assert self.args['scratch'] % 256 == 0 and self.args['offsets'] % 8 == 0
        self.reset()

    def reset(self):
        self.buf.out.fill_(OUT_CANARY)
        self.buf.offsets.fill_(OFF_CANARY)
        self.buf.status.fill_(STATUS_CANARY)

    def __call__(self, **changed):
        import torch
        a = dict(self.args, **changed)
        rc = native.lib().sq_deflate_encode_planes(*[a[k] for k in self.args], native._stream_ptr())
        torch.cuda.synchronize()
        return rc

    def untouched(self):
        return (bool((self.buf.out == OUT_CANARY).all()) and bool((self.buf.offsets == OFF_CANARY).all())
                and int(self.buf.status.item()) == STATUS_CANARY)


def test_capacity_exactly_enough_and_one_byte_short():
    planes = K.content('cumsum', (2, 50, 70), np.uint16, seed=9)
    streams, buf = encode(planes, 32, 32, 2)
    needed = int(buf.offsets[-1].item())
    assert 0 < needed < buf.bound
    call = Call(planes, 32, 32)
    assert call(out_capacity=needed) == SQ_OK
    assert int(call.buf.status.item()) == 0
    got = streams_of(call.buf)
    check_streams(got, planes, 32, 32, 2)
    assert got == streams
    assert bool((call.buf.out[needed:] == OUT_CANARY).all()), 'bytes were written past the capacity'
    call.reset()
    assert call(out_capacity=needed - 1) == SQ_OK
    assert int(call.buf.status.item()) != 0
    assert bool((call.buf.out == OUT_CANARY).all()), 'bytes were written although the capacity was one byte short'
    assert int(call.buf.offsets[-1].item()) == needed      # the size that would have been needed


def test_reused_buffers_hold_nothing_stale():
    """One DeflateBuffers, three stacks: after streams of every tile, a stack of zeros has no stream at all, and a stack with one
    pixel exactly one -- sizes, the tiles' any-flags and the status of the call before leave nothing behind."""
    import torch
    shape, t = (2, 40, 72), 16
    first = K.content('cumsum', shape, np.uint16, seed=2)
    buf = native.deflate_encode_planes(torch.from_numpy(first).to(_dev()), t, t, 2)
    torch.cuda.synchronize()
    check_streams(streams_of(buf), first, t, t, 2)
    zero = K.content('zero', shape, np.uint16)
    assert native.deflate_encode_planes(torch.from_numpy(zero).to(_dev()), t, t, 2, buffers=buf) is buf
    torch.cuda.synchronize()
    assert int(buf.status.item()) == 0 and not buf.offsets.cpu().numpy().any()
    pixel = K.content('one-pixel', shape, np.uint16)
    assert native.deflate_encode_planes(torch.from_numpy(pixel).to(_dev()), t, t, 2, buffers=buf) is buf
    torch.cuda.synchronize()
    streams = streams_of(buf)
    assert sum(1 for s in streams if s) == 1
    check_streams(streams, pixel, t, t, 2)
    check_sizes(streams, pixel, t, t, 2, 'one pixel behind a full and an empty stack')


def _refusals():
    I, W = native.SQ_ERR_INVALID, native.SQ_ERR_WORKSPACE
    return [('pitch-below-width', lambda c: dict(pitch=c.args['w'] - 1), I),
            ('plane-stride-too-small', lambda c: dict(plane_stride=(c.args['h'] - 1) * c.args['pitch'] + c.args['w'] - 1), I),
            ('planes-at-an-odd-address', lambda c: dict(planes=c.args['planes'] + 1), I),
            ('scratch-one-byte-short', lambda c: dict(scratch_bytes=c.need - 1), W),
            ('scratch-off-256', lambda c: dict(scratch=c.args['scratch'] + 128), I),
            ('offsets-off-8', lambda c: dict(offsets=c.args['offsets'] + 4), I),
            ('null-planes', lambda c: dict(planes=None), I), ('null-scratch', lambda c: dict(scratch=None), I),
            ('null-offsets', lambda c: dict(offsets=None), I), ('null-out', lambda c: dict(out=None), I),
            ('null-status', lambda c: dict(status=None), I),
            ('negative-capacity', lambda c: dict(out_capacity=-1), I),
            ('tile-height-zero', lambda c: dict(tile_h=0), I)]


@pytest.fixture(scope='module')
def refusal_call():
    # (two planes: the plane stride counts; 128 spare scratch bytes: the misaligned scratch is still large enough, so that the
    # alignment is what is refused)
    return Call(K.content('cumsum', (2, 40, 72), np.uint16, seed=3), 16, 16, extra_scratch=128)


@pytest.mark.parametrize('name', [r[0] for r in _refusals()])
def test_refusals_return_their_status_and_touch_nothing(refusal_call, name):
    _, change, want = next(r for r in _refusals() if r[0] == name)
    c = refusal_call
    c.reset()
    assert c(**change(c)) == want
    assert c.untouched(), 'a refused call wrote to out, offsets or status'


def test_the_call_is_accepted_without_the_changes(refusal_call):
    """The refusals above are refusals of the one changed argument: unchanged, the call encodes."""
    c = refusal_call
    c.reset()
    assert c() == SQ_OK
    assert int(c.buf.status.item()) == 0
    check_streams(streams_of(c.buf), c.planes_np, c.th, c.tw, 2)


def test_no_planes_is_an_empty_call(refusal_call):
    c = refusal_call
    c.reset()
    assert c(n_planes=0) == SQ_OK
    assert int(c.buf.offsets[0].item()) == 0 and int(c.buf.status.item()) == 0
    assert bool((c.buf.out == OUT_CANARY).all()) and bool((c.buf.offsets[1:] == OFF_CANARY).all())
