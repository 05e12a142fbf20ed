"""Device chunk encoder (csrc/blosc.hip) at the LZ4 format's edges and at scale.  The inputs and what each one has to
produce come from tests/blosc_cases.py (no device there, checked by tests/test_blosc_cpu.py).  Every frame is decoded by
the independent reader (tests/blosc_ref.py) and by the store's reader (omezarr.blosc_decode), and every LZ4 stream in it
has to pass blosc_ref.lz4_sequences, which holds a block to the rules of liblz4's safe decoder: a stream our lenient
readers accept and liblz4 refuses is a store zarr cannot open."""
import functools
import struct

import numpy as np
import pytest

import blosc_cases as K
import blosc_ref
from image_stitcher_amd import native, omezarr, synth

pytestmark = pytest.mark.gpu
BLK = K.BLK


def _dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def encode(planes_np, cy, cx):
    """-> the frame of every chunk (b'' for an all-zero one), and the offsets."""
    import torch
    buf = native.blosc_encode_planes(torch.from_numpy(planes_np).to(_dev()), cy, cx)
    torch.cuda.synchronize()
    assert int(buf.status.item()) == 0
    offsets, out = buf.offsets.cpu().numpy(), buf.out.cpu().numpy()
    assert offsets[0] == 0 and np.all(np.diff(offsets) >= 0) and offsets[-1] <= len(out)
    return [out[offsets[i]:offsets[i + 1]].tobytes() for i in range(len(offsets) - 1)], offsets


def check_frame(frame: bytes, want: bytes, esz: int):
    """The three checks every frame gets: both readers reproduce the chunk, and every compressed stream passes the strict
    parser (and decodes through it to the shuffled block).  -> [(raw_size, stored_raw, sequences | None)] per block."""
    hd = blosc_ref.parse_header(frame)
    assert (hd['version'], hd['versionlz'], hd['codec'], hd['typesize']) == (2, 1, 1, esz)
    assert hd['nbytes'] == len(want) and hd['cbytes'] == len(frame) and hd['blocksize'] == min(BLK, len(want))
    assert hd['dont_split'] and hd['shuffle'] == (esz > 1) and not hd['memcpyed']
    assert blosc_ref.blosc_decompress(frame) == want
    assert omezarr.blosc_decode(frame) == want
    lz4_input = K.shuffled(want, esz)
    blocks = []
    for b, raw_size, stored_raw, stream in blosc_ref.blosc_block_streams(frame):
        assert b == len(blocks) and raw_size == min(BLK, len(want) - b * BLK)
        seqs = None
        if not stored_raw:
            assert len(stream) < raw_size
            seqs = blosc_ref.lz4_sequences(stream, raw_size)
            assert blosc_ref.lz4_decode_strict(stream, raw_size) == lz4_input[b * BLK:b * BLK + raw_size]
        blocks.append((raw_size, stored_raw, seqs))
    assert len(blocks) == -(-len(want) // BLK)
    return blocks


def padded_chunk(plane, iy, ix, cy, cx):
    full = np.zeros((cy, cx), dtype=plane.dtype)
    part = plane[iy * cy:(iy + 1) * cy, ix * cx:(ix + 1) * cx]
    full[:part.shape[0], :part.shape[1]] = part
    return full


def check_plane(plane, cy, cx):
    """Encodes one plane and checks every chunk's frame.  -> {(iy, ix): blocks of check_frame, None for a zero chunk}."""
    frames, _ = encode(plane[None], cy, cx)
    ncy, ncx = -(-plane.shape[0] // cy), -(-plane.shape[1] // cx)
    assert len(frames) == ncy * ncx
    got = {}
    for iy in range(ncy):
        for ix in range(ncx):
            want = padded_chunk(plane, iy, ix, cy, cx)
            frame = frames[iy * ncx + ix]
            if not want.any():
                assert frame == b''
                got[iy, ix] = None
                continue
            got[iy, ix] = check_frame(frame, want.tobytes(), plane.dtype.itemsize)
    return got


# ---- planted literal-run and match lengths ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _mid_cases():
    return K.mid_cases()


@functools.lru_cache(maxsize=None)
def _end_cases():
    return K.end_cases()


def _planted_hits(cases, esz):
    """Encodes every seed of every target as one chunk of one plane; -> {(kind, target): hits of 8}.  Every block has to
    pass the three checks and be stored compressed whether or not its seed hits."""
    streams = [c for _, _, seeds in cases for c in seeds]
    planes, cy, cx = K.rows_plane([c['stream'] for c in streams], esz)
    frames, _ = encode(planes, cy, cx)
    assert len(frames) == len(streams)
    hits, at = {}, 0
    for kind, target, seeds in cases:
        n_hit = 0
        for c in seeds:
            ((raw_size, stored_raw, seqs),) = check_frame(frames[at], planes[0, at].tobytes(), esz)
            at += 1
            assert raw_size == c['n'] and not stored_raw, f'{kind} {target} seed {c["seed"]}: stored raw, the sequences are hidden'
            if kind == 'end':
                # whatever was found, nothing starts in the last 12 bytes, and a copy of fewer stays literal
                assert all(s[3] <= c['n'] - 12 for s in seqs[:-1])
                assert seqs[-1][0] >= (5 if target >= 12 else target)
                n_hit += seqs[1:] == c['sequences'][1:]
            else:
                n_hit += len(seqs) == 3 and seqs[1] == c['sequences'][1]
        hits[kind, target] = n_hit
    return hits


def _print_hits(hits, esz):
    for kind in dict.fromkeys(k for k, _ in hits):
        print(f'hits of {K.SEEDS}, element size {esz}, {kind}: ' + '  '.join(f'{t}:{h}' for (k, t), h in hits.items() if k == kind))
    print(f'minimum over the targets: {min(hits.values())} of {K.SEEDS}')


@pytest.mark.parametrize('esz', [1, 2])
def test_planted_literal_runs_and_match_lengths(esz):
    """A run of g literals and a match of m bytes planted in mid-block (blosc_cases.mid_stream): g at the 1-, 2- and
    3-byte boundaries of the length encoding (15, 270, 525), m at the same boundaries (19, 274, 529), at the minimum (4)
    and one and two 64-lane extension steps long (68, 132), each with its neighbours.  The second sequence of the stream
    has to be exactly (g, m) in at least one of 8 seeds (a hash slot overwritten by a later position may move a match)."""
    hits = _planted_hits(_mid_cases(), esz)
    _print_hits(hits, esz)
    assert [t for (k, t) in hits if k == 'lit'] == list(K.LIT_TARGETS) and [t for (k, t) in hits if k == 'match'] == list(K.MATCH_TARGETS)
    assert all(h >= 1 for h in hits.values()), hits


@pytest.mark.parametrize('esz', [1, 2])
def test_planted_copy_at_the_end_of_the_block(esz):
    """The block's last K bytes copy K earlier ones (blosc_cases.end_stream), K = 4..20 and 200.  From K = 12 on the last
    match starts at n - K (n - 12 is the last legal start), is K - 5 long (it ends at n - 5) and 5 literals follow; below,
    the K bytes stay literals.  Every K is seen exactly so in at least one of 8 seeds."""
    hits = _planted_hits(_end_cases(), esz)
    _print_hits(hits, esz)
    assert [t for (_, t) in hits] == list(K.END_K)
    assert all(h >= 1 for h in hits.values()), hits


# ---- block and chunk sizes -------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _size_cases():
    return K.size_cases()


def test_chunks_of_1_to_16_bytes_go_out_raw():
    for name, plane, cy, cx, last in _size_cases()[:16]:
        got = check_plane(plane, cy, cx)
        assert len(got) == 6 and got[2, 1] is None and sum(v is not None for v in got.values()) == 5, name
        for blocks in got.values():
            assert blocks is None or blocks == [(last, True, None)], name


@pytest.mark.parametrize('name', list(K.SIZE_LAST_BLOCKS))
def test_odd_block_lengths_and_short_last_blocks(name):
    """Blocks of odd length (1089, 16383) and last blocks of 1, 2, 12, 13 and 14 bytes behind compressible full blocks:
    compressed and raw blocks in one frame, in the real chunk and in the zero-padded edge chunk beside it."""
    (_, plane, cy, cx, last), = [c for c in _size_cases() if c[0] == name]
    got = check_plane(plane, cy, cx)
    assert set(got) == {(0, 0), (0, 1)}
    for blocks in got.values():
        assert blocks[-1][0] == last == K.SIZE_LAST_BLOCKS[name]
        assert all(not raw for size, raw, _ in blocks if size == BLK)             # the texture compresses
        assert all(raw for size, raw, _ in blocks if size <= 16)                  # 1 + n >= n
        if last > 1000:
            assert not blocks[-1][1]


# ---- structured fuzz -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('chunk_bytes', K.FUZZ_CHUNK_BYTES)
@pytest.mark.parametrize('esz', [1, 2])
def test_fuzz_of_literal_runs_and_copies(esz, chunk_bytes):
    planes, cy, cx, streams = K.fuzz_plane(esz, chunk_bytes)
    frames, _ = encode(planes, cy, cx)
    assert len(frames) == len(streams) == K.FUZZ_CHUNKS[chunk_bytes]
    n_raw = n_lz4 = 0
    for i, frame in enumerate(frames):
        assert K.shuffled(planes[0, i].tobytes(), esz) == streams[i].tobytes()
        if not streams[i].any():                                    # zeros copied from zeros: the chunk is dropped
            assert frame == b''
            continue
        blocks = check_frame(frame, planes[0, i].tobytes(), esz)
        n_raw += sum(raw for _, raw, _ in blocks)
        n_lz4 += sum(not raw for _, raw, _ in blocks)
    assert n_raw >= 10 and n_lz4 >= 10, (n_raw, n_lz4)             # both kinds of block in the call


# ---- the packing kernels past their first pass -----------------------------------------------------------------------

@pytest.mark.parametrize('count', list(K.CHUNK_GRIDS))
def test_chunk_counts_around_the_scan_width(count):
    """scan_kernel gives each of its 1024 threads (n + 1023) / 1024 consecutive sizes: 1023, 1024 and 1025 chunks sit
    around one per thread (1025: two per thread, the last threads idle), 2049 and 3249 take three and four.  A third of
    the chunks are all zero, so equal consecutive offsets pass through every part of the scan."""
    plane, zero = K.count_plane(count)
    frames, offsets = encode(plane[None], 8, 8)
    assert len(frames) == count
    want_len = np.where(zero, 0, 16 + 4 + 4 + 64)                   # 64 random bytes: header, one bstart, one raw block
    assert np.array_equal(np.array([len(f) for f in frames]), want_len)
    assert np.array_equal(offsets, np.concatenate([[0], np.cumsum(want_len)]))
    gx = K.CHUNK_GRIDS[count][1]
    for i, frame in enumerate(frames):
        want = padded_chunk(plane, i // gx, i % gx, 8, 8)
        assert want.any() != bool(zero[i])
        if not zero[i]:
            assert struct.unpack_from('<I', frame, 12)[0] == len(frame)
            assert check_frame(frame, want.tobytes(), 1) == [(64, True, None)]


@pytest.mark.parametrize('full', [False, True], ids=['plane-1000x2000', 'plane-1040x2064'])
def test_chunk_of_263_blocks(full):
    """One uint16 chunk of 1040 x 2064: 263 blocks, the last one 512 bytes -- past the 64 threads of chunk_size_kernel and
    the 256 of assemble_kernel's bstarts loop.  Under the 1000 x 2000 plane the chunk is edge-padded: the zero columns let
    even its random rows compress a little and the blocks from 253 on are all zero.  Under a plane that fills the chunk,
    raw and compressed blocks interleave up to the last block."""
    plane, cy, cx = K.chunk_263_plane(full)
    (frame,), offsets = encode(plane[None], cy, cx)
    want = padded_chunk(plane, 0, 0, cy, cx).tobytes()
    blocks = check_frame(frame, want, 2)
    assert len(blocks) == 263 and blocks[-1][0] == 512 and offsets[1] == len(frame)
    raw = np.array([r for _, r, _ in blocks])
    bstarts = np.frombuffer(frame, '<i4', 263, 16)
    cb = np.array([struct.unpack_from('<i', frame, int(at))[0] for at in bstarts])
    assert bstarts[0] == 16 + 4 * 263 and np.array_equal(np.diff(bstarts), 4 + cb[:-1]) and bstarts[-1] + 4 + cb[-1] == len(frame)
    assert np.array_equal(cb == np.array([s for s, _, _ in blocks]), raw)
    assert len(set(cb[:64])) > 8 and len(set(cb[64:253])) > 8                 # a sum over equal sizes would hide a lost term
    if full:
        for lo, hi in ((0, 64), (64, 256), (256, 263)):
            assert raw[lo:hi].any() and not raw[lo:hi].all(), (lo, hi)
    else:
        assert (cb[253:] < 200).all()                                         # rows 1000.. are padding


def test_chunk_of_exactly_32_mib():
    """4096 x 4096 uint16 in one chunk: 2048 blocks fill assemble_kernel's bstart array.  Zero but for four pixels, so
    block 0 is all zero in a frame that exists, one pixel lies in the last block and one has a zero low byte.  The
    blocks are long runs: each is decoded through the strict parser, the store's reader decodes the whole frame, and
    the lenient reader (one Python step per byte of a run of offset 1) the blocks that hold a pixel, the first and the last."""
    plane, cy, cx = K.chunk_32mib_plane()
    (frame,), offsets = encode(plane[None], cy, cx)
    want = plane.tobytes()
    hd = blosc_ref.parse_header(frame)
    assert (hd['nbytes'], hd['blocksize'], hd['cbytes'], hd['typesize']) == (32 << 20, BLK, len(frame), 2) and offsets[1] == len(frame)
    bstarts = np.frombuffer(frame, '<i4', 2048, 16)
    assert bstarts[0] == 16 + 4 * 2048 and np.all(np.diff(bstarts) > 0)
    lz4_input = K.shuffled(want, 2)
    streams = list(blosc_ref.blosc_block_streams(frame))
    assert [s[0] for s in streams] == list(range(2048))
    at = int(bstarts[0])
    with_pixel = {(y * 4096 + x) * 2 // BLK for (y, x) in K.BIG_PIXELS}
    assert 2047 in with_pixel and 0 not in with_pixel
    for b, raw_size, stored_raw, stream in streams:
        assert bstarts[b] == at and raw_size == BLK and not stored_raw and len(stream) < 200
        at += 4 + len(stream)
        block = lz4_input[b * BLK:(b + 1) * BLK]
        assert blosc_ref.lz4_decode_strict(stream, BLK) == block, b
        if b in with_pixel or b in (0, 1, 2046):
            assert blosc_ref.lz4_decompress_block(memoryview(stream), BLK) == block, b
    assert at == len(frame)
    assert omezarr.blosc_decode(frame) == want


# ---- capacity and refusals, through the C ABI ------------------------------------------------------------------------

class Call:
    """One geometry's device buffers and the raw sq_blosc_encode_planes call, every argument overridable."""

    def __init__(self, planes_np, cy, cx):
        import torch
        self.L = native.lib()
        self.planes = torch.from_numpy(planes_np).to(_dev())
        self.n, self.h, self.w = planes_np.shape
        self.dtype = native.sq_dtype_of(planes_np.dtype)
        self.cy, self.cx = cy, cx
        geo = (self.n, self.h, self.w, self.dtype, cy, cx)
        self.n_chunks = int(self.L.sq_blosc_chunk_count(self.n, self.h, self.w, cy, cx))
        self.bound, self.need = int(self.L.sq_blosc_out_bound(*geo)), int(self.L.sq_blosc_scratch_bytes(*geo))
        assert min(self.n_chunks, self.bound, self.need) > 0
        self.scratch = torch.empty(self.need + 512, dtype=torch.uint8, device=_dev())
        assert self.scratch.data_ptr() % 256 == 0
        self.offsets = torch.full((self.n_chunks + 1,), 77, dtype=torch.int64, device=_dev())
        self.out = torch.full((self.bound,), 0xA5, dtype=torch.uint8, device=_dev())      # always the worst case, whatever capacity says
        self.status = torch.full((1,), 9, dtype=torch.int32, device=_dev())

    def __call__(self, **over):
        import torch
        a = dict(planes=self.planes.data_ptr(), plane_stride=self.h * self.w, pitch=self.w, n=self.n, h=self.h, w=self.w, dtype=self.dtype,
                 cy=self.cy, cx=self.cx, scratch=self.scratch.data_ptr(), scratch_bytes=self.need, offsets=self.offsets.data_ptr(),
                 out=self.out.data_ptr(), capacity=self.bound, status=self.status.data_ptr())
        assert set(over) <= set(a)
        a.update(over)
        assert a['capacity'] <= self.bound
        rc = self.L.sq_blosc_encode_planes(*a.values(), native._stream_ptr())
        torch.cuda.synchronize()
        return rc, self.L.sq_last_error().decode()


def test_output_capacity_exact_and_one_byte_short():
    """The "output too small" path: with out_capacity == total the call writes the very same bytes; one byte less and it
    returns success (the shortfall is only known on the device), sets *status, still reports the total in
    offsets[n_chunks], and writes nothing into out."""
    planes = np.stack([synth.scene_patch(7 + p, 50, 60, 100, 130) for p in range(2)]).astype(np.uint16)
    planes[1, :64, :64] = 0                                         # a zero chunk in the middle of the offsets
    call = Call(planes, 64, 64)
    assert call()[0] == 0 and int(call.status.item()) == 0
    offsets = call.offsets.cpu().numpy().copy()
    total = int(offsets[-1])
    assert 0 < total < call.bound and len(offsets) == 2 * 2 * 3 + 1 and offsets[6] == offsets[7]
    first = call.out.cpu().numpy().copy()
    assert (first[total:] == 0xA5).all()
    for i in range(call.n_chunks):
        if offsets[i + 1] > offsets[i]:
            check_frame(first[offsets[i]:offsets[i + 1]].tobytes(), padded_chunk(planes[i // 6], i % 6 // 3, i % 3, 64, 64).tobytes(), 2)
    call.out.fill_(0xA5)
    assert call(capacity=total)[0] == 0 and int(call.status.item()) == 0
    assert np.array_equal(call.offsets.cpu().numpy(), offsets) and np.array_equal(call.out.cpu().numpy(), first)
    call.out.fill_(0xA5)
    call.offsets.fill_(77)
    assert call(capacity=total - 1)[0] == 0
    assert int(call.status.item()) == 1
    assert np.array_equal(call.offsets.cpu().numpy(), offsets)       # the sizes are still reported: the caller can retry
    assert bool((call.out == 0xA5).all())
    assert call()[0] == 0 and int(call.status.item()) == 0           # status is cleared by the next call
    assert np.array_equal(call.out.cpu().numpy(), first)


def test_host_refusals_and_their_messages():
    planes = np.full((2, 20, 30), 5, np.uint8)
    call = Call(planes, 16, 16)
    E = native
    refused = [
        (dict(pitch=29), E.SQ_ERR_INVALID, 'pitch / plane stride smaller than the plane'),
        (dict(plane_stride=19 * 30 + 29), E.SQ_ERR_INVALID, 'pitch / plane stride smaller than the plane'),
        (dict(scratch_bytes=call.need - 1), E.SQ_ERR_WORKSPACE, f'scratch {call.need - 1} < {call.need} bytes'),
        (dict(scratch=call.scratch.data_ptr() + 1), E.SQ_ERR_INVALID, 'scratch must be 256-byte, offsets 8-byte aligned'),
        (dict(scratch=call.scratch.data_ptr() + 128), E.SQ_ERR_INVALID, 'scratch must be 256-byte'),
        (dict(offsets=call.offsets.data_ptr() + 4), E.SQ_ERR_INVALID, 'offsets 8-byte aligned'),
        (dict(dtype=E.SQ_F32), E.SQ_ERR_UNSUPPORTED, f'dtype {E.SQ_F32} (uint8 / uint16 planes)'),
        (dict(dtype=E.SQ_U16, cy=1, cx=(16 << 20) + 1), E.SQ_ERR_UNSUPPORTED, f'chunks of {(32 << 20) + 2} bytes (at most 32 MiB)'),
        (dict(cy=0), E.SQ_ERR_INVALID, 'bad sizes'), (dict(n=-1), E.SQ_ERR_INVALID, 'bad sizes'), (dict(h=0), E.SQ_ERR_INVALID, 'bad sizes'),
        (dict(out=None), E.SQ_ERR_INVALID, 'NULL argument'), (dict(status=None), E.SQ_ERR_INVALID, 'NULL argument'),
    ]
    for over, code, message in refused:
        rc, text = call(**over)
        assert rc == code and message in text and text.startswith('sq_blosc'), (over, rc, text)
        assert int(call.status.item()) == 9 and bool((call.offsets == 77).all()) and bool((call.out == 0xA5).all()), over   # nothing ran
    # the nearest accepted neighbours: the exact plane stride, and any plane stride at all for a single plane
    assert call()[0] == 0 and int(call.status.item()) == 0
    want = call.out.cpu().numpy().copy()
    offsets = call.offsets.cpu().numpy().copy()
    assert offsets[-1] > 0
    assert call(plane_stride=19 * 30 + 30)[0] == 0 and np.array_equal(call.out.cpu().numpy(), want)
    assert call(n=1, plane_stride=0)[0] == 0 and np.array_equal(call.offsets.cpu().numpy()[:5], offsets[:5])
    # no planes: one offset, zero, and success
    call.offsets.fill_(77)
    assert call(n=0)[0] == 0
    assert call.offsets.cpu().numpy().tolist() == [0] + [77] * call.n_chunks


def test_size_queries_and_the_encode_call_accept_the_same_geometries():
    """sq_blosc_out_bound, sq_blosc_scratch_bytes and sq_blosc_encode_planes refuse the same (geometry, dtype) with the same
    code; sq_blosc_chunk_count, which is not told the dtype, refuses exactly what every dtype is refused."""
    call = Call(np.full((1, 8, 8), 3, np.uint8), 8, 8)
    L, E = call.L, native
    geometries = [(1, 8, 8, 8, 8), (1, 8, 8, 4096, 4096), (1, 8, 8, 4096, 8192), (1, 8, 8, 4096, 8193), (1, 8, 8, 1, (32 << 20) + 1),
                  (1, 8, 8, 1, (16 << 20) + 1), (3, 5, 7, 2, 2), (0, 8, 8, 8, 8), (-1, 8, 8, 8, 8), (1, 0, 8, 8, 8), (1, 8, 0, 8, 8),
                  (1, 8, 8, 0, 8), (1, 8, 8, 8, 0)]
    seen = set()
    for n, h, w, cy, cx in geometries:
        codes = {}
        for dtype in (E.SQ_U8, E.SQ_U16, E.SQ_F32):
            bound, need = int(L.sq_blosc_out_bound(n, h, w, dtype, cy, cx)), int(L.sq_blosc_scratch_bytes(n, h, w, dtype, cy, cx))
            code = min(bound, 0)
            assert min(need, 0) == code and (code < 0 or (bound >= 0 and need >= 256)), (n, h, w, dtype, cy, cx)
            # the encode call with a scratch too small for anything: a geometry it accepts gets as far as the scratch check
            rc, text = call(n=n, h=h, w=w, dtype=dtype, cy=cy, cx=cx, plane_stride=h * w, pitch=max(w, 1), scratch_bytes=0)
            assert rc == (code if code < 0 else E.SQ_ERR_WORKSPACE), (n, h, w, dtype, cy, cx, rc, text)
            codes[dtype] = code
        count = int(L.sq_blosc_chunk_count(n, h, w, cy, cx))
        assert (count < 0) == (codes[E.SQ_U8] < 0 and codes[E.SQ_U16] < 0), (n, h, w, cy, cx, count, codes)
        if count >= 0:
            assert count == max(n, 0) * -(-h // cy) * -(-w // cx)
        seen.add((codes[E.SQ_U8], codes[E.SQ_U16], codes[E.SQ_F32], min(count, 0)))
    U, I = E.SQ_ERR_UNSUPPORTED, E.SQ_ERR_INVALID
    assert seen == {(0, 0, U, 0), (0, U, U, 0), (U, U, U, U), (I, I, I, I)}


def test_uint8_chunk_of_32_mib_through_the_wrapper():
    """4096 x 8192 uint8 is a legal 32 MiB chunk: the wrapper's size queries accept it and the frame has 2048 blocks."""
    plane = np.zeros((8, 8), np.uint8)
    plane[3, 5] = 200
    (frame,), _ = encode(plane[None], 4096, 8192)
    hd = blosc_ref.parse_header(frame)
    assert (hd['nbytes'], hd['blocksize'], hd['cbytes'], hd['typesize'], hd['shuffle']) == (32 << 20, BLK, len(frame), 1, False)
    bstarts = np.frombuffer(frame, '<i4', 2048, 16)
    assert bstarts[0] == 16 + 4 * 2048 and np.all(np.diff(bstarts) > 0)
    for b, raw_size, stored_raw, stream in blosc_ref.blosc_block_streams(frame):
        assert raw_size == BLK and not stored_raw
        block = blosc_ref.lz4_decode_strict(stream, BLK)
        if b == 1:                                                          # pixel (3, 5) is byte 3 * 8192 + 5 of the chunk
            assert block[24581 - BLK] == 200 and block.count(0) == BLK - 1
        else:
            assert block == bytes(BLK), b
