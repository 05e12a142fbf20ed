"""The two Blosc-1 / LZ4 readers (the store reader in omezarr.py and the independent one in tests/blosc_ref.py) on frames
built here by hand from the format documents: known LZ4 vectors, split and unsplit blocks, shuffle, memcpy'd frames."""
import struct

import numpy as np
import pytest

import blosc_ref
from image_stitcher_amd import omezarr


def lz4_greedy(data: bytes) -> bytes:
    """A plain greedy LZ4 block encoder (reference for the tests; quadratic search, tiny inputs only)."""
    n, out, anchor, i = len(data), bytearray(), 0, 0

    def emit(lit, off=None, ml=0):
        token = (min(len(lit), 15) << 4) | (min(ml - 4, 15) if off else 0)
        out.append(token)
        if len(lit) >= 15:
            r = len(lit) - 15
            out.extend([255] * (r // 255) + [r % 255])
        out.extend(lit)
        if off:
            out.extend(struct.pack('<H', off))
            if ml - 4 >= 15:
                r = ml - 4 - 15
                out.extend([255] * (r // 255) + [r % 255])

    while i <= n - 12:
        best = None
        for j in range(max(0, i - 300), i):
            if data[j:j + 4] == data[i:i + 4]:
                best = j
        if best is None:
            i += 1
            continue
        ml = 4
        while i + ml < n - 5 and data[best + ml] == data[i + ml]:
            ml += 1
        emit(data[anchor:i], i - best, ml)
        i += ml
        anchor = i
    emit(data[anchor:])
    return bytes(out)


def frame(raw: bytes, typesize: int, blocksize: int, shuffle: bool, dont_split: bool) -> bytes:
    nblocks = -(-len(raw) // blocksize)
    body, bstarts = bytearray(), []
    for b in range(nblocks):
        blk = raw[b * blocksize:(b + 1) * blocksize]
        if shuffle and typesize > 1:
            nel = len(blk) // typesize
            blk = np.frombuffer(blk, np.uint8, nel * typesize).reshape(nel, typesize).T.tobytes() + blk[nel * typesize:]
        split = (not dont_split) and blocksize // typesize >= 128 and len(blk) == blocksize
        bstarts.append(16 + 4 * nblocks + len(body))
        ns = typesize if split else 1
        for k in range(ns):
            part = blk[k * len(blk) // ns:(k + 1) * len(blk) // ns]
            c = lz4_greedy(part)
            if len(c) >= len(part):
                c = part
            body += struct.pack('<i', len(c)) + c
    flags = (1 if shuffle and typesize > 1 else 0) | (0x10 if dont_split else 0) | (1 << 5)
    total = 16 + 4 * nblocks + len(body)
    return struct.pack('<BBBBIII', 2, 1, flags, typesize, len(raw), blocksize, total) + struct.pack(f'<{nblocks}i', *bstarts) + bytes(body)


def test_known_lz4_vector():
    # 20 x 'a': literal 'a', match offset 1 length 14, then the mandatory 5 trailing literals
    block = bytes([0x1A, ord('a'), 0x01, 0x00, 0x50]) + b'aaaaa'
    assert blosc_ref.lz4_decompress_block(memoryview(block), 20) == b'a' * 20
    assert bytes(omezarr._lz4_block(block, 20)) == b'a' * 20
    assert lz4_greedy(b'a' * 20) == block
    with pytest.raises(ValueError):
        blosc_ref.lz4_decompress_block(memoryview(block), 19)


@pytest.mark.parametrize('typesize', [1, 2])
@pytest.mark.parametrize('dont_split', [True, False])
def test_both_readers_on_hand_built_frames(typesize, dont_split):
    rng = np.random.default_rng(typesize * 2 + dont_split)
    smooth = (np.arange(1500) // 7 % 251).astype(np.uint16 if typesize == 2 else np.uint8)
    noisy = rng.integers(0, 1 << (8 * typesize), 700).astype(smooth.dtype)
    raw = np.concatenate([smooth, noisy, np.zeros(600, smooth.dtype), smooth[:123]]).tobytes()
    for blocksize in (512, 1024, len(raw)):
        f = frame(raw, typesize, blocksize, shuffle=True, dont_split=dont_split)
        assert blosc_ref.blosc_decompress(f) == raw and omezarr.blosc_decode(f) == raw
        h = blosc_ref.parse_header(f)
        assert (h['nbytes'], h['cbytes'], h['typesize'], h['codec'], h['dont_split']) == (len(raw), len(f), typesize, 1, dont_split)
    # memcpy'd frame
    f = struct.pack('<BBBBIII', 2, 1, 0x02, typesize, len(raw), len(raw), 16 + len(raw)) + raw
    assert blosc_ref.blosc_decompress(f) == raw and omezarr.blosc_decode(f) == raw
    with pytest.raises(ValueError):
        blosc_ref.blosc_decompress(f[:-1])


def test_host_chunk_writers_refuse_codecs_they_do_not_implement(tmp_path):
    """emit_chunk / write_plane_levels used to fall through to zlib for anything that was not 'none' --
    'blosc' (the Stitcher default, encoded on the DEVICE) then left zlib bytes under a .zarray that says blosc."""
    from image_stitcher_amd import omezarr
    plane = np.arange(64 * 64, dtype=np.uint16).reshape(1, 64, 64)
    for bad in ('blosc', 'lz4', 'zstd'):
        with pytest.raises(ValueError, match='device encoder'):
            omezarr.write_plane_levels(str(tmp_path / 's'), [plane], [(0, 0, 0)], (1, 1, 1, 32, 32), compression=bad)
        with pytest.raises(ValueError, match='device encoder'):
            omezarr.emit_chunk(str(tmp_path / 's'), (0, 0, 0, 0, 0, 0, plane[0], 0, 0, 32, 32), bad)
    assert not (tmp_path / 's').exists()
    for ok in ('zlib', 'none', None):
        assert omezarr.write_plane_levels(str(tmp_path / f's_{ok}'), [plane], [(0, 0, 0)], (1, 1, 1, 32, 32), compression=ok) > 0


def test_both_readers_decode_genuine_c_blosc_frames():
    """frames produced by the GENUINE c-blosc 1.21.0 (imagecodecs 2021.8.26 under the authoring
    container's /opt/conda/bin/python3.9; tests/golden/make_blosc_golden.py cblosc) -- LZ4 with and without byte
    shuffle, levels 1 / 5 / 9, typesize 1 / 2, split streams, an incompressible (memcpy'd) chunk, a 42-byte chunk --
    decode to the seeded raw chunk with BOTH readers of this repo.  That pins the readers the device encoder's tests
    lean on to third-party output."""
    import json
    import os
    import sys
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
    sys.path.insert(0, golden)
    import make_blosc_golden as G
    with open(os.path.join(golden, 'blosc_cblosc_frames.json')) as fh:
        index = json.load(fh)
    assert index['encoder'] == 'c-blosc 1.21.0'
    frames = np.load(os.path.join(golden, 'blosc_cblosc_frames.npz'))
    seen_flags = set()
    for e in index['frames']:
        frame = frames[e['name']].tobytes()
        raw = G.chunk(e['kind'], e['h'], e['w'], e['dtype'], e['seed']).tobytes()
        assert G.sha(raw) == e['raw_sha256'] and len(frame) == e['cbytes']       # the seeded chunk is the one c-blosc saw
        hd = blosc_ref.parse_header(frame)
        assert hd['nbytes'] == len(raw) and hd['cbytes'] == len(frame) and hd['typesize'] == np.dtype(e['dtype']).itemsize
        assert blosc_ref.blosc_decompress(frame) == raw, e['name']
        assert omezarr.blosc_decode(frame) == raw, e['name']
        seen_flags.add(e['flags'])
    assert {0x21, 0x20, 0x23} <= seen_flags          # shuffled, unshuffled, memcpy'd -- split (no 0x10) streams throughout
    assert len(index['frames']) >= 15


# ---- the strict parser (blosc_ref.lz4_sequences): what liblz4's safe decoder asks for beyond a decodable stream ---------

def lz4_from_sequences(stream, sequences) -> bytes:
    """The LZ4 block that says `sequences` ([(literals, match_len | None, offset | None, out_pos)]) about `stream`."""
    stream, out, at = bytes(stream), bytearray(), 0

    def length(x):
        return bytes([255] * ((x - 15) // 255) + [(x - 15) % 255]) if x >= 15 else b''

    for lit, ml, off, out_pos in sequences:
        out.append((min(lit, 15) << 4) | (min(ml - 4, 15) if ml is not None else 0))
        out += length(lit) + stream[at:at + lit]
        at += lit
        assert at == out_pos
        if ml is not None:
            out += struct.pack('<H', off) + length(ml - 4)
            at += ml
    return bytes(out)


A20 = b'a' * 20
KNOWN = bytes([0x1A, ord('a'), 0x01, 0x00, 0x50]) + b'aaaaa'           # 20 x 'a': 1 literal, match of 14 at offset 1, 5 literals

# (rule, violating block, its nearest legal neighbour, whether the lenient decoder takes the violating one) -- all of 20 x 'a'
STRICT_RULES = [
    ('match starts after n - 12',
     lz4_from_sequences(A20, [(9, 6, 1, 9), (5, None, None, 20)]), lz4_from_sequences(A20, [(8, 7, 1, 8), (5, None, None, 20)]), True),
    ('match ends after n - 5',
     lz4_from_sequences(A20, [(1, 15, 1, 1), (4, None, None, 20)]), KNOWN, True),
    ('last token announces a match',
     KNOWN[:4] + bytes([0x53]) + KNOWN[5:], KNOWN, True),
    ('offset 0', bytes([0x1A, ord('a'), 0x00, 0x00, 0x50]) + b'aaaaa', KNOWN, False),
    ('offset past the start of the output', bytes([0x1A, ord('a'), 0x02, 0x00, 0x50]) + b'aaaaa', KNOWN, False),
    ('block ends with a match', bytes([0x1F, ord('a'), 0x01, 0x00, 0x00]), KNOWN, False),
    ('input goes on after the last literals', KNOWN + b'\x01\x00\x00', KNOWN, False),
    ('input ends inside the last literals', KNOWN[:-1], KNOWN, False),
    ('input ends inside a length', bytes([0xF0, 255]), bytes([0xF0, 5]) + A20, False),
]


@pytest.mark.parametrize('rule', STRICT_RULES, ids=[r[0].replace(' ', '-') for r in STRICT_RULES])
def test_strict_parser_refuses_what_liblz4_refuses(rule):
    _, bad, good, lenient_takes_it = rule
    seqs = blosc_ref.lz4_sequences(good, 20)
    assert seqs[-1][1:] == (None, None, 20) and sum(s[0] + (s[1] or 0) for s in seqs) == 20
    assert blosc_ref.lz4_decode_strict(good, 20) == A20 == blosc_ref.lz4_decompress_block(memoryview(good), 20)
    with pytest.raises(ValueError, match='LZ4 strict'):
        blosc_ref.lz4_sequences(bad, 20)
    if lenient_takes_it:      # decodable, and to the right bytes: only the strict parser tells these from a good block
        assert blosc_ref.lz4_decompress_block(memoryview(bad), 20) == A20
        assert bytes(omezarr._lz4_block(bad, 20)) == A20


def test_strict_parser_on_the_known_vector_and_on_sizes():
    assert blosc_ref.lz4_sequences(KNOWN, 20) == [(1, 14, 1, 1), (5, None, None, 20)]
    for wrong in (19, 21):                                  # the output is exactly n bytes
        with pytest.raises(ValueError, match='LZ4 strict'):
            blosc_ref.lz4_sequences(KNOWN, wrong)
    assert blosc_ref.lz4_sequences(b'\x00', 0) == [(0, None, None, 0)]
    with pytest.raises(ValueError, match='LZ4 strict'):
        blosc_ref.lz4_sequences(b'', 0)
    # a match may start at n - 12 and end at n - 5 exactly; 12 bytes cannot hold one, 13 can
    assert blosc_ref.lz4_sequences(lz4_from_sequences(b'a' * 13, [(1, 7, 1, 1), (5, None, None, 13)]), 13)[0] == (1, 7, 1, 1)
    with pytest.raises(ValueError, match='LZ4 strict'):
        blosc_ref.lz4_sequences(lz4_from_sequences(b'a' * 12, [(1, 6, 1, 1), (5, None, None, 12)]), 12)
    # length bytes: 15 + 255 k takes a terminating zero byte
    for lit in (14, 15, 16, 269, 270, 271, 524, 525, 526):
        raw = bytes(range(1, 200)) * 3
        block = lz4_from_sequences(raw[:lit], [(lit, None, None, lit)])
        assert len(block) == 1 + lit + (0 if lit < 15 else (lit - 15) // 255 + 1)
        assert blosc_ref.lz4_sequences(block, lit) == [(lit, None, None, lit)]
        assert blosc_ref.lz4_decode_strict(block, lit) == raw[:lit]
    # overlapping copies of every small offset, laid down by doubling
    for off in (1, 2, 3, 7, 64):
        raw = (bytes(range(1, off + 1)) * 700)[:700]
        block = lz4_from_sequences(raw, [(off, 700 - 5 - off, off, off), (5, None, None, 700)])
        assert blosc_ref.lz4_decode_strict(block, 700) == raw == blosc_ref.lz4_decompress_block(memoryview(block), 700)


def test_genuine_c_blosc_streams_pass_the_strict_parser():
    """Every LZ4 stream c-blosc 1.21.0 wrote into tests/golden/blosc_cblosc_frames.npz obeys the rules of the strict
    parser (so the parser asks for nothing liblz4's own encoder does not do), and decodes through it to the bytes the
    lenient decoder gives."""
    import os
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
    frames = np.load(os.path.join(golden, 'blosc_cblosc_frames.npz'))
    n_streams, min_last, latest = 0, 1 << 30, 1 << 30
    for name in frames.files:
        for _, raw_size, stored_raw, stream in blosc_ref.blosc_block_streams(frames[name].tobytes()):
            if stored_raw:
                continue
            seqs = blosc_ref.lz4_sequences(stream, raw_size)
            assert blosc_ref.lz4_decode_strict(stream, raw_size) == blosc_ref.lz4_decompress_block(memoryview(stream), raw_size)
            n_streams += 1
            if len(seqs) > 1:
                min_last = min(min_last, seqs[-1][0])
                latest = min(latest, raw_size - seqs[-2][3])
    print(f'{n_streams} c-blosc streams pass; shortest last literal run {min_last}, latest match start n - {latest}')
    assert n_streams == 29 and min_last >= 5 and latest >= 12


@pytest.mark.parametrize('typesize', [1, 2])
@pytest.mark.parametrize('dont_split', [True, False])
def test_greedy_reference_encoder_passes_the_strict_parser(typesize, dont_split):
    rng = np.random.default_rng(typesize * 2 + dont_split)
    smooth = (np.arange(1500) // 7 % 251).astype(np.uint16 if typesize == 2 else np.uint8)
    noisy = rng.integers(0, 1 << (8 * typesize), 700).astype(smooth.dtype)
    raw = np.concatenate([smooth, noisy, np.zeros(600, smooth.dtype), smooth[:123]]).tobytes()
    compressed = 0
    for blocksize in (512, 1024, len(raw)):
        f = frame(raw, typesize, blocksize, shuffle=True, dont_split=dont_split)
        parts = []
        for _, raw_size, stored_raw, stream in blosc_ref.blosc_block_streams(f):
            parts.append(stream if stored_raw else blosc_ref.lz4_decode_strict(stream, raw_size))
            compressed += not stored_raw
        assert sum(len(p) for p in parts) == len(raw)
    assert compressed >= 6
    for n in range(13, 40):                                 # short blocks: the end-of-block rules decide everything
        data = (b'ab' * 20)[:n]
        assert blosc_ref.lz4_decode_strict(lz4_greedy(data), n) == data


# ---- the case tables of tests/test_blosc_edges_gpu.py: every input is what its builder says it is ----------------------

def test_planted_streams_are_what_their_builders_say():
    import blosc_cases as K
    cases = K.mid_cases() + K.end_cases()
    assert [t for k, t, _ in cases if k == 'lit'] == list(K.LIT_TARGETS) and [t for k, t, _ in cases if k == 'match'] == list(K.MATCH_TARGETS)
    assert [t for k, t, _ in cases if k == 'end'] == list(range(4, 21)) + [200]
    for kind, target, seeds in cases:
        assert len(seeds) == K.SEEDS == 8 and len({c['stream'].tobytes() for c in seeds}) == 8
        for c in seeds:
            s, n = c['stream'], c['n']
            assert len(s) == n == (K.END_L if kind == 'end' else K.MID_L) and s.min() >= 1 and n % 2 == 0
            # the planted sequences reproduce the stream, are legal LZ4, and are the ONLY matches there are
            assert K.apply_sequences(s, c['sequences']) == s.tobytes()
            block = lz4_from_sequences(s, c['sequences'])
            assert len(block) < n                                               # stored compressed, not raw
            assert blosc_ref.lz4_sequences(block, n) == c['sequences']
            assert blosc_ref.lz4_decode_strict(block, n) == s.tobytes() == blosc_ref.lz4_decompress_block(memoryview(block), n)
            if kind == 'end':
                k, c1, c3 = c['k'], c['copy1'], c['copy3']
                assert k == target and c3 == n - k and (s[c3:] == s[c['src3']:c['src3'] + k]).all()
                assert K.repeats(s) == set(range(c1, c1 + K.S1_LEN - 3)) | set(range(c3, c3 + k - 3))
                want = [(15, k - 5, c3 - c['src3'], n - k), (5, None, None, n)] if k >= 12 else [(15 + k, None, None, n)]
                assert c['sequences'][1:] == want
            else:
                g, m2, c1, c2 = c['g'], c['m2'], c['copy1'], c['copy2']
                assert (g, m2) == ((target, 19) if kind == 'lit' else (15, target))
                assert (s[c1:c1 + K.S1_LEN] == s[64:64 + K.S1_LEN]).all() and (s[c2:c2 + m2] == s[c['src2']:c['src2'] + m2]).all()
                assert s[c1 + K.S1_LEN] != s[64 + K.S1_LEN] and s[c2 + m2] != s[c['src2'] + m2] and c2 == c1 + K.S1_LEN + g
                assert K.repeats(s) == set(range(c1, c1 + K.S1_LEN - 3)) | set(range(c2, c2 + m2 - 3))
                assert c['sequences'][1] == (g, m2, c2 - c['src2'], c2) and c['sequences'][2][0] >= 16


def test_uint16_pixels_shuffle_back_to_the_stream():
    import blosc_cases as K
    rng = np.random.default_rng(4)
    for n in (2, 14, 600, K.MID_L, K.BLK, K.BLK + 14, 3 * K.BLK + 1000):
        t = rng.integers(0, 256, n, dtype=np.uint8)
        px = K.pixels_of(t, 2)
        assert px.dtype == np.uint16 and px.size == n // 2
        assert K.shuffled(px.tobytes(), 2) == t.tobytes()
        nel = min(n, K.BLK) // 2
        assert int(px[0]) == int(t[0]) | (int(t[nel]) << 8)
        assert K.pixels_of(t, 1).tobytes() == t.tobytes() == K.shuffled(t.tobytes(), 1)
    planes, cy, cx = K.rows_plane([c['stream'] for c in K.mid_cases()[0][2]], 2)
    assert planes.shape == (1, 8, K.MID_L // 2) and (cy, cx) == (1, K.MID_L // 2)


def test_size_fuzz_and_packing_cases_are_what_they_say():
    import blosc_cases as K
    sizes = K.size_cases()
    assert [c[4] for c in sizes[:16]] == list(range(1, 17))
    for name, plane, cy, cx, last in sizes:
        cb = cy * cx * plane.dtype.itemsize
        assert plane.shape[0] == cy or cb <= 16
        assert last == cb - (cb - 1) // K.BLK * K.BLK and plane[:cy, :cx].all()
        if name in K.SIZE_LAST_BLOCKS:
            assert last == K.SIZE_LAST_BLOCKS[name]
    assert {c[0] for c in sizes} >= set(K.SIZE_LAST_BLOCKS)
    assert sorted(K.SIZE_LAST_BLOCKS.values()) == [1, 2, 12, 13, 14, 1089, 16383]
    # the fuzz: overlapping copies, edge lengths and all-random streams do occur; the planes carry the streams
    rng = np.random.default_rng(1)
    streams = [K.fuzz_stream(rng, 4096) for _ in range(64)]
    assert all(len(s) == 4096 for s in streams)
    n_rep = [len(K.repeats(s)) for s in streams]
    assert min(n_rep) == 0 and max(n_rep) > 2000
    for esz in (1, 2):
        planes, cy, cx, streams = K.fuzz_plane(esz, K.BLK + 14)
        assert planes.shape == (1, 200, (K.BLK + 14) // esz) and (cy, cx) == (1, (K.BLK + 14) // esz)
        assert K.shuffled(planes[0, 7].tobytes(), esz) == streams[7].tobytes()
    # chunk counts on both sides of the scan's 1024 threads and of two values per thread
    for count in (1023, 1024, 1025, 2049, 3249):
        plane, zero = K.count_plane(count)
        gy, gx = K.CHUNK_GRIDS[count]
        assert (-(-plane.shape[0] // 8), -(-plane.shape[1] // 8)) == (gy, gx) and len(zero) == count == gy * gx
        assert 0.25 < zero.mean() < 0.45
        runs = np.diff(np.flatnonzero(np.diff(np.concatenate([[0], zero.astype(int), [0]]))))[::2]
        assert runs.min() == 1 and runs.max() >= 7
        for i in (0, 1, count // 2, count - 1):
            y, x = divmod(i, gx)
            assert bool(plane[8 * y:8 * y + 8, 8 * x:8 * x + 8].any()) != bool(zero[i])
    plane, cy, cx = K.chunk_263_plane()
    assert plane.shape == (1000, 2000) and cy * cx * 2 == 262 * K.BLK + 512
    assert K.chunk_263_plane(True)[0].shape == (cy, cx) == (1040, 2064)
    plane, cy, cx = K.chunk_32mib_plane()
    assert cy * cx * 2 == 2048 * K.BLK == 32 << 20 and not plane[:2].any() and plane[4095, 4095] and plane[5, 17] == 256
    assert int(np.count_nonzero(plane)) == len(K.BIG_PIXELS) == 4
