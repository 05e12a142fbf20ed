"""Device JPEG tile encoder (csrc/jpeg.hip) at the format's and at its own edges.  tests/test_jpeg_gpu.py runs four shapes; read
against the kernels, these never ran there: the 64-bit pixel load next to a partial block (and switched off by the pointer or by
the plane stride alone), jpeg_tile_kernel past its first round of 64 intervals, jpeg_scan_kernel with more than one tile per
thread, the interval kernel at exactly 64 and 65 blocks, the largest sides, byte stuffing at a group's last byte and before a
marker, every pad length, all 100 quantisation tables, the capacity at its exact edge, reused buffers, every refusal.  Every stream
is held BYTE FOR BYTE to ``jpegtile.encode_tile`` (tests/test_jpeg_cpu.py holds that to an independent decoder and a float64 DCT
on the same inputs); the streams of four cases are also decoded by tests/jpeg_ref.py and held to the float64 DCT directly, so
that a mistake shared by definition and kernel cannot pass.  Inputs and what each is there for: tests/jpeg_cases.py."""
import numpy as np
import pytest

import jpeg_cases as K
import jpeg_ref as R
from deflate_device import _dev, device_planes
from image_stitcher_amd import jpegtile as J
from image_stitcher_amd import native
from jpeg_device import check_equal, device_streams, first_difference, guarded_planes

pytestmark = pytest.mark.gpu

E_BOUND = R.transform_bound(J.DCT_MATRIX, J.DCT_SCALE_BITS)


def _report(label, streams, planes, th, tw):
    raw = len(streams) * th * tw
    total = sum(map(len, streams))
    print(f'{label}: {len(streams)} tiles ({sum(1 for s in streams if s)} with a stream), {total} device bytes, '
          f'{100.0 * total / raw:.1f} % of raw')


def _held_to_the_float_dct(streams, planes, th, tw, label):
    """The device's own bytes, decoded without jpegtile: every coefficient is the nearest multiple of its divisor (read from the
    stream's DQT) to the float64 DCT of the tile's pixels, up to the distance E between the integer and the float transform."""
    worst = -np.inf
    for tile, s in zip(K.tiles_of(planes, th, tw), streams):
        if not tile.any():
            assert s == b''
            continue
        d = R.decode(s)
        assert (d.height, d.width) == (th, tw)
        worst = max(worst, R.rounding_excess(d.coefficients, d.divisors, tile, E_BOUND))
    print(f'{label}: largest (|cQ - n| - Q/2) / E of the device streams = {worst:.4f}')
    assert worst < 1
    return worst


# ---------------------------------------------------------------------------------------------------- streams equal the definition
@pytest.mark.parametrize('shape_name', [s[0] for s in K.EDGE_SHAPES])
def test_streams_equal_the_host_definition(shape_name):
    _, shape, (th, tw), layout = K.edge_shape(shape_name)
    contents = dict(K.EDGE_CONTENTS)
    if shape_name in K.FULL_CONTENT_SHAPES:
        contents.update({name: K.QUALITIES for name in K.CONTENTS if name not in contents})
    for name, qualities in contents.items():
        for quality in qualities:
            planes = K.edge_content(name, shape_name, quality)
            if layout is not None:      # the buffer around the window is K.GUARD: the window must not look like it
                assert K.longest_guard_run(planes) < 3
            label = f'{shape_name} {name} q{quality}'
            streams = check_equal(planes, th, tw, quality, layout if layout is not None else False, label)
            _report(label, streams, planes, th, tw)
            if name == 'zero':
                assert all(s == b'' for s in streams)
            if name == 'pixel':
                assert sum(s != b'' for s in streams) == 1
            if shape_name == 'tiles2625' and name in ('uniform', 'binary'):
                sizes = np.array([len(s) for s in streams])
                assert not sizes[875:1750].any() and not sizes[175:350].any() and np.count_nonzero(sizes) == 2625 - 875 - 175
            if shape_name in ('mixed', 'round65', 'tall129') and (name, quality) in (('uniform', 100), ('binary', 1), ('ramp', 90)):
                _held_to_the_float_dct(streams, planes, th, tw, label)


@pytest.mark.parametrize('case', [c[0] for c in K.FFRUNS_SHAPES])
def test_ff_runs_and_an_ff_in_the_last_byte_of_a_group(case):
    """tests/test_jpeg_cpu.py holds this content to: two FF in a row, an FF in byte 3 of word 63 of a 64-word group of stuff_out,
    an FF in each byte of a word, rounds of more than two groups."""
    _, shape, (th, tw) = next(c for c in K.FFRUNS_SHAPES if c[0] == case)
    planes = K.content('ffruns', shape)
    streams = check_equal(planes, th, tw, 100, False, f'ffruns {case}')
    _report(f'ffruns {case} q100', streams, planes, th, tw)
    assert b'\xFF\x00\xFF\x00' in K.entropy_data(streams[0])


def test_the_dc_sweep_on_the_widest_tile():
    """Every DC numerator 362^2 (S - 8192) once, in order, through the reciprocal division: a rounding boundary crossed one block
    early or late moves a DC difference."""
    _, shape, (th, tw), _ = K.edge_shape('widest')
    planes = K.content('dcsweep', shape)
    for quality in K.DCSWEEP_QUALITIES:
        streams = check_equal(planes, th, tw, quality, False, f'widest dcsweep q{quality}')
        _report(f'widest dcsweep q{quality}', streams, planes, th, tw)


def test_every_quality_on_one_tile():
    """All 100 tables -- every divisor the quality rule can produce (251 values; tests/test_jpeg_cpu.py) under the reciprocal and
    its one correction step -- in one set of buffers; the device's bytes of every quality also decoded and held to the float64 DCT."""
    import torch
    planes = K.sweep_tile()
    n, h, w = planes.shape
    th, tw = h, w
    dev = torch.from_numpy(planes).to(_dev())
    worst_case = int(native.lib().sq_jpeg_out_bound(n, h, w, native.SQ_U8, th, tw))
    buf, worst, total = None, -np.inf, 0
    for quality in range(1, 101):
        again = native.jpeg_encode_planes(dev, th, tw, quality, buffers=buf, capacity=worst_case)
        torch.cuda.synchronize()
        assert buf is None or again is buf
        buf = again
        assert int(buf.status.item()) == 0
        (got,) = device_streams(buf)
        want = J.encode_tile(planes[0], quality)
        assert got == want, f'quality {quality}: {first_difference(got, want)}'
        d = R.decode(got)
        worst = max(worst, R.rounding_excess(d.coefficients, d.divisors, planes[0], E_BOUND))
        total += len(got)
    print(f'quality sweep: 100 streams, {total} device bytes, {total / (h * w):.1f} % of raw (100 x {h * w} bytes); '
          f'largest (|cQ - n| - Q/2) / E of the device streams = {worst:.4f}')
    assert worst < 1


def test_the_largest_tiles_end_their_intervals_every_way():
    """The device's stream of noise on the tallest tile: every pad length 0..7 and an FF as the last data byte before RSTm, read
    from the device's bytes by the independent decoder (which checks every marker, its number and the padding)."""
    _, shape, (th, tw), _ = K.edge_shape('tallest')
    planes = K.edge_content('uniform', 'tallest', 100)
    (s,) = check_equal(planes, th, tw, 100, False, 'tallest uniform q100')
    d = R.decode(s)
    assert set(d.pads) == set(range(8)) and any(data[-1] == 0xFF for data in d.intervals)
    assert len(d.pads) == th // 8 and s[2 + 69 + 5:2 + 69 + 9] == bytes((th >> 8, th & 255, 0, 8))


# ---------------------------------------------------------------------------------------------------- through the C ABI
SQ_OK = 0
OUT_FILL, STALE = 0x5A, 0xFF


class Call:
    """One geometry's buffers, filled with stale bytes, and sq_jpeg_encode_planes called on them with single arguments replaced."""

    def __init__(self, planes_np, th, tw, quality=100, extra_scratch=0):
        import torch
        self.planes_np, self.th, self.tw, self.quality = planes_np, th, tw, quality
        n, h, w = planes_np.shape
        self.dev = device_planes(planes_np, False)
        L = native.lib()
        self.worst = int(L.sq_jpeg_out_bound(n, h, w, native.SQ_U8, th, tw))
        self.buf = native.JpegBuffers(n, h, w, th, tw, _dev(), capacity=self.worst)
        self.need = int(L.sq_jpeg_scratch_bytes(*self.buf.geometry))
        if extra_scratch:
            self.buf.scratch = torch.empty(self.need + extra_scratch, dtype=torch.uint8, device=_dev())
        self.args = dict(planes=self.dev.data_ptr(), plane_stride=h * w, pitch=w, n_planes=n, h=h, w=w, dtype=native.SQ_U8,
                         tile_h=th, tile_w=tw, quality=quality, scratch=self.buf.scratch.data_ptr(),
                         scratch_bytes=self.buf.scratch.numel(), offsets=self.buf.offsets.data_ptr(), out=self.buf.out.data_ptr(),
                         out_capacity=self.buf.out.numel(), status=self.buf.status.data_ptr())
        assert self.args['scratch'] % 256 == 0 and self.args['offsets'] % 8 == 0
        self.fill()

    def fill(self, status=True):
        """Stale bytes everywhere a call reads or writes: 0xFF in scratch and offsets, 0x5A in out (and 0x5A5A5A5A in status)."""
        self.buf.scratch.fill_(STALE)
        self.buf.offsets.fill_(-1)
        self.buf.out.fill_(OUT_FILL)
        if status:
            self.buf.status.fill_(0x5A5A5A5A)
        self.before = self.snapshot()

    def snapshot(self):
        return [t.cpu().numpy().tobytes() for t in (self.buf.out, self.buf.offsets, self.buf.status, self.buf.scratch)]

    def __call__(self, **changed):
        import torch
        a = dict(self.args, **changed)
        rc = native.lib().sq_jpeg_encode_planes(*[a[k] for k in self.args], native._stream_ptr())
        torch.cuda.synchronize()
        return rc

    def want(self):
        return K.expected_streams(self.planes_np, self.th, self.tw, self.quality)


def test_capacity_exactly_enough_one_byte_short_and_none():
    """Stale bytes in scratch, offsets and out before every call.  Exactly sum(sizes): the host's streams and not a byte behind
    them; one byte less, and 0: the status set, out untouched in every byte, offsets[-1] the size needed; then enough room
    again, the status word of the call before still set when the call starts: it is cleared, not inherited."""
    planes = K.content('uniform', (1, 24, 40), seed=21)
    call = Call(planes, 16, 16)
    want = call.want()
    needed = sum(map(len, want))
    assert 16 * 16 * len(want) < needed < call.worst
    assert call(out_capacity=needed) == SQ_OK
    assert int(call.buf.status.item()) == 0 and device_streams(call.buf) == want
    assert bool((call.buf.out[needed:] == OUT_FILL).all()), 'bytes were written past the capacity'
    for capacity in (needed - 1, 0):
        call.fill()
        assert call(out_capacity=capacity) == SQ_OK
        assert int(call.buf.status.item()) != 0
        assert bool((call.buf.out == OUT_FILL).all()), f'bytes were written although the capacity was {capacity} of {needed}'
        assert int(call.buf.offsets[-1].item()) == needed
    call.fill(status=False)
    assert int(call.buf.status.item()) != 0
    assert call(out_capacity=needed) == SQ_OK
    assert int(call.buf.status.item()) == 0 and device_streams(call.buf) == want
    assert bool((call.buf.out[needed:] == OUT_FILL).all())
    print(f'capacity: {len(want)} tiles, {needed} device bytes, {100.0 * needed / (len(want) * 256):.1f} % of raw')


def test_reused_buffers_hold_nothing_stale():
    """One JpegBuffers: noise in every tile, then a stack with zero tiles and a zero plane (sizes go to 0, no stream of the call
    before is counted), then zeros (no stream at all), then one pixel."""
    import torch
    shape, t = (2, 40, 72), 16
    first = K.content('uniform', shape, seed=2)
    worst = int(native.lib().sq_jpeg_out_bound(*shape, native.SQ_U8, t, t))
    buf = native.jpeg_encode_planes(torch.from_numpy(first).to(_dev()), t, t, 100, capacity=worst)
    torch.cuda.synchronize()
    assert int(buf.status.item()) == 0 and all(device_streams(buf)) and device_streams(buf) == K.expected_streams(first, t, t, 100)
    second = first.copy()
    second[1] = 0
    second[0, 16:32] = 0
    second[0, :, 32:48] = 0
    for planes, with_stream in ((second, 8), (np.zeros(shape, np.uint8), 0), (K.content('pixel', shape), 1)):
        assert native.jpeg_encode_planes(torch.from_numpy(planes).to(_dev()), t, t, 100, buffers=buf, capacity=worst) is buf
        torch.cuda.synchronize()
        streams = device_streams(buf)
        assert int(buf.status.item()) == 0 and streams == K.expected_streams(planes, t, t, 100)
        assert sum(1 for s in streams if s) == with_stream
        _report(f'reuse, {with_stream} tiles with a stream', streams, planes, t, t)


def _refusals():
    I, W, U = native.SQ_ERR_INVALID, native.SQ_ERR_WORKSPACE, native.SQ_ERR_UNSUPPORTED
    out = [(f'null-{k}', (lambda c, k=k: {k: None}), I, 'NULL argument') for k in ('planes', 'scratch', 'offsets', 'out', 'status')]
    out += [('pitch-below-width', lambda c: dict(pitch=c.args['w'] - 1), I, 'pitch / plane stride'),
            ('plane-stride-too-small', lambda c: dict(plane_stride=(c.args['h'] - 1) * c.args['pitch'] + c.args['w'] - 1), I,
             'pitch / plane stride'),
            ('scratch-one-byte-short', lambda c: dict(scratch_bytes=c.need - 1), W, 'sq_jpeg_encode_planes: scratch '),
            ('scratch-off-8', lambda c: dict(scratch=c.args['scratch'] + 8, scratch_bytes=c.need), I, 'scratch must be 256-byte'),
            ('offsets-off-4', lambda c: dict(offsets=c.args['offsets'] + 4), I, 'offsets 8-byte'),
            ('dtype-uint16', lambda c: dict(dtype=native.SQ_U16), U, 'uint8 planes only'),
            ('quality-0', lambda c: dict(quality=0), I, 'quality 0'), ('quality-101', lambda c: dict(quality=101), I, 'quality 101'),
            ('negative-capacity', lambda c: dict(out_capacity=-1), I, 'negative out_capacity'),
            ('negative-planes', lambda c: dict(n_planes=-1), I, 'bad sizes')]
    for side in (0, 4, 12):
        out += [(f'tile-height-{side}', (lambda c, s=side: dict(tile_h=s)), I, 'multiples of 8'),
                (f'tile-width-{side}', (lambda c, s=side: dict(tile_w=s)), I, 'multiples of 8')]
    for side in (65504, 65528, 65536):      # T.81 holds the first two; libjpeg decodes neither
        out += [(f'tile-height-{side}', (lambda c, s=side: dict(tile_h=s)), U, f'tiles of {side} x 16'),
                (f'tile-width-{side}', (lambda c, s=side: dict(tile_w=s)), U, f'tiles of 16 x {side}')]
    out += [('tile-above-32Mi', lambda c: dict(tile_h=65496, tile_w=520), U, 'tiles of 65496 x 520'),
            ('tile-65528x520', lambda c: dict(tile_h=65528, tile_w=520), U, 'tiles of 65528 x 520')]
    return out


@pytest.fixture(scope='module')
def refusal_call():
    # (two planes: the plane stride counts; 128 spare scratch bytes: the misaligned scratch is still large enough)
    return Call(K.content('uniform', (2, 40, 72), seed=3), 16, 16, extra_scratch=128)


@pytest.mark.parametrize('name', [r[0] for r in _refusals()])
def test_refusals_return_their_status_and_touch_nothing(refusal_call, name):
    _, change, want, says = next(r for r in _refusals() if r[0] == name)
    c = refusal_call
    c.fill()
    assert c(**change(c)) == want
    message = native.lib().sq_last_error().decode()
    assert message.startswith('sq_jpeg') and says in message, message
    for what, before, after in zip(('out', 'offsets', 'status', 'scratch'), c.before, c.snapshot()):
        assert before == after, f'the refused call wrote to {what}'


def test_the_call_is_accepted_without_the_changes(refusal_call):
    c = refusal_call
    c.fill()
    assert c() == SQ_OK
    assert int(c.buf.status.item()) == 0 and device_streams(c.buf) == c.want()


def test_no_planes_is_an_empty_call(refusal_call):
    c = refusal_call
    c.fill()
    assert c(n_planes=0) == SQ_OK
    out, offsets, status, scratch = c.snapshot()
    assert int(c.buf.offsets[0].item()) == 0 and int(c.buf.status.item()) == 0
    assert out == c.before[0] and offsets[8:] == c.before[1][8:] and scratch == c.before[3]


def test_the_size_queries_are_their_formulas():
    L = native.lib()
    up256 = lambda v: (v + 255) // 256 * 256
    for name, (n, h, w), (th, tw), _ in K.EDGE_SHAPES + [(c[0], c[1], c[2], None) for c in K.FFRUNS_SHAPES] \
            + [('sweep', K.SWEEP_SHAPE, K.SWEEP_SHAPE[1:], None)]:
        tiles = n * -(-h // th) * -(-w // tw)
        intervals = tiles * (th // 8)
        assert L.sq_jpeg_chunk_count(n, h, w, th, tw) == tiles, name
        # every block 20 + 63 * 26 bits, every byte of an interval stuffed, a marker behind it; 312 bytes before the data
        assert L.sq_jpeg_out_bound(n, h, w, native.SQ_U8, th, tw) == \
            tiles * (312 + (th // 8) * (2 * (((tw // 8) * (20 + 63 * 26) + 7) // 8) + 2)), name
        assert L.sq_jpeg_scratch_bytes(n, h, w, native.SQ_U8, th, tw) == up256(4 * intervals) + up256(4 * tiles) + 256, name
