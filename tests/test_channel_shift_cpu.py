"""--channel-shift without a device: the two statements of the definition (tests/shift_ref.py, image_stitcher_amd/channelshift.py)
against each other and against independent ones, the kernel's separable form against the definition, the option's checks and
parser, and the chain's byte counts with the new buffer.  Every comparison is equality."""
import itertools
import os
import re

import numpy as np
import pytest

import shift_cases
import shift_ref
from image_stitcher_amd import channelshift, native, stitcher_cli
from image_stitcher_amd.tilechain import BUFFERS, WRITER, TileChain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [(h, w) for h, w in shift_cases.shapes('uint16') if h * w <= 400]


# ---------------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize('dtype', shift_cases.DTYPES)
def test_loop_equals_the_vectorised_form(dtype):
    shapes = [(h, w) for h, w in shift_cases.shapes(dtype) if h * w <= 400]
    assert len(shapes) >= 9
    for (h, w), shift in itertools.product(shapes, shift_cases.SHIFTS):
        planes = shift_cases.planes(dtype, h, w)
        want = shift_cases.reference(dtype, h, w, shift)
        for i in (0, 1, 4):      # noise, maximum, checkerboard
            np.testing.assert_array_equal(shift_ref.loop(planes[i], *shift), want[i], err_msg=f'{(h, w)} {shift}')


@pytest.mark.parametrize('dtype', shift_cases.DTYPES)
def test_host_module_equals_the_definition(dtype):
    for (h, w), shift in itertools.product(shift_cases.shapes(dtype), shift_cases.SHIFTS):
        planes = shift_cases.planes(dtype, h, w)
        want = shift_cases.reference(dtype, h, w, shift)
        for i, name in enumerate(shift_cases.PLANE_NAMES):
            got = channelshift.shift_image(planes[i], *shift)
            assert got.dtype == planes.dtype
            np.testing.assert_array_equal(got, want[i], err_msg=f'{(h, w)} {shift} {name}')


def test_host_module_on_rgb_and_page_stacks():
    h, w = 37, 53
    for dtype in shift_cases.DTYPES:
        planes = shift_cases.planes(dtype, h, w)
        rgb = np.ascontiguousarray(np.moveaxis(planes[[0, 3, 4]], 0, 2))
        sy, sx = [77, 0, -300], [-200, 0, 16384]
        got = channelshift.shift_image(rgb, sy, sx)
        want = shift_ref.shift_file_image(rgb, sy, sx)
        assert got.shape == rgb.shape == want.shape
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got[:, :, 1], rgb[:, :, 1])      # the plane with a zero pair is the file's
        for c in range(3):
            np.testing.assert_array_equal(got[:, :, c], shift_cases.reference(dtype, h, w, (sy[c], sx[c]))[[0, 3, 4][c]])
        # one pair for all three planes
        np.testing.assert_array_equal(channelshift.shift_image(rgb, 128, -128), shift_ref.shift_file_image(rgb, [128] * 3, [-128] * 3))
        # a page stack of one page
        page = planes[:1]
        np.testing.assert_array_equal(channelshift.shift_image(page, 77, -200), shift_ref.shift_image(page, 77, -200))
        assert channelshift.shift_image(page, 77, -200).shape == (1, h, w)
    with pytest.raises(ValueError):
        channelshift.shift_image(rgb, [1, 2], [3, 4])
    with pytest.raises(ValueError):
        channelshift.shift_image(planes[0].astype(np.float32), 1, 1)
    for bad in (16385, -16385, 1.0, True, '1', None):
        with pytest.raises(ValueError):
            channelshift.shift_image(planes[0], bad, 0)


def test_read_shifted(tmp_path):
    from image_stitcher_amd import tiffio
    img = np.array(shift_cases.planes('uint16', 37, 53)[0])
    path = str(tmp_path / 'tile.tiff')
    tiffio.write_tiff(path, img)
    np.testing.assert_array_equal(channelshift.read_shifted(path, 0, 0), img)
    np.testing.assert_array_equal(channelshift.read_shifted(path, 77, -200), shift_ref.shift_image(img, 77, -200))


@pytest.mark.parametrize('dtype', shift_cases.DTYPES)
def test_identity(dtype):
    for h, w in shift_cases.shapes(dtype):
        planes = shift_cases.planes(dtype, h, w)
        np.testing.assert_array_equal(shift_cases.reference(dtype, h, w, (0, 0)), planes)
        np.testing.assert_array_equal(channelshift.shift_image(planes[0], 0, 0), planes[0])
        np.testing.assert_array_equal(shift_ref.loop(planes[0], 0, 0), planes[0]) if h * w <= 400 else None


@pytest.mark.parametrize('dtype', shift_cases.DTYPES)
def test_whole_pixel_shifts_are_padded_slices(dtype):
    """An independent statement: out(y, x) = I(clamp(y + dy), clamp(x + dx)) is np.pad(mode='edge') followed by a slice."""
    pad = 70
    for (h, w), (dy, dx) in itertools.product(shift_cases.shapes(dtype), [(1, 0), (0, -1), (3, -9), (-2, 5), (64, -64), (-64, 64)]):
        planes = shift_cases.planes(dtype, h, w)
        padded = np.pad(planes, ((0, 0), (pad, pad), (pad, pad)), mode='edge')
        want = padded[:, pad + dy:pad + dy + h, pad + dx:pad + dx + w]
        np.testing.assert_array_equal(shift_ref.shift_image(planes, 256 * dy, 256 * dx), want, err_msg=f'{(h, w)} {(dy, dx)}')
        np.testing.assert_array_equal(channelshift.shift_image(planes[0], 256 * dy, 256 * dx), want[0])


def test_a_shift_larger_than_the_plane_gives_edge_values():
    for dtype in shift_cases.DTYPES:
        n = 0
        for h, w in shift_cases.shapes(dtype):
            if h <= 64 and w <= 64:
                planes = shift_cases.planes(dtype, h, w)
                got = shift_cases.reference(dtype, h, w, (16384, -16384))
                assert (got == planes[:, -1:, :1]).all()      # every output is the bottom-left pixel
                got = shift_cases.reference(dtype, h, w, (-16384, 16384))
                assert (got == planes[:, :1, -1:]).all()
                n += 1
        assert n >= 10


def test_half_pixel_on_two_rows_is_the_rounded_mean():
    for dtype in shift_cases.DTYPES:
        top = int(np.iinfo(dtype).max)
        plane = np.array([[0, 1, 2, top, top - 1, 7], [1, 1, 5, top, top, 8]], dtype=dtype)
        a, b = plane[0].astype(np.int64), plane[1].astype(np.int64)
        want = np.stack([(a + b + 1) >> 1, b]).astype(dtype)      # row 1 lies at the clamp: the edge row itself
        np.testing.assert_array_equal(shift_ref.shift_image(plane, 128, 0), want)
        np.testing.assert_array_equal(channelshift.shift_image(plane, 128, 0), want)
        np.testing.assert_array_equal(shift_ref.loop(plane, 128, 0), want)


@pytest.mark.parametrize('dtype', shift_cases.DTYPES)
def test_separable_clamped_index_form_equals_the_definition(dtype):
    """What csrc/shift.hip computes: constant weights, clamped tap indices, the horizontal blend first.  Its intermediates stay
    below 2^24 and 2^32."""
    top = int(np.iinfo(dtype).max)
    largest_h = largest_v = 0
    for (h, w), shift in itertools.product(shift_cases.shapes(dtype), shift_cases.SHIFTS):
        got, hmax, vmax = shift_ref.separable(shift_cases.planes(dtype, h, w), *shift)
        np.testing.assert_array_equal(got, shift_cases.reference(dtype, h, w, shift), err_msg=f'{(h, w)} {shift}')
        largest_h, largest_v = max(largest_h, hmax), max(largest_v, vmax)
    assert largest_h == top * 256 < 2 ** 24                      # reached by the all-maximum plane
    assert largest_v == top * 65536 + 32768 < 2 ** 32


# ---------------------------------------------------------------------------------------------------- the option
def test_parse_pixels():
    for text, want in (('0.5', 128), ('-0.5', -128), ('0.001953125', 1), ('-0.001953125', 0), ('64', 16384), ('-64', -16384),
                       ('0', 0), ('3', 768), ('-2', -512), ('+1.25', 320), ('0.3', 77), ('-0.78125', -200),
                       ('63.998046875', 16384), ('0.00195312', 0)):
        assert channelshift.parse_pixels(text) == want, text
    for bad in ('64.01', '-64.01', '1e1', '1/3', 'nan', '', 'inf', ' 1', '1 ', '0x10', '1_0', '.5', '5.', '--1', 'one', None, 1, 0.5):
        with pytest.raises(ValueError):
            channelshift.parse_pixels(bad)


def test_check_option():
    assert channelshift.check_option(None) == {} and channelshift.check_option({}) == {}
    got = channelshift.check_option({'A': (1, -2), 'B': [0, 0], 'C': (16384, -16384)})
    assert got == {'A': (1, -2), 'C': (16384, -16384)} and type(got) is dict
    assert all(type(v) is int for pair in got.values() for v in pair)
    for bad in ({'A': (1.0, 2)}, {'A': (True, 2)}, {'A': ('1', 2)}, {'A': (1, 16385)}, {'A': (-16385, 0)}, {'A': (1,)},
                {'A': (1, 2, 3)}, {'A': 5}, {'A': '12'}, {'A': None}, {'A': (np.int64(3), 2)}, {5: (1, 2)}, [('A', (1, 2))], 'A', 7):
        with pytest.raises(ValueError):
            channelshift.check_option(bad)


def test_command_line():
    args = stitcher_cli.parse_args(['-i', 'x', '--channel-shift', 'Fluorescence 488 nm Ex', '-0.5', '3',
                                    '--channel-shift', 'B', '0.3', '-0.78125'])
    assert stitcher_cli.channel_shifts_of(args.channel_shift) == {'Fluorescence 488 nm Ex': (-128, 768), 'B': (77, -200)}
    assert stitcher_cli.channel_shifts_of(stitcher_cli.parse_args(['-i', 'x']).channel_shift) is None
    with pytest.raises(ValueError, match="'B'"):
        stitcher_cli.channel_shifts_of([['B', '1', '1'], ['B', '2', '2']])
    with pytest.raises(ValueError):
        stitcher_cli.channel_shifts_of([['B', '1e1', '1']])
    help_text = next(kw['help'] for names, kw in stitcher_cli.FLAGS if names == ('--channel-shift',))
    assert 'imaged at (y, x) in the reference channel and at (y + DY, x + DX) in channel NAME' in help_text


def test_header_exports_and_constants():
    with open(os.path.join(ROOT, 'include', 'squidstitch.h')) as fh:
        header = fh.read()
    assert re.search(r'int\s+sq_shift_tiles\s*\(', header)
    assert re.search(r'#define\s+SQ_SHIFT_MAX\s+16384\b', header) and re.search(r'#define\s+SQ_SHIFT_MAX_SIDE\s+65535\b', header)
    assert re.search(r'#define\s+SQ_SHIFT_ROWS_PER_THREAD\s+32\b', header)
    assert 'sq_shift_tiles' in native.EXPORTS and len(native.EXPORTS['sq_shift_tiles'][1]) == 13
    assert (native.SQ_SHIFT_MAX, native.SQ_SHIFT_MAX_SIDE, native.SQ_SHIFT_ROWS_PER_THREAD) == (16384, 65535, 32)
    assert channelshift.MAX_SHIFT == shift_ref.MAX_SHIFT == native.SQ_SHIFT_MAX and channelshift.MAX_SIDE == native.SQ_SHIFT_MAX_SIDE
    assert shift_cases.RPT == native.SQ_SHIFT_ROWS_PER_THREAD
    with open(os.path.join(ROOT, 'image-stitcher_amd', 'csrc', 'Makefile')) as fh:
        assert re.search(r'^SRCS\s*=.*\bshift\.hip\b', fh.read(), re.M)
    if os.path.exists(os.path.join(ROOT, 'image-stitcher_amd', 'csrc', 'libsquidstitch.so')):
        assert hasattr(native.lib(), 'sq_shift_tiles')


def test_modules_are_written_apart():
    with open(os.path.join(ROOT, 'tests', 'shift_ref.py')) as fh:
        assert not re.search(r'^\s*(from|import)\s+\S*(channelshift|image_stitcher_amd)', fh.read(), re.M)
    with open(os.path.join(ROOT, 'image-stitcher_amd', 'channelshift.py')) as fh:
        assert not re.search(r'^\s*(from|import)\s+\S*shift_ref', fh.read(), re.M)


# ---------------------------------------------------------------------------------------------------- the chain's bytes
FH, FW, NUM_Z = 97, 131, 2
DPC_PLANES = range(2 * NUM_Z, 3 * NUM_Z)
GRID = list(itertools.product((False, True), (0, 20000), (1, 2), ('none', 'hot'), (False, True), (False, True), ('uint8', 'uint16')))


def _chain(shifted, ppm, k, despeckle, tophat, dpc, dtype):
    kw = dict(channel_shifts={0: (77, -200), 3: (0, 256)}, num_z=NUM_Z) if shifted else {}
    return TileChain(distortion_ppm=ppm, binning=k, binning_method='mean', dpc_planes=DPC_PLANES if dpc else (), dpc_gain=1,
                     despeckle=despeckle, despeckle_threshold=40, tophat_radius=5 if tophat else None, seam_qc_radius=2,
                     file_shape=(FH, FW), tile_shape=(FH // k, FW // k), dtype=dtype, **kw)


@pytest.mark.parametrize('n', [1, 6])
def test_chain_bytes_with_the_shifted_copy(n):
    for shifted, ppm, k, despeckle, tophat, dpc, dtype in GRID:
        chain = _chain(shifted, ppm, k, despeckle, tophat, dpc, dtype)
        b = np.dtype(dtype).itemsize
        raw, tile = n * FH * FW * b, n * (FH // k) * (FW // k) * b
        for derived in ((False, True) if dpc else (False,)):
            # buffer by buffer: the raw tiles, the right halves, their corrected copies, the SHIFTED copy of the staged planes
            # (the right halves have none), the binned copies, the despeckle's destination, the top-hat's scratch
            want = raw + derived * raw + bool(ppm) * (raw + derived * raw) + shifted * raw + (k > 1) * (tile + derived * tile) + \
                (despeckle != 'none') * tile + tophat * tile
            assert chain.plane_bytes(n, derived) == want, (shifted, ppm, k, despeckle, tophat, dpc, dtype, derived)
        assert chain.writer_plane_bytes(n) == raw + bool(ppm) * raw + shifted * raw + (k > 1) * tile
        # off -- by default, with None and with an empty mapping -- the counts are those of a chain without the argument
        if not shifted:
            for kw in (dict(channel_shifts=None), dict(channel_shifts={}, num_z=5)):
                other = TileChain(distortion_ppm=ppm, binning=k, binning_method='mean', dpc_planes=DPC_PLANES if dpc else (),
                                  dpc_gain=1, despeckle=despeckle, despeckle_threshold=40, tophat_radius=5 if tophat else None,
                                  seam_qc_radius=2, file_shape=(FH, FW), tile_shape=(FH // k, FW // k), dtype=dtype, **kw)
                assert other.buffers == chain.buffers and 'shift' not in [name for name, _, _ in chain.buffers]
                assert other.plane_bytes(n, dpc) == chain.plane_bytes(n, dpc)


def test_chain_table_key_and_plane_shifts():
    assert ('shift', 'file', 'chunk', 'shifted') in BUFFERS and 'shift' in WRITER
    names = [b[0] for b in BUFFERS]
    assert names.index('distortion') < names.index('shift') < names.index('binning')      # correct, shift, bin
    chain = _chain(True, 20000, 2, 'hot', True, True, 'uint16')
    assert chain.key('shift', 3, 6) == ('shift', 3, 6, FH, FW, '<u2')
    assert _chain(True, 0, 1, 'none', False, False, 'uint8').key('shift', 1, 4) == ('shift', 1, 4, FH, FW, '|u1')
    # channel 0 and channel 3 of two z levels each
    assert chain.plane_shifts([0, 1, 2]) == [(77, -200), (77, -200), (0, 0)]
    assert chain.plane_shifts([2, 3, 4, 5]) is None and chain.plane_shifts([]) is None and chain.plane_shifts(None) is None
    assert chain.plane_shifts([5, 6]) == [(0, 0), (0, 256)]
    assert _chain(False, 0, 1, 'none', False, False, 'uint8').plane_shifts([0, 1]) is None
