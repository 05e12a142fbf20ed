"""--composite without a GPU: the numpy definition against plain per-pixel loops, the level choice, the PNG writer against an
independent decoder, the sidecar, the flags and every construction-time refusal, and the two entry points' declarations."""
import json
import os
import re

import numpy as np
import pytest

import composite_ref as R
from image_stitcher_amd import composite, native, omezarr, png, stitcher_cli
from image_stitcher_amd.stitcher import Stitcher
from image_stitcher_amd.stitcher_parameters import StitchingParameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the definition
def _loops_block_mean(plane, k):
    f = 1 << k
    h, w = plane.shape
    out = np.zeros((-(-h // f), -(-w // f)), dtype=plane.dtype)
    for Y in range(out.shape[0]):
        for X in range(out.shape[1]):
            total = count = 0
            for y in range(Y * f, min(h, (Y + 1) * f)):
                for x in range(X * f, min(w, (X + 1) * f)):
                    total += int(plane[y, x])
                    count += 1
            out[Y, X] = total // count
    return out


def _loops_render(means, windows, colors):
    n, h, w = means.shape
    out = np.zeros((h, w, 3), dtype=np.uint8)
    for y in range(h):
        for x in range(w):
            for j in range(3):
                total = 0
                for c in range(n):
                    m, (a, b) = int(means[c, y, x]), windows[c]
                    v = 0 if m <= a else (255 if m >= b else (m - a) * 255 // (b - a))
                    total += v * ((colors[c] >> (16 - 8 * j)) & 0xFF) // 255
                out[y, x, j] = min(255, total)
    return out


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16])
@pytest.mark.parametrize('k', [0, 1, 2, 3])
def test_reference_equals_per_pixel_loops(dtype, k):
    rng = np.random.default_rng(k)
    top = int(np.iinfo(dtype).max)
    planes = rng.integers(0, top + 1, (3, 21, 27)).astype(dtype)      # neither side a multiple of 2, 4 or 8
    planes[0, :10] = top
    got = R.block_mean(planes, k)
    assert got.dtype == planes.dtype and got.shape == (3, -(-21 // (1 << k)), -(-27 // (1 << k)))
    for c in range(3):
        np.testing.assert_array_equal(got[c], _loops_block_mean(planes[c], k))
    if k == 0:
        np.testing.assert_array_equal(got, planes)
    windows = R.windows_of(planes, 5, 95)
    for p, win in zip(planes, windows):
        assert win == omezarr.contrast_window(np.bincount(p.ravel(), minlength=top + 1), 5, 95, top)
    colors = [0xFFCF00, 0x0000FF, 0xFFFFFF]
    np.testing.assert_array_equal(R.render(got, windows, colors), _loops_render(got, windows, colors))
    image, level, wins = R.composite(planes, colors, max(got.shape[1:]), 5, 95)
    assert level == k and wins == windows
    np.testing.assert_array_equal(image, R.render(got, windows, colors))


def test_render_saturates_and_clamps():
    means = np.array([[[0, 10, 11, 500, 1000, 65535]]] * 2, dtype=np.uint16)
    img = R.render(means, [(10, 1000), (10, 1000)], [0xFFFFFF, 0x80FF00])
    np.testing.assert_array_equal(img[0, :, 0], [0, 0, 0, 126 + 126 * 128 // 255, 255, 255])
    np.testing.assert_array_equal(img[0, :, 1], [0, 0, 0, 252, 255, 255])
    np.testing.assert_array_equal(img[0, :, 2], [0, 0, 0, 126, 255, 255])


# ------------------------------------------------------------------------------------------------ level choice
@pytest.mark.parametrize('h,w,max_side,k', [(100, 100, 100, 0), (101, 100, 100, 1), (100, 201, 100, 2), (4096, 4096, 4096, 0),
                                            (4097, 1, 4096, 1), (29108, 36428, 4096, 4), (16 * 256, 16 * 256, 16, 8),
                                            (1, 1, 16, 0), (36428, 29108, 16384, 2)])
def test_level_choice(h, w, max_side, k):
    assert composite.choose_level(h, w, max_side) == R.choose_level(h, w, max_side) == k
    f = 1 << k
    assert max(-(-h // f), -(-w // f)) <= max_side
    assert k == 0 or max(-(-h // (f // 2)), -(-w // (f // 2))) > max_side


def test_level_beyond_8_is_refused_with_the_side_that_works():
    h, w = 5000, 16 * 256 + 1      # 4097 columns need 17 pixels at k = 8
    with pytest.raises(ValueError, match=r'smallest composite_max_side that\s+works is 20\b'):
        composite.choose_level(h, w, 16)
    with pytest.raises(ValueError):
        R.choose_level(h, w, 16)
    assert composite.choose_level(h, w, 20) == 8 and composite.choose_level(h, w, 19 + 1) == R.choose_level(h, w, 20)
    with pytest.raises(ValueError, match='20'):
        composite.choose_level(h, w, 19)


# ------------------------------------------------------------------------------------------------ PNG
@pytest.mark.parametrize('shape', [(1, 1), (1, 7), (5, 1), (17, 33), (64, 64), (131, 257)])
def test_png_writer_round_trips(tmp_path, shape):
    rng = np.random.default_rng(sum(shape))
    img = rng.integers(0, 256, shape + (3,)).astype(np.uint8)
    img[: shape[0] // 2] = img[:1]      # repeated rows: something to compress
    path = png.write_rgb8(str(tmp_path / 'a.png'), img)
    with open(path, 'rb') as fh:
        data = fh.read()
    assert data == png.encode_rgb8(img)
    np.testing.assert_array_equal(R.decode_png(data), img)
    w, h, depth, ctype, comp, flt, interlace = __import__('struct').unpack('>IIBBBBB', data[16:29])
    assert (w, h, depth, ctype, comp, flt, interlace) == (shape[1], shape[0], 8, 2, 0, 0, 0)
    try:
        from PIL import Image
    except ImportError:
        return
    with Image.open(path) as im:
        assert im.mode == 'RGB'
        np.testing.assert_array_equal(np.asarray(im), img)


def test_png_writer_refuses_other_arrays():
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 3), np.uint16), np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            png.encode_rgb8(bad)


def test_decoder_handles_all_five_filter_types():
    """The test decoder is independent of the writer (which emits filter type 0 only): rows filtered by hand."""
    import struct
    import zlib
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (5, 6, 3)).astype(np.uint8)
    flat = img.reshape(5, 18).astype(np.int64)
    raw = b''
    for y in range(5):
        prev = flat[y - 1] if y else np.zeros(18, np.int64)
        a = np.concatenate([np.zeros(3, np.int64), flat[y][:-3]])
        c = np.concatenate([np.zeros(3, np.int64), prev[:-3]])
        if y == 0:
            pred = np.zeros(18, np.int64)
        elif y == 1:
            pred = a
        elif y == 2:
            pred = prev
        elif y == 3:
            pred = (a + prev) // 2
        else:
            p = a + prev - c
            pa, pb, pc = abs(p - a), abs(p - prev), abs(p - c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, prev, c))
        raw += bytes([y]) + ((flat[y] - pred) & 0xFF).astype(np.uint8).tobytes()
    chunk = lambda kind, body: struct.pack('>I', len(body)) + kind + body + struct.pack('>I', zlib.crc32(kind + body) & 0xFFFFFFFF)
    comp = zlib.compress(raw)
    data = (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', 6, 5, 8, 2, 0, 0, 0)) + chunk(b'IDAT', comp[:7]) +
            chunk(b'IDAT', comp[7:]) + chunk(b'IEND', b''))
    np.testing.assert_array_equal(R.decode_png(data), img)


# ------------------------------------------------------------------------------------------------ sidecar
def test_sidecar_schema(tmp_path):
    meta = composite.sidecar(store='R0_stitched_mip.ome.zarr', kind='mip', z=None, level=4, shape=(1820, 2277),
                             source_shape=(29108, 36428), labels=['a', 'b'], colors=[0x00FF00, 0xFFCF00],
                             windows=[(5, 900), (0, 65535)], percentiles=(0.1, 99.9))
    assert meta == {'source': {'store': 'R0_stitched_mip.ome.zarr', 'kind': 'mip', 'z': None}, 'level': 4, 'factor': 16,
                    'shape': [1820, 2277], 'source_shape': [29108, 36428],
                    'channels': [{'label': 'a', 'color': '00FF00', 'window': {'start': 5, 'end': 900}},
                                 {'label': 'b', 'color': 'FFCF00', 'window': {'start': 0, 'end': 65535}}],
                    'percentiles': [0.1, 99.9]}
    assert composite.sidecar(store='s.ome.tiff', kind='stack', z=3, level=0, shape=(2, 2), source_shape=(2, 2), labels=[], colors=[],
                             windows=[], percentiles=(1, 99))['source']['z'] == 3
    rgb = np.zeros((2, 3, 3), np.uint8)
    a, b = composite.write_outputs(str(tmp_path / 'R0_stitched_composite'), rgb, meta)
    assert a.endswith('R0_stitched_composite.png') and b.endswith('R0_stitched_composite.json')
    with open(b) as fh:
        assert json.load(fh) == meta
    with open(a, 'rb') as fh:
        np.testing.assert_array_equal(R.decode_png(fh.read()), rgb)


# ------------------------------------------------------------------------------------------------ flags and refusals
def test_cli_flags():
    args = stitcher_cli.parse_args(['-i', 'x'])
    assert (args.composite, args.composite_max_side, args.composite_z, args.composite_channels) == (False, 4096, None, None)
    args = stitcher_cli.parse_args(['-i', 'x', '--composite', '--composite-max-side', '512', '--composite-z', '3',
                                    '--composite-channels', 'Fluorescence 561 nm Ex', 'BF LED matrix full_G'])
    assert (args.composite, args.composite_max_side, args.composite_z) == (True, 512, 3)
    assert args.composite_channels == ['Fluorescence 561 nm Ex', 'BF LED matrix full_G']
    for bad in (['--composite-max-side', 'big'], ['--composite-z', '1.5'], ['--composite-channels']):
        with pytest.raises(SystemExit):
            stitcher_cli.parse_args(['-i', 'x', *bad])
    for flag in ('--composite', '--composite-max-side', '--composite-z', '--composite-channels'):
        assert flag + '``' in stitcher_cli.__doc__ and any(names == (flag,) for names, _ in stitcher_cli.FLAGS)
    assert 'eighteen switches' in stitcher_cli.__doc__


def test_construction_time_refusals(tmp_path):
    params = StitchingParameters(input_folder=str(tmp_path))
    s = Stitcher(params)
    assert (s.composite, s.composite_max_side, s.composite_z, s.composite_channels) == (False, 4096, None, None)
    s = Stitcher(params, composite=True, composite_max_side=16, composite_z=0, composite_channels=('b', 'a'))
    assert (s.composite, s.composite_max_side, s.composite_z, s.composite_channels) == (True, 16, 0, ['b', 'a'])
    assert Stitcher(params, composite=True, composite_max_side=16384).composite_max_side == 16384
    for bad in (15, 16385, 0, -4096, 100.0, '512', None, True):
        with pytest.raises(ValueError, match='composite_max_side'):
            Stitcher(params, composite=True, composite_max_side=bad)
    for bad in (-1, 1.0, '2', True):
        with pytest.raises(ValueError, match='composite_z'):
            Stitcher(params, composite=True, composite_z=bad)
    for bad in ('abc', [], ['a', 'a'], ['a', 3], [str(i) for i in range(17)]):
        with pytest.raises(ValueError, match='composite_channels'):
            Stitcher(params, composite=True, composite_channels=bad)
    # works for both output formats and both fusion modes; the windows are percentiles whatever --contrast-limits says
    tiff = StitchingParameters(input_folder=str(tmp_path), output_format='.ome.tiff')
    assert Stitcher(tiff, composite=True, fusion_mode='feather', contrast_percentiles=(2, 98)).contrast_percentiles == (2.0, 98.0)


# ------------------------------------------------------------------------------------------------ the entry points
def test_entry_points_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, 'include', 'squidstitch.h')) as fh:
        header = fh.read()
    for name in ('sq_block_mean', 'sq_composite_render'):
        assert name in native.EXPORTS
        m = re.search(r'/\*(?:(?!\*/).)*\*/\s*int\s+' + name + r'\s*\(', header, re.S)
        assert m, name
        comment = m.group(0).split('/*')[-1]
        assert 'stitcher.py:861-885' in comment and '_save_debug_slice' in comment, name
        assert hasattr(native.lib(), name)
    declared = int(re.search(r'#define\s+SQ_VERSION\s+(\d+)\b', header).group(1))
    assert declared == native.SQ_VERSION == native.lib().sq_version() == 108
    assert callable(native.block_mean) and callable(native.composite_render)
    with open(os.path.join(ROOT, 'image-stitcher_amd', 'csrc', 'Makefile')) as fh:
        assert 'composite.hip' in fh.read()
