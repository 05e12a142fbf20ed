"""--despeckle without a device: the numpy definition against scipy, against a per-pixel loop and its own properties, the
options' parsing and refusals, and the declarations of the entry point.  Every comparison is equality."""
import os
import re

import numpy as np
import pytest

import despeckle_ref
import tophat_ref
from image_stitcher_amd import native, stitcher_cli, synth
from image_stitcher_amd.stitcher import Stitcher
from image_stitcher_amd.stitcher_parameters import StitchingParameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCIPY_SHAPES = [(1, 1), (1, 300), (300, 1), (2, 2), (3, 5), (33, 31), (257, 255)]
LOOP_SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (3, 5), (33, 31)]


def _top(dtype):
    return int(np.iinfo(np.dtype(dtype)).max)


@pytest.mark.parametrize('dtype', ['uint8', 'uint16'])
@pytest.mark.parametrize('shape', SCIPY_SHAPES)
def test_reference_equals_scipy_median(dtype, shape):
    ndi = pytest.importorskip('scipy.ndimage')
    planes = tophat_ref.sample_planes(dtype, *shape).reshape((-1,) + shape)
    for plane in planes:
        want = ndi.median_filter(plane, size=3, mode='nearest')
        np.testing.assert_array_equal(despeckle_ref.median9(plane), want)
        out, fired = despeckle_ref.despeckle(plane, 0, 'both')
        np.testing.assert_array_equal(out, want)
        np.testing.assert_array_equal(fired, want != plane)
    np.testing.assert_array_equal(despeckle_ref.median9(planes), np.stack([despeckle_ref.median9(p) for p in planes]))


@pytest.mark.parametrize('dtype', ['uint8', 'uint16'])
@pytest.mark.parametrize('mode', ['hot', 'both'])
@pytest.mark.parametrize('shape', LOOP_SHAPES)
def test_reference_equals_the_per_pixel_loop(shape, mode, dtype):
    planes = tophat_ref.sample_planes(dtype, *shape).reshape((-1,) + shape)
    rng = np.random.default_rng(5)
    planes = np.concatenate([planes, rng.integers(0, _top(dtype) + 1, (1,) + shape).astype(dtype)])
    for threshold in (0, 1, 40, _top(dtype)):
        got, fired = despeckle_ref.despeckle(planes, threshold, mode)
        assert got.dtype == planes.dtype and fired.dtype == bool
        for i, plane in enumerate(planes):
            want, want_fired = despeckle_ref.loop(plane, threshold, mode)
            np.testing.assert_array_equal(got[i], want)
            np.testing.assert_array_equal(fired[i], want_fired)


@pytest.mark.parametrize('dtype', ['uint8', 'uint16'])
def test_properties(dtype):
    top = _top(dtype)
    img = tophat_ref.sample_planes(dtype, 40, 52)[0, 0]
    rng = np.random.default_rng(2)
    noisy = rng.integers(0, top + 1, (40, 52)).astype(dtype)
    for plane in (img, noisy):
        for threshold in (0, 1, 40):
            hot, fired_hot = despeckle_ref.despeckle(plane, threshold, 'hot')
            assert (hot <= plane).all()                                   # hot never raises a pixel
            np.testing.assert_array_equal(fired_hot, hot != plane)
            both, fired_both = despeckle_ref.despeckle(plane, threshold, 'both')
            np.testing.assert_array_equal(fired_both, both != plane)
            assert (fired_hot <= fired_both).all()
        for mode in despeckle_ref.MODES:                                  # T = dtype max: the identity
            out, fired = despeckle_ref.despeckle(plane, top, mode)
            np.testing.assert_array_equal(out, plane)
            assert not fired.any()
    assert despeckle_ref.despeckle(noisy, 0, 'both')[1].mean() > 0.5      # far from degenerate
    const = np.full((17, 9), 77, dtype=dtype)
    for mode in despeckle_ref.MODES:
        out, fired = despeckle_ref.despeckle(const, 0, mode)
        np.testing.assert_array_equal(out, const)
        assert not fired.any()
    # one maximal pixel on a ramp: replaced, its eight neighbours untouched -- in the interior, at the corners, on the edges
    h, w = 12, 15
    ramp = (np.arange(h)[:, None] * 3 + np.arange(w)[None, :] * 2).astype(dtype)
    spots = [(5, 7), (0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, 6), (h - 1, 6), (4, 0), (4, w - 1)]
    for y, x in spots:
        plane = ramp.copy()
        plane[y, x] = top
        for mode in despeckle_ref.MODES:
            out, fired = despeckle_ref.despeckle(plane, 20, mode)
            assert fired[y, x] and fired.sum() == 1 and out[y, x] < top
            assert out[y, x] == despeckle_ref.median9(plane)[y, x]
            rest = np.ones((h, w), bool)
            rest[y, x] = False
            np.testing.assert_array_equal(out[rest], ramp[rest])
    # two adjacent hot pixels: both replaced (the median of nine withstands up to four outliers)
    for (y0, x0), (y1, x1) in (((5, 7), (5, 8)), ((5, 7), (6, 7)), ((5, 7), (6, 8)), ((0, 5), (0, 6))):
        plane = ramp.copy()
        plane[y0, x0] = plane[y1, x1] = top
        out, fired = despeckle_ref.despeckle(plane, 20, 'hot')
        assert fired[y0, x0] and fired[y1, x1] and fired.sum() == 2 and out.max() < top
    # one dead pixel: 'both' replaces it, 'hot' leaves it
    plane = ramp.copy() + 100
    plane[5, 7] = 0
    assert despeckle_ref.despeckle(plane, 20, 'both')[1][5, 7] and not despeckle_ref.despeckle(plane, 20, 'hot')[1].any()
    # RGB: the colours are filtered independently
    rgb = np.stack([img, img[::-1], noisy], axis=2)
    got = despeckle_ref.despeckle_image(rgb, 3, 'both')
    assert got.shape == rgb.shape and got.dtype == rgb.dtype
    for k in range(3):
        np.testing.assert_array_equal(got[:, :, k], despeckle_ref.despeckle(rgb[:, :, k], 3, 'both')[0])
    np.testing.assert_array_equal(despeckle_ref.despeckle_image(img, 3, 'hot'), despeckle_ref.despeckle(img, 3, 'hot')[0])
    for bad in (dict(threshold=-1, mode='hot'), dict(threshold=65536, mode='hot'), dict(threshold=3, mode='cold')):
        with pytest.raises(ValueError):
            despeckle_ref.despeckle(img, **bad)
    with pytest.raises(ValueError):
        despeckle_ref.despeckle(img.astype(np.float32), 3, 'hot')


def test_cli_parsing_and_defaults():
    a = stitcher_cli.parse_args(['-i', 'x'])
    assert a.despeckle == 'none' and a.despeckle_threshold == 1000
    a = stitcher_cli.parse_args(['-i', 'x', '--despeckle', 'both', '--despeckle-threshold', '40'])
    assert a.despeckle == 'both' and a.despeckle_threshold == 40
    assert stitcher_cli.parse_args(['-i', 'x', '--despeckle', 'hot']).despeckle == 'hot'
    with pytest.raises(SystemExit):
        stitcher_cli.parse_args(['-i', 'x', '--despeckle', 'median'])
    with pytest.raises(SystemExit):
        stitcher_cli.parse_args(['-i', 'x', '--despeckle-threshold', '1.5'])
    doc = stitcher_cli.__doc__
    assert 'eighteen switches' in doc
    for flag in ('--despeckle', '--despeckle-threshold'):
        assert '``' + flag + '``' in doc and any(names == (flag,) for names, _ in stitcher_cli.FLAGS)
    help_text = dict((names[0], kw['help']) for names, kw in stitcher_cli.FLAGS)['--despeckle']
    assert 'raw tiles' in help_text


def test_construction_refusals(tmp_path):
    spec = synth.GridSpec(rows=1, cols=1, tile_h=16, tile_w=16, ov_y=0, ov_x=0, seed=1)
    root = str(tmp_path / 'acq')
    synth.write_acquisition(spec, root)
    params = StitchingParameters(input_folder=root)
    for threshold in (-1, 65536, 2.5, True, '7', None):
        with pytest.raises(ValueError, match='despeckle_threshold'):
            Stitcher(params, despeckle='hot', despeckle_threshold=threshold)
    with pytest.raises(ValueError, match='despeckle_threshold'):
        Stitcher(params, despeckle_threshold=-1)                # refused with or without a mode
    for mode in ('median', None, True, 'HOT'):
        with pytest.raises(ValueError, match='despeckle'):
            Stitcher(params, despeckle=mode)
    st = Stitcher(params, despeckle_threshold=7)                # a threshold without a mode: accepted and unused
    assert st.despeckle == 'none' and st.despeckle_threshold == 7
    st = Stitcher(params)
    assert st.despeckle == 'none' and st.despeckle_threshold == 1000
    assert st.despeckle_replaced == {} and st.despeckle_staged == {}
    for threshold in (0, 65535, np.int64(12)):
        st = Stitcher(params, despeckle='both', despeckle_threshold=threshold)
        assert (st.despeckle, st.despeckle_threshold) == ('both', int(threshold))


@pytest.mark.parametrize('dtype,threshold,ok', [('uint8', 1000, False), ('uint8', 255, False), ('uint8', 254, True),
                                                ('uint16', 65535, False), ('uint16', 65534, True), ('uint16', 1000, True)])
def test_threshold_is_checked_against_the_dtype(tmp_path, dtype, threshold, ok):
    """A threshold that could never fire is refused once the dtype is known (the default on uint8 data)."""
    spec = synth.GridSpec(rows=1, cols=2, tile_h=16, tile_w=16, ov_y=0, ov_x=4, seed=1, dtype=dtype)
    root = str(tmp_path / 'acq')
    synth.write_acquisition(spec, root)

    def parsed(**kw):
        st = Stitcher(StitchingParameters(input_folder=root), **kw)
        st.get_timepoints()
        st.extract_acquisition_parameters()
        st.get_pixel_size()
        st.parse_acquisition_metadata()
        return st

    if ok:
        assert parsed(despeckle='hot', despeckle_threshold=threshold).dtype == np.dtype(dtype).type
    else:
        with pytest.raises(ValueError, match='despeckle_threshold'):
            parsed(despeckle='hot', despeckle_threshold=threshold)
    parsed(despeckle_threshold=threshold)                       # without a mode the threshold is unused


def test_entry_point_is_declared():
    header = open(os.path.join(ROOT, 'include', 'squidstitch.h')).read()
    assert re.search(r'int\s+sq_despeckle_tiles\s*\(', header)
    assert re.search(r'#define\s+SQ_DESPECKLE_HOT\s+1\b', header) and re.search(r'#define\s+SQ_DESPECKLE_BOTH\s+2\b', header)
    assert 'tests/despeckle_ref.py' in header
    assert '#define SQ_VERSION 108' in header and native.SQ_VERSION == 108
    assert 'sq_despeckle_tiles' in native.EXPORTS and len(native.EXPORTS['sq_despeckle_tiles'][1]) == 14
    assert (native.SQ_DESPECKLE_HOT, native.SQ_DESPECKLE_BOTH) == (1, 2)
    assert native.DESPECKLE_MODES == {'hot': 1, 'both': 2}
    makefile = open(os.path.join(ROOT, 'image-stitcher_amd', 'csrc', 'Makefile')).read()
    assert 'despeckle.hip' in makefile and os.path.exists(os.path.join(ROOT, 'image-stitcher_amd', 'csrc', 'despeckle.hip'))
    if os.path.exists(native.LIB_PATH):
        assert native.lib().sq_version() == 108
        assert hasattr(native.lib(), 'sq_despeckle_tiles')
