"""--background-subtract tophat without a device: the numpy definition against scipy and its own properties, the options'
parsing and refusals, and the declarations of the entry point."""
import os
import re

import numpy as np
import pytest

import tophat_ref
from image_stitcher_amd import native, stitcher_cli, synth
from image_stitcher_amd.stitcher import Stitcher
from image_stitcher_amd.stitcher_parameters import StitchingParameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [((64, 96), 3), ((5, 7), 4), ((33, 31), 16), ((1, 1), 1), ((100, 3), 2)]


def _tile(dtype, h, w, seed=1):
    return tophat_ref.sample_planes(dtype, h, w, seed)[0, 0]


@pytest.mark.parametrize('dtype', ['uint8', 'uint16'])
@pytest.mark.parametrize('shape,radius', SHAPES)
def test_reference_equals_scipy(dtype, shape, radius):
    ndi = pytest.importorskip('scipy.ndimage')
    img = _tile(dtype, *shape)
    k = 2 * radius + 1
    e = ndi.minimum_filter(img, size=k, mode='constant', cval=np.iinfo(img.dtype).max)
    o = ndi.maximum_filter(e, size=k, mode='constant', cval=0)
    np.testing.assert_array_equal(tophat_ref.tophat(img, radius), img - o)
    np.testing.assert_array_equal(tophat_ref.erode(img, radius), e)


@pytest.mark.parametrize('dtype', ['uint8', 'uint16'])
@pytest.mark.parametrize('shape,radius', SHAPES + [((9, 40), 1)])
def test_reference_equals_the_two_dimensional_definition(dtype, shape, radius):
    for plane in tophat_ref.sample_planes(dtype, *shape).reshape((-1,) + shape):
        np.testing.assert_array_equal(tophat_ref.tophat(plane, radius), tophat_ref.brute(plane, radius))


@pytest.mark.parametrize('dtype', ['uint8', 'uint16'])
def test_properties(dtype):
    img = _tile(dtype, 40, 52)
    for radius in (1, 3, 60):      # 60: larger than the tile
        out = tophat_ref.tophat(img, radius)
        assert out.dtype == img.dtype and out.shape == img.shape and (out <= img).all()
        opened = tophat_ref.opening(img, radius)
        np.testing.assert_array_equal(tophat_ref.opening(opened, radius), opened)      # idempotent on its own opening
        np.testing.assert_array_equal(tophat_ref.tophat(opened, radius), np.zeros_like(img))
    const = np.full((17, 9), 77, dtype=dtype)
    assert not tophat_ref.tophat(const, 2).any()
    np.testing.assert_array_equal(tophat_ref.tophat(img, 60), img - img.min())           # the window covers the whole tile
    assert tophat_ref.tophat(np.array([[5]], dtype=dtype), 1)[0, 0] == 0
    assert len(np.unique(tophat_ref.tophat(_tile(dtype, 64, 96), 3))) > 10               # far from degenerate
    rgb = np.stack([img, img[::-1], img[:, ::-1]], axis=2)
    got = tophat_ref.tophat_image(rgb, 2)
    for k in range(3):
        np.testing.assert_array_equal(got[:, :, k], tophat_ref.tophat(rgb[:, :, k], 2))


def test_cli_parsing_and_defaults():
    a = stitcher_cli.parse_args(['-i', 'x'])
    assert a.background_subtract == 'none' and a.background_radius == 50
    a = stitcher_cli.parse_args(['-i', 'x', '--background-subtract', 'tophat', '--background-radius', '7'])
    assert a.background_subtract == 'tophat' and a.background_radius == 7
    with pytest.raises(SystemExit):
        stitcher_cli.parse_args(['-i', 'x', '--background-subtract', 'rolling-ball'])
    doc = stitcher_cli.__doc__
    assert 'eighteen switches' in doc
    for flag in ('--background-subtract', '--background-radius'):
        assert flag + '``' in doc and any(names == (flag,) for names, _ in stitcher_cli.FLAGS)


def test_construction_refusals(tmp_path):
    spec = synth.GridSpec(rows=1, cols=1, tile_h=16, tile_w=16, ov_y=0, ov_x=0, seed=1)
    root = str(tmp_path / 'acq')
    synth.write_acquisition(spec, root)
    params = StitchingParameters(input_folder=root)
    for radius in (0, 128, -1, 2.5, True):
        with pytest.raises(ValueError, match='background_radius'):
            Stitcher(params, background_subtract='tophat', background_radius=radius)
    with pytest.raises(ValueError, match='background_subtract'):
        Stitcher(params, background_subtract='rolling-ball')
    st = Stitcher(params, background_radius=9)      # a radius without the method: accepted and unused
    assert st.background_subtract == 'none' and st.background_radius == 9
    st = Stitcher(params)
    assert st.background_subtract == 'none' and st.background_radius == 50
    st = Stitcher(params, background_subtract='tophat', background_radius=127)
    assert (st.background_subtract, st.background_radius) == ('tophat', 127)


def test_entry_point_is_declared():
    header = open(os.path.join(ROOT, 'include', 'squidstitch.h')).read()
    assert re.search(r'int\s+sq_tophat_tiles\s*\(', header) and re.search(r'int64_t\s+sq_tophat_scratch_bytes\s*\(', header)
    assert '#define SQ_VERSION 108' in header and native.SQ_VERSION == 108
    assert 'sq_tophat_tiles' in native.EXPORTS and 'sq_tophat_scratch_bytes' in native.EXPORTS
    assert len(native.EXPORTS['sq_tophat_tiles'][1]) == 11
    makefile = open(os.path.join(ROOT, 'image-stitcher_amd', 'csrc', 'Makefile')).read()
    assert 'tophat.hip' in makefile and os.path.exists(os.path.join(ROOT, 'image-stitcher_amd', 'csrc', 'tophat.hip'))
    if os.path.exists(native.LIB_PATH):
        assert native.lib().sq_version() == 108
        assert native.tophat_scratch_bytes(6, 33, 31, 'uint16') >= 6 * 33 * 31 * 2
        with pytest.raises(ValueError):
            native.tophat_scratch_bytes(1, 8, 8, 'float32')
