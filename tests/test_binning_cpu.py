"""--tile-binning without a device: the numpy definition (tests/bin_ref.py) on hand-computed planes, the package's host helper
against it, the constructor, the command line, the header and the argument checks of native.bin_tiles."""
import json
import os
import re

import numpy as np
import pytest
import torch

import bin_cases
import bin_ref
from image_stitcher_amd import binning, native, stitcher_cli, synth
from image_stitcher_amd.stitcher import Stitcher
from image_stitcher_amd.stitcher_parameters import StitchingParameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mean_level(a):
    """The truncated 2 x 2 mean of the mean-pyramid tests (tests/test_pyramid_mean_cpu.py), restated."""
    h, w = a.shape[-2] // 2 * 2, a.shape[-1] // 2 * 2
    s = a[..., 0:h:2, 0:w:2].astype(np.uint32) + a[..., 0:h:2, 1:w:2] + a[..., 1:h:2, 0:w:2] + a[..., 1:h:2, 1:w:2]
    return (s >> 2).astype(a.dtype)


# 4 x 6: K = 2 uses all of it, K = 3 drops the last row
P46 = [[1, 2, 3, 4, 5, 6],
       [7, 8, 9, 10, 11, 12],
       [0, 1, 2, 253, 254, 255],
       [0, 0, 1, 1, 255, 255]]
# 5 x 7: K = 2 drops a row and a column, K = 3 drops two rows and a column
P57 = [[10, 20, 30, 40, 50, 60, 70],
       [1, 1, 1, 1, 1, 1, 99],
       [200, 200, 200, 0, 0, 0, 99],
       [255, 255, 255, 255, 255, 255, 99],
       [99, 99, 99, 99, 99, 99, 99]]
HAND = {
    # (plane, K): the block sums S, worked out by hand
    ('P46', 2): [[18, 26, 34], [1, 257, 1019]],
    ('P46', 3): [[33, 810]],
    ('P57', 2): [[32, 72, 112], [910, 710, 510]],
    ('P57', 3): [[663, 153]],
}


@pytest.mark.parametrize('dtype', ['uint8', 'uint16'])
@pytest.mark.parametrize('method', ['mean', 'sum'])
@pytest.mark.parametrize('name,k', sorted(HAND))
def test_definition_on_hand_computed_planes(name, k, method, dtype):
    scale = 1 if dtype == 'uint8' else 257      # 255 * 257 = 65535: the uint16 plane is the uint8 one times 257
    plane = (np.array({'P46': P46, 'P57': P57}[name], dtype=np.int64) * scale).astype(dtype)
    top = int(np.iinfo(dtype).max)
    sums = np.array(HAND[(name, k)], dtype=np.int64) * scale
    want = sums // (k * k) if method == 'mean' else np.minimum(sums, top)
    got = bin_ref.bin_image(plane, k, method)
    assert got.dtype == plane.dtype and got.shape == (plane.shape[0] // k, plane.shape[1] // k)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(bin_ref.loop(plane, k, method), want)
    np.testing.assert_array_equal(binning.bin_image(plane, k, method), want)
    if method == 'sum':
        assert (want == top).any() and (want < top).any()      # both branches of the clamp


@pytest.mark.parametrize('dtype', ['uint8', 'uint16'])
def test_definition_properties(dtype):
    top = int(np.iinfo(dtype).max)
    a = np.random.default_rng(5).integers(0, top + 1, (3, 12, 18)).astype(dtype)
    # K = 2 'mean' on even sizes is the mean pyramid's level 1
    np.testing.assert_array_equal(bin_ref.bin_image(a, 2, 'mean'), mean_level(a))
    for k in range(1, 9):
        full = np.full((9, 11), top, dtype=dtype)
        assert (bin_ref.bin_image(full, k, 'sum') == top).all() and (bin_ref.bin_image(full, k, 'mean') == top).all()
        assert bin_ref.bin_image(full, k, 'sum').shape == (9 // k, 11 // k)
    for method in ('mean', 'sum'):      # K = 1 is the identity
        np.testing.assert_array_equal(bin_ref.bin_image(a, 1, method), a)
        np.testing.assert_array_equal(binning.bin_image(a[0], 1, method), a[0])
    # the dropped rows and columns reach no result
    b = a.copy()
    b[:, 10:, :] ^= 1
    b[:, :, 15:] ^= 1
    np.testing.assert_array_equal(bin_ref.bin_image(a, 5, 'sum'), bin_ref.bin_image(b, 5, 'sum'))
    # RGB: per colour plane
    rgb = np.moveaxis(a, 0, 2)
    got = bin_ref.bin_file_image(rgb, 3, 'mean')
    assert got.shape == (4, 6, 3)
    for c in range(3):
        np.testing.assert_array_equal(got[:, :, c], bin_ref.bin_image(a[c], 3, 'mean'))
    np.testing.assert_array_equal(binning.bin_image(rgb, 3, 'mean'), got)
    for bad in (dict(factor=0), dict(factor=9), dict(factor=True), dict(factor=2.0), dict(factor=2, method='median'),
                dict(factor=8, planes=a[:, :7])):
        with pytest.raises(ValueError):
            bin_ref.bin_image(bad.get('planes', a), bad['factor'], bad.get('method', 'mean'))
    with pytest.raises(ValueError):
        bin_ref.bin_image(a.astype(np.float32), 2)
    with pytest.raises(ValueError):      # hb < 1 is refused by the package as well
        binning.bin_image(a[0, :7], 8, 'mean')


@pytest.mark.parametrize('dtype', bin_cases.DTYPES)
@pytest.mark.parametrize('k', bin_cases.FACTORS)
def test_host_helper_equals_the_reference_on_the_kernel_planes(k, dtype):
    for h, w in bin_cases.shapes(k):
        planes = bin_cases.planes(dtype, k, h, w)
        for method in ('mean', 'sum'):
            want = bin_cases.reference(dtype, k, h, w, method)
            for i, plane in enumerate(planes):
                got = binning.bin_image(plane, k, method)
                assert got.dtype == plane.dtype
                np.testing.assert_array_equal(got, want[i], err_msg=f'{(h, w)} {method} {bin_cases.PLANE_NAMES[i]}')


@pytest.mark.parametrize('dtype', bin_cases.DTYPES)
@pytest.mark.parametrize('k', bin_cases.FACTORS)
def test_low_noise_plane_saturates_part_of_its_sums(k, dtype):
    """What tests/test_binning_gpu.py relies on, for the seeds chosen: on the noise of range [0, 2 M / K^2] the share of
    saturated 'sum' outputs lies in 0.1..0.9 on every shape of 1000 outputs and more."""
    seen = 0
    for h, w in bin_cases.shapes(k):
        if (h // k) * (w // k) >= 1000:
            share = bin_ref.saturated_share(bin_cases.reference(dtype, k, h, w, 'sum')[bin_cases.LOW_NOISE])
            assert 0.1 < share < 0.9, (h, w, share)
            seen += 1
    assert seen >= 3


@pytest.mark.parametrize('dtype', bin_cases.DTYPES)
@pytest.mark.parametrize('k', bin_cases.FACTORS)
def test_shapes_reach_the_vector_loads_and_the_element_path(k, dtype):
    """Every (dtype, K) has shapes whose rows all lie on 16-byte boundaries -- the 16-byte loads and the packed store, which
    every real tile takes -- with several runs per row and more than one run of rows, and shapes that have not."""
    outs = bin_cases.run_columns(dtype, k)
    assert outs == {('uint16', 2): 4, ('uint16', 3): 8, ('uint16', 4): 2, ('uint16', 5): 8, ('uint16', 6): 4, ('uint16', 7): 8,
                    ('uint16', 8): 1, ('uint8', 2): 8, ('uint8', 3): 16, ('uint8', 4): 4, ('uint8', 5): 16, ('uint8', 6): 8,
                    ('uint8', 7): 16, ('uint8', 8): 2}[(dtype, k)]
    vector = [(h, w) for h, w in bin_cases.shapes(k) if bin_cases.takes_vector_loads(dtype, k, h, w)]
    assert {(5 * k, 16 * (3 * k + 1)), (5 * k + 1, 112 * k), (4 * k, 2048)} <= set(vector)
    assert any(w // k >= 3 * outs and h // k > 4 for h, w in vector)                  # several runs, two runs of rows
    assert any((w // k) % outs for h, w in vector) or 16 % k == 0                     # a partial run at the row's end
    assert len(vector) < len(bin_cases.shapes(k))
    # the model itself: an odd pitch never, a phase K cannot reach never, a row shorter than a run never
    assert not bin_cases.takes_vector_loads(dtype, k, 5 * k, 16 * 3 * k + 1)
    assert bin_cases.takes_vector_loads(dtype, k, 5 * k, 16 * 3 * k, first_element=1) == (k % 2 == 1)
    assert not bin_cases.takes_vector_loads(dtype, k, 5 * k, k * (outs - 1), pitch=16 * k)


def _acquisition(tmp_path, **kw):
    spec = synth.GridSpec(**dict(dict(rows=1, cols=2, tile_h=18, tile_w=22, ov_y=0, ov_x=4, seed=1), **kw))
    root = str(tmp_path / 'acq')
    synth.write_acquisition(spec, root)
    return root


def _parsed(root, **kw):
    st = Stitcher(StitchingParameters(input_folder=root), **kw)
    st.get_timepoints()
    st.extract_acquisition_parameters()
    st.get_pixel_size()
    st.parse_acquisition_metadata()
    return st


def test_construction_refusals(tmp_path):
    params = StitchingParameters(input_folder=_acquisition(tmp_path))
    for factor in (True, 0, 9, 2.0, '2', None, -1):
        with pytest.raises(ValueError, match='tile_binning'):
            Stitcher(params, tile_binning=factor)
    for method in ('median', None, True, 'MEAN', 1):
        with pytest.raises(ValueError, match='tile_binning_method'):
            Stitcher(params, tile_binning=2, tile_binning_method=method)
    with pytest.raises(ValueError, match='tile_binning_method'):
        Stitcher(params, tile_binning_method='median')      # refused with or without a factor
    st = Stitcher(params)
    assert (st.tile_binning, st.tile_binning_method) == (1, 'mean')
    for factor in (1, 8, np.int64(3)):
        st = Stitcher(params, tile_binning=factor, tile_binning_method='sum')
        assert (st.tile_binning, st.tile_binning_method) == (int(factor), 'sum')


def test_metadata_is_that_of_the_binned_folder(tmp_path, capsys):
    root = _acquisition(tmp_path)
    plain = _parsed(root)
    assert (plain.input_height, plain.input_width, plain.file_height, plain.file_width) == (18, 22, 18, 22)
    assert '[binning]' not in capsys.readouterr().out
    st = _parsed(root, tile_binning=4)
    assert (st.input_height, st.input_width, st.file_height, st.file_width) == (4, 5, 18, 22)
    assert capsys.readouterr().out.count('[binning]') == 1
    # the pixel size: (sensor * K) / magnification in this order, what the pre-binned folder's JSON gives
    with open(os.path.join(root, 'acquisition parameters.json')) as fh:
        ap = json.load(fh)
    ap['sensor_pixel_size_um'] = ap['sensor_pixel_size_um'] * 4
    with open(os.path.join(root, 'acquisition parameters.json'), 'w') as fh:
        json.dump(ap, fh)
    pre = Stitcher(StitchingParameters(input_folder=root))
    pre.extract_acquisition_parameters()
    pre.get_pixel_size()
    assert st.pixel_size_um == pre.pixel_size_um and st.file_pixel_size_um == plain.pixel_size_um == plain.file_pixel_size_um
    assert st.pixel_binning == plain.pixel_binning      # left as the file says
    # get_tile bins on the host
    v = next(iter(st.get_region_data(0, 'R0').values()))
    from image_stitcher_amd.tiffio import read_image
    np.testing.assert_array_equal(st.get_tile(0, 'R0', v['x'], v['y'], v['channel'], v['z_level']),
                                  bin_ref.bin_image(read_image(v['filepath']), 4, 'mean'))
    # K larger than a tile side is refused when the metadata is parsed
    for k, ok in ((8, True), (7, True)):
        assert _parsed(root, tile_binning=k).input_height == 18 // k
    small = _acquisition(tmp_path / 'small', tile_h=6, tile_w=22)
    with pytest.raises(ValueError, match='tile_binning'):
        _parsed(small, tile_binning=7)
    assert _parsed(small, tile_binning=6).input_height == 1


def test_cli_parsing_defaults_docstring_and_help():
    a = stitcher_cli.parse_args(['-i', 'x'])
    assert a.tile_binning == 1 and a.tile_binning_method == 'mean'
    a = stitcher_cli.parse_args(['-i', 'x', '--tile-binning', '4', '--tile-binning-method', 'sum'])
    assert a.tile_binning == 4 and a.tile_binning_method == 'sum'
    for bad in (['--tile-binning', '0'], ['--tile-binning', '9'], ['--tile-binning', '2.0'], ['--tile-binning-method', 'max']):
        with pytest.raises(SystemExit):
            stitcher_cli.parse_args(['-i', 'x'] + bad)
    doc = stitcher_cli.__doc__
    for flag in ('--tile-binning', '--tile-binning-method'):
        assert '``' + flag + '``' in doc and any(names == (flag,) for names, _ in stitcher_cli.FLAGS)
    help_text = ' '.join(dict((names[0], kw['help']) for names, kw in stitcher_cli.FLAGS)['--tile-binning'].split())
    assert 'equals a run without the flag on a folder that holds the binned files' in help_text
    assert 'sensor_pixel_size_um is multiplied by K' in help_text and 'byte for byte' in help_text


def test_entry_point_is_declared_and_exported():
    header = open(os.path.join(ROOT, 'include', 'squidstitch.h')).read()
    assert re.search(r'int\s+sq_bin_tiles\s*\(', header)
    assert re.search(r'#define\s+SQ_BIN_MEAN\s+1\b', header) and re.search(r'#define\s+SQ_BIN_SUM\s+2\b', header)
    assert re.search(r'#define\s+SQ_BIN_MAX_FACTOR\s+8\b', header)
    assert 'tests/bin_ref.py' in header and 'the reference has nothing like it' in header
    assert '#define SQ_VERSION 108' in header and native.SQ_VERSION == 108
    assert 'sq_bin_tiles' in native.EXPORTS and len(native.EXPORTS['sq_bin_tiles'][1]) == 13
    assert (native.SQ_BIN_MEAN, native.SQ_BIN_SUM, native.SQ_BIN_MAX_FACTOR) == (1, 2, 8)
    assert native.BIN_METHODS == {'mean': 1, 'sum': 2}
    makefile = open(os.path.join(ROOT, 'image-stitcher_amd', 'csrc', 'Makefile')).read()
    assert 'bin.hip' in makefile.split() and os.path.exists(os.path.join(ROOT, 'image-stitcher_amd', 'csrc', 'bin.hip'))
    assert os.path.exists(native.LIB_PATH), 'the library is built before the tests run'
    assert native.lib().sq_version() == 108
    assert hasattr(native.lib(), 'sq_bin_tiles')


def test_host_side_refusals_of_bin_tiles():
    """The checkers run before anything touches a device: host tensors serve (tests/test_native_args_cpu.py)."""
    t = torch.zeros((3, 8, 8), dtype=torch.uint16)
    for factor in (True, 1, 9, 2.0, '2', None):
        with pytest.raises(ValueError, match='binning factor'):
            native.bin_tiles(t, factor)
    for method in ('median', None, 1, 'MEAN'):
        with pytest.raises(ValueError, match='binning method'):
            native.bin_tiles(t, 2, method)
    with pytest.raises(ValueError, match='device tensor'):
        native.bin_tiles(t, 2)                       # a host tensor
    with pytest.raises(ValueError, match='device tensor'):
        native.bin_tiles(np.zeros((8, 8), np.uint16), 2)
    # what bin_tiles asks of its planes is what the shared checkers say
    assert native._plane_layout(t[::2], 'tiles') == (2, 8, 8, 128, 8)
    with pytest.raises(ValueError):
        native._plane_layout(t.permute(0, 2, 1), 'tiles')
    assert native._int_in(np.int64(8), 2, native.SQ_BIN_MAX_FACTOR, 'binning factor') == 8
