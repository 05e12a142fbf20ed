"""Guide channel and depth-map store of the best-focus projection without a device: the two flags, the constructor's refusals,
the numpy definition against hand-computed cases, the new entry points of the library and the depth store's host writer."""
import json
import os

import numpy as np
import pytest

from focus_guide_ref import focus_guide_reference, select_by_depth, unsigned_depth
from image_stitcher_amd import native, omezarr, stitcher_cli
from image_stitcher_amd.stitcher import Stitcher
from image_stitcher_amd.stitcher_parameters import StitchingParameters


def test_flags_parse_with_their_defaults(tmp_path):
    a = stitcher_cli.parse_args(['-i', str(tmp_path)])
    assert a.focus_guide_channel is None and a.focus_depth_map is False
    a = stitcher_cli.parse_args(['-i', str(tmp_path), '--z-projection', 'focus', '--focus-guide-channel',
                                 'Fluorescence 488 nm Ex', '--focus-depth-map'])
    assert a.focus_guide_channel == 'Fluorescence 488 nm Ex' and a.focus_depth_map is True


def test_flags_reach_the_stitcher(tmp_path, monkeypatch):
    seen = {}

    class Fake:
        def __init__(self, params, **kw):
            seen.update(kw)

        def run(self):
            seen['ran'] = True

    monkeypatch.setattr(stitcher_cli, 'Stitcher', Fake)
    stitcher_cli.main(['-i', str(tmp_path), '--z-projection', 'focus-only', '--focus-guide-channel', 'BF_G', '--focus-depth-map'])
    assert seen['focus_guide_channel'] == 'BF_G' and seen['focus_depth_map'] is True and seen['ran']
    stitcher_cli.main(['-i', str(tmp_path)])
    assert seen['focus_guide_channel'] is None and seen['focus_depth_map'] is False


def test_constructor_refuses_the_options_without_a_focus_projection(tmp_path):
    params = StitchingParameters(input_folder=str(tmp_path))
    for proj in ('none', 'max', 'max-only'):
        with pytest.raises(ValueError, match='focus_guide_channel'):
            Stitcher(params, z_projection=proj, focus_guide_channel='488')
        with pytest.raises(ValueError, match='focus_depth_map'):
            Stitcher(params, z_projection=proj, focus_depth_map=True)
    for proj in ('focus', 'focus-only'):
        s = Stitcher(params, z_projection=proj, focus_guide_channel='488', focus_depth_map=True)
        assert s.focus_guide_channel == '488' and s.focus_depth_map is True
    s = Stitcher(params, z_projection='focus')
    assert s.focus_guide_channel is None and s.focus_depth_map is False


def test_cli_reports_the_refusal(tmp_path, capsys):
    with pytest.raises(SystemExit) as exc:
        stitcher_cli.main(['-i', str(tmp_path), '--z-projection', 'max', '--focus-depth-map'])
    assert exc.value.code == 1
    assert 'focus_depth_map' in capsys.readouterr().err


def test_unknown_guide_is_refused_with_the_names_there_are(tmp_path):
    from image_stitcher_amd import synth
    spec = synth.GridSpec(rows=1, cols=2, tile_h=16, tile_w=16, ov_y=2, ov_x=2, nz=2, channels=tuple(synth.DEFAULT_CHANNELS[:2]),
                          seed=1)
    root = str(tmp_path / 'acq')
    synth.write_acquisition(spec, root)
    st = Stitcher(StitchingParameters(input_folder=root), z_projection='focus-only', focus_guide_channel='no such channel')
    st.get_timepoints()
    st.extract_acquisition_parameters()
    st.get_pixel_size()
    with pytest.raises(ValueError, match='focus_guide_channel') as exc:
        st.parse_acquisition_metadata()
    for name in st.monochrome_channels:
        assert name in str(exc.value)
    ok = Stitcher(StitchingParameters(input_folder=root), z_projection='focus-only', focus_guide_channel=st.monochrome_channels[1])
    ok.get_timepoints()
    ok.extract_acquisition_parameters()
    ok.get_pixel_size()
    ok.parse_acquisition_metadata()
    assert ok._guide == 1


# --- the numpy definition, by hand.  One 1 x 3 tile at canvas columns 1..3 of a 1 x 5 canvas; R = 0, so the score of a pixel is
# its own modified Laplacian: [1, 5, 2] -> [4, 7, 3], a flat tile -> 0.
RECTS = np.array([[0, 0, 1, 3, 0, 1]])
SHARP = np.array([[1, 5, 2]], dtype=np.uint16)
FLAT = np.full((1, 3), 9, dtype=np.uint16)


def _planes(*tiles):
    return np.stack(tiles)[:, None]


def test_follower_takes_the_guides_plane_not_its_own_sharpest():
    guide = [(_planes(FLAT, SHARP), RECTS, None, [0, 1])]              # the guide is sharp at z = 1
    follower = [(_planes(SHARP + 100, FLAT + 50), RECTS, None, [0, 1])]   # the follower, on its own, would choose z = 0
    outs, depth = focus_guide_reference([guide, follower], 0, 1, 5, 0, 2)
    assert depth.tolist() == [[-1, 1, 1, 1, -1]]
    assert outs[0].tolist() == [[0, 1, 5, 2, 0]]
    assert outs[1].tolist() == [[0, 59, 59, 59, 0]]
    # the other way round: the follower decides, and the first channel takes ITS depth
    outs, depth = focus_guide_reference([guide, follower], 1, 1, 5, 0, 2)
    assert depth.tolist() == [[-1, 0, 0, 0, -1]]
    assert outs[0].tolist() == [[0, 9, 9, 9, 0]] and outs[1].tolist() == [[0, 101, 105, 102, 0]]


def test_follower_plane_missing_at_the_guides_depth_gives_zero():
    guide = [(_planes(FLAT, SHARP), RECTS, None, [0, 1])]
    follower = [(_planes(SHARP + 100), RECTS, None, [0])]              # no plane at z = 1 at all
    outs, depth = focus_guide_reference([guide, follower], 0, 1, 5, 0, 2)
    assert depth.tolist() == [[-1, 1, 1, 1, -1]] and outs[1].tolist() == [[0, 0, 0, 0, 0]]
    # a plane at z = 1 that covers only column 3 (its own rectangle list: ragged input)
    narrow = np.array([[0, 2, 1, 1, 0, 3]])
    follower = [(_planes(SHARP + 100), RECTS, None, [0]), (_planes(SHARP + 200), narrow, None, [1])]
    outs, _ = focus_guide_reference([guide, follower], 0, 1, 5, 0, 2)
    assert outs[1].tolist() == [[0, 0, 0, 202, 0]]


def test_uncovered_guide_gives_zero_and_depth_zero_in_the_unsigned_plane():
    left = np.array([[0, 0, 1, 2, 0, 0]])                               # the guide covers columns 0..1 only
    guide = [(_planes(SHARP, FLAT), left, None, [0, 1])]
    follower = [(_planes(SHARP + 100, FLAT + 50), RECTS, None, [0, 1])]   # the follower covers columns 1..3
    outs, depth = focus_guide_reference([guide, follower], 0, 1, 5, 0, 2)
    assert depth.tolist() == [[0, 0, -1, -1, -1]]
    assert outs[1].tolist() == [[0, 101, 0, 0, 0]]
    u = unsigned_depth(depth, 2)
    assert u.dtype == np.uint8 and u.tolist() == [[1, 1, 0, 0, 0]]
    assert unsigned_depth(depth, 300).dtype == np.uint16
    stack = np.arange(2 * 5, dtype=np.uint16).reshape(2, 1, 5) + 1
    assert select_by_depth(stack, depth).tolist() == [[1, 2, 0, 0, 0]]


def test_entry_points_and_version():
    assert 'sq_fuse_select_depth' in native.EXPORTS and 'sq_focus_depth_plane' in native.EXPORTS
    L = native.lib()
    assert L.sq_fuse_select_depth is not None and L.sq_focus_depth_plane is not None
    assert L.sq_version() == 108 and native.SQ_VERSION == 108
    assert native.SQ_SELECT_ACCUMULATE == 32
    assert native.depth_dtype_for(10) == np.uint8 and native.depth_dtype_for(255) == np.uint8
    assert native.depth_dtype_for(256) == np.uint16 and native.depth_dtype_for(300) == np.uint16
    with pytest.raises(ValueError):
        native.depth_dtype_for(0)
    # refusals that need no device: a depth dtype that is neither uint8 nor uint16, and a missing plane
    assert L.sq_focus_depth_plane(None, 4, 4, 4, None, 4, native.sq_dtype_of('float32'), None) == -1
    assert b'dtype' in L.sq_last_error()
    assert L.sq_focus_depth_plane(None, 4, 4, 4, None, 4, native.sq_dtype_of('uint8'), None) == -1
    assert L.sq_fuse_select_depth(None, None, 0, native.sq_dtype_of('uint8'), None, 0, None) == -1


@pytest.mark.parametrize('num_z,dtype', [(10, np.uint8), (300, np.uint16)])
@pytest.mark.parametrize('guide', [None, 'B'])
def test_depth_store_from_the_host_writer(tmp_path, num_z, dtype, guide):
    rng = np.random.default_rng(num_z)
    names = ['A', 'B', 'C']
    labels = omezarr.depth_labels(names, guide)
    assert labels == (['depth(B)'] if guide else ['depth(A)', 'depth(B)', 'depth(C)'])
    depth = unsigned_depth(rng.integers(-1, num_z, (1, len(labels), 1, 75, 101)), num_z)
    assert depth.dtype == dtype and depth.max() == num_z
    path = str(tmp_path / 'R0_stitched_depth.ome.zarr')
    omezarr.write_depth_store(path, depth, num_z=num_z, labels=labels, pixel_size_um=0.5, dz_um=1.5, num_levels=3,
                              chunks=(1, 1, 1, 32, 32), compression='zlib')
    level0 = omezarr.read_array(os.path.join(path, '0'))
    assert level0.shape == (1, len(labels), 1, 75, 101) and level0.dtype == dtype
    np.testing.assert_array_equal(level0, depth)
    # levels above 0: nearest (index 2 o + 1 of the level before), never a mean -- every value is one of level 0's
    from oracle import stitch_oracle as O
    want = O.pyramid_nearest(depth, 3)
    for lv in (1, 2):
        np.testing.assert_array_equal(omezarr.read_array(os.path.join(path, str(lv))), want[lv])
    with open(os.path.join(path, '.zattrs')) as fh:
        attrs = json.load(fh)
    assert 'type' not in attrs['multiscales'][0]
    assert [c['label'] for c in attrs['omero']['channels']] == labels
    assert all(c['window']['start'] == 0 and c['window']['end'] == num_z for c in attrs['omero']['channels'])
    assert attrs['multiscales'][0]['datasets'][1]['coordinateTransformations'][0]['scale'] == [1, 1, 1.5, 1.0, 1.0]
    assert not os.path.exists(omezarr.sidecar_paths(path)[0]) and not os.path.exists(omezarr.sidecar_paths(path)[1])
    with pytest.raises(ValueError):
        omezarr.write_depth_store(path, depth.astype(np.float32), num_z=num_z, labels=labels, pixel_size_um=0.5)


def test_stitcher_writes_the_depth_store_by_nearest_under_the_mean_pyramid(tmp_path):
    """save_region_depth of a Stitcher whose run uses pyramid_method='mean' and percentile windows: nearest levels, the
    0 ... num_z window, no sidecars."""
    params = StitchingParameters(input_folder=str(tmp_path), output_format='.ome.zarr')
    st = Stitcher(params, z_projection='focus-only', focus_depth_map=True, pyramid_method='mean', contrast_limits='percentile',
                  zarr_compression='zlib')
    st.output_folder = str(tmp_path / 'out')
    st.monochrome_channels, st.num_c, st.num_z, st.pixel_size_um = ['A', 'B'], 2, 10, 0.75
    st.num_pyramid_levels, st.chunks, st.acquisition_params = 2, (1, 1, 1, 16, 16), {}
    rng = np.random.default_rng(2)
    depth = unsigned_depth(rng.integers(-1, 10, (1, 2, 1, 40, 50)), 10)
    path = st.save_region_depth(0, 'R0', depth)
    assert path.endswith(os.path.join('0_stitched', 'R0_stitched_depth.ome.zarr'))
    np.testing.assert_array_equal(omezarr.read_array(os.path.join(path, '0')), depth)
    np.testing.assert_array_equal(omezarr.read_array(os.path.join(path, '1')), depth[..., 1::2, 1::2][..., :20, :25])
    with open(os.path.join(path, '.zattrs')) as fh:
        attrs = json.load(fh)
    assert [c['label'] for c in attrs['omero']['channels']] == ['depth(A)', 'depth(B)']
    assert all(c['window']['end'] == 10 for c in attrs['omero']['channels']) and 'type' not in attrs['multiscales'][0]
