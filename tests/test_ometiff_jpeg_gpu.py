"""``--ome-tiff-compression jpeg`` end to end.  A uint8 acquisition (3 x 3 tiles, 2 channels x 3 z, registered) and the uint8 RGB
one of tests/test_ometiff_pyramid_gpu.py are written as pyramid OME-TIFFs with JPEG tiles: EVERY tile stream of every level of
the file equals ``jpegtile.encode_tile`` of the corresponding zero-padded tile of the same run's .ome.zarr store level, byte for
byte, for both pyramid methods -- so the file holds exactly what the host definition makes of the stitched planes, and no decoder
is needed.  Below that: the writer driven directly with a partly filled last batch, two regions through one retargeted writer, the
depth map of --focus-depth-map staying deflate, the deflate file unchanged by the new code, and the refusals of a run."""
import dataclasses
import os

import numpy as np
import pytest

import jpeg_cases as K
from helpers import load_case, spec_of
from image_stitcher_amd import jpegtile as J
from image_stitcher_amd import ometiff, omezarr, synth
from image_stitcher_amd.stitcher_parameters import StitchingParameters
from test_ometiff_pyramid_gpu import LEVELS, TILE, Small, _val

pytestmark = pytest.mark.gpu

SPEC = synth.GridSpec(rows=3, cols=3, tile_h=96, tile_w=128, ov_y=20, ov_x=28, channels=tuple(synth.DEFAULT_CHANNELS[:2]), nz=3,
                      seed=12, dtype='uint8', missing=((8, 1, 0, 0),))
QUALITY = 80      # (not the default: the option has to arrive)


@pytest.fixture(scope='module')
def acquisition(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('jpg') / 'acq')
    synth.write_acquisition(SPEC, root)
    return root


def run(root, fmt, use_registration=True, **kw):
    st = Small(StitchingParameters(input_folder=root, output_format=fmt, use_registration=use_registration), **kw)
    st.run()
    return st, os.path.join(st.output_folder, '0_stitched')


def check_file_against_store(path, store, quality, n_levels=LEVELS, tile=(TILE, TILE)):
    """Every tile stream of the file is the host definition's of the store's tile; -> (tiles with a stream, zero tiles)."""
    streams = ometiff.read_tile_streams(path)
    _, ifds = ometiff.read_pyramid_structure(path)
    zero = J.encode_tile(np.zeros(tile, np.uint8), quality)
    assert len(streams) == n_levels
    real = zeros = 0
    for lv in range(n_levels):
        want = omezarr.read_array(os.path.join(store, str(lv)))
        assert want.dtype == np.uint8 and want.any()
        planes = want.reshape((-1,) + want.shape[3:])
        assert len(streams[lv]) == len(planes) == len(ifds)
        for p, plane in enumerate(planes):
            expect = K.expected_streams(plane[None], tile[0], tile[1], quality)
            assert len(streams[lv][p]) == len(expect)
            for i, (got, w) in enumerate(zip(streams[lv][p], expect)):
                assert got == (w or zero), f'level {lv} plane {p} tile {i}: {len(got)} bytes in the file, {len(w or zero)} expected'
                real += bool(w)
                zeros += not w
    for top in ifds:
        for lv, t in enumerate([top] + top['sub']):
            assert _val(t, 259) == 7 and _val(t, 262) == 1 and 317 not in t and _val(t, 258) == 8
            assert (_val(t, 323), _val(t, 322)) == tuple(tile)
    return real, zeros


@pytest.mark.parametrize('method', ['nearest', 'mean'])
def test_every_tile_stream_is_the_host_definition_of_the_store(acquisition, method, capsys):
    _, zfolder = run(acquisition, '.ome.zarr', pyramid_method=method, z_projection='max')
    st, folder = run(acquisition, '.ome.tiff', pyramid_method=method, z_projection='max', ome_tiff_layout='pyramid',
                     ome_tiff_compression='jpeg', ome_tiff_quality=QUALITY)
    out = capsys.readouterr().out
    for tag in ('', '_mip'):      # the projection follows the option
        path = os.path.join(folder, f'R0_stitched{tag}.ome.tiff')
        real, zeros = check_file_against_store(path, os.path.join(zfolder, f'R0_stitched{tag}.ome.zarr'), QUALITY)
        assert real > 0 and (zeros > 0 or tag)      # (the plane with the missing corner file)
        assert f'[ome-tiff] R0_stitched{tag}.ome.tiff: {LEVELS} levels, tiles {TILE} x {TILE}, ' in out
        assert f'bytes, jpeg quality {QUALITY}' in out
        print(f'{tag or "stack"}: {os.path.getsize(path)} bytes in the file')


def test_uint8_rgb_acquisition(tmp_path):
    """RGB files stay three grey planes (<base>_R/_G/_B) and a fluorescence channel: four JPEG-tiled planes."""
    root = str(tmp_path / 'acq')
    synth.write_acquisition(spec_of(load_case('coord_rgb')[0]), root)
    _, zfolder = run(root, '.ome.zarr', use_registration=False)
    st, folder = run(root, '.ome.tiff', use_registration=False, ome_tiff_layout='pyramid', ome_tiff_compression='jpeg')
    assert st.ome_tiff_quality == 90 and len(st.monochrome_channels) == 4
    real, _ = check_file_against_store(os.path.join(folder, 'R0_stitched.ome.tiff'), os.path.join(zfolder, 'R0_stitched.ome.zarr'), 90)
    assert real > 0


def test_two_regions_through_one_retargeted_writer(tmp_path):
    spec = dataclasses.replace(SPEC, regions=('A1', 'A2'), nz=1, missing=())
    root = str(tmp_path / 'acq')
    synth.write_acquisition(spec, root)
    _, zfolder = run(root, '.ome.zarr')
    _, folder = run(root, '.ome.tiff', ome_tiff_layout='pyramid', ome_tiff_compression='jpeg', ome_tiff_quality=QUALITY)
    for region in ('A1', 'A2'):
        real, _ = check_file_against_store(os.path.join(folder, f'{region}_stitched.ome.tiff'),
                                           os.path.join(zfolder, f'{region}_stitched.ome.zarr'), QUALITY)
        assert real > 0


def test_the_depth_map_stays_deflate(acquisition):
    """--z-projection focus --focus-depth-map: _edf follows the option, the depth file's tiles are deflate and hold the store's
    depths exactly."""
    kw = dict(z_projection='focus', focus_depth_map=True)
    _, zfolder = run(acquisition, '.ome.zarr', **kw)
    _, folder = run(acquisition, '.ome.tiff', ome_tiff_layout='pyramid', ome_tiff_compression='jpeg', ome_tiff_quality=QUALITY, **kw)
    check_file_against_store(os.path.join(folder, 'R0_stitched_edf.ome.tiff'), os.path.join(zfolder, 'R0_stitched_edf.ome.zarr'), QUALITY)
    path = os.path.join(folder, 'R0_stitched_depth.ome.tiff')
    _, ifds = ometiff.read_pyramid_structure(path)
    for top in ifds:
        for t in [top] + top['sub']:
            assert _val(t, 259) == 8 and _val(t, 317) == 2
    levels, _ = ometiff.read_pyramid_tiff(path)
    for lv in range(LEVELS):
        want = omezarr.read_array(os.path.join(zfolder, 'R0_stitched_depth.ome.zarr', str(lv)))
        for c in range(want.shape[1]):
            assert np.array_equal(levels[lv][c], want[0, c, 0]), (lv, c)


def test_the_deflate_file_is_unchanged(tmp_path):
    """A deflate run's file, byte for byte, is what the container makes of the packed streams the deflate encoder gives for the
    store's levels -- the path of the parent commit, driven here without the writer: nothing of it moved."""
    import torch
    from image_stitcher_amd import native
    root = str(tmp_path / 'acq')      # (no missing file: one group of planes, one batch, one append per level)
    synth.write_acquisition(dataclasses.replace(SPEC, nz=1, missing=()), root)
    st, folder = run(root, '.ome.tiff', ome_tiff_layout='pyramid')
    _, zfolder = run(root, '.ome.zarr')
    with open(os.path.join(folder, 'R0_stitched.ome.tiff'), 'rb') as fh:
        got = fh.read()
    levels = [omezarr.read_array(os.path.join(zfolder, 'R0_stitched.ome.zarr', str(lv))) for lv in range(LEVELS)]
    shapes = [lv.shape for lv in levels]
    xml = ometiff.ome_xml(shapes[0], np.uint8, st.monochrome_channels, st.monochrome_colors, st.pixel_size_um, st._dz_um(), 'R0_t0')
    file = ometiff.PyramidTiff(str(tmp_path / 'want.ome.tiff'), shapes, np.uint8, tile=(TILE, TILE), compression='deflate', xml=xml)
    n = shapes[0][1] * shapes[0][2]
    for lv, level in enumerate(levels):      # one batch holds both planes of this acquisition
        buf = native.deflate_encode_planes(torch.from_numpy(level.reshape((n,) + level.shape[3:])).cuda(), TILE, TILE, 2)
        torch.cuda.synchronize()
        off = buf.offsets.cpu().numpy()
        file.append(lv, list(range(n)), buf.out[:int(off[-1])].cpu().numpy(), np.diff(off))
    file.close()
    with open(str(tmp_path / 'want.ome.tiff'), 'rb') as fh:
        want = fh.read()
    assert got == want


# ---------------------------------------------------------------------------------------------------- the writer driven directly
W_SHAPE, W_LEVELS, W_BATCH, W_ZERO = (1, 7, 1, 150, 333), 3, 3, 4


def test_writer_with_a_partial_last_batch(tmp_path):
    """3, 3 and 1 planes through the two slots of a writer whose device buffers held a stale pattern: the planes behind the last
    batch's one plane are encoded as zeros (no streams), plane W_ZERO costs no tile, every stream is the host definition's."""
    import torch
    img = np.stack([K.content('image', (1,) + W_SHAPE[3:], seed=k)[0] for k in range(W_SHAPE[1])]).reshape(W_SHAPE)
    img[0, W_ZERO] = 0
    shapes = omezarr.level_shapes(W_SHAPE, W_LEVELS)
    planes = torch.from_numpy(img.reshape((-1,) + W_SHAPE[3:])).cuda()
    coords = [(0, c, 0) for c in range(W_SHAPE[1])]
    path = str(tmp_path / 'w.ome.tiff')
    meta = dict(pixel_size_um=0.5, channel_names=[f'c{k}' for k in range(7)], channel_colors=[0xFFFFFF] * 7, name='w')
    with ometiff.PyramidTiffWriter(path, shapes, np.uint8, meta=meta, chunks=(1, 1, 1, 32, 64), batch=W_BATCH, compression='jpeg',
                                   quality=75, device=planes.device, verbose=False) as w:
        assert w.matches(shapes, np.uint8, W_BATCH, 'jpeg', (1, 1, 1, 32, 64), quality=75)
        assert not w.matches(shapes, np.uint8, W_BATCH, 'jpeg', (1, 1, 1, 32, 64), quality=76)
        for slot in w._dev:
            for level in slot:
                level.fill_(0x5A)
        for b0 in range(0, len(coords), W_BATCH):
            m = min(W_BATCH, len(coords) - b0)
            w.acquire(m).copy_(planes[b0:b0 + m])
            w.submit(coords[b0:b0 + m])
    for enc in w._enc[0]:      # slot 0 took batches 0 and 2: its encoders' last offsets are batch 2's
        off = enc.offsets.cpu().numpy()
        per = enc.n_chunks // W_BATCH
        assert off[per] > 0 and (off[per:] == off[per]).all(), 'a plane behind the last batch has streams'
        assert int(enc.status.item()) == 0
    streams = ometiff.read_tile_streams(path)
    zero = J.encode_tile(np.zeros((32, 64), np.uint8), 75)
    from oracle import stitch_oracle as O
    want = O.pyramid_nearest(img, W_LEVELS)
    for lv in range(W_LEVELS):
        for k in range(W_SHAPE[1]):
            expect = [s or zero for s in K.expected_streams(want[lv][0, k], 32, 64, 75)]
            assert streams[lv][k] == expect, (lv, k)
            if k == W_ZERO:
                assert all(s == zero for s in streams[lv][k])
    assert w.bytes_written == os.path.getsize(path)


def test_noise_is_refused_with_a_message_that_names_the_way_out(tmp_path):
    """Tiles that do not shrink below raw (noise at quality 100) do not fit the buffers the writer page-locks: the run fails and
    says what to do."""
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (1, 1, 1, 64, 64), dtype=np.uint8)
    with pytest.raises(RuntimeError, match=r'quality 100.*deflate'):
        ometiff.write_pyramid_tiff(str(tmp_path / 'n.ome.tiff'), img, meta=dict(pixel_size_um=1.0), chunks=(1, 1, 1, 32, 32),
                                   compression='jpeg', quality=100, verbose=False)


def test_a_run_refuses_what_jpeg_cannot_hold(tmp_path):
    spec = dataclasses.replace(SPEC, dtype='uint16', nz=1, missing=())
    root = str(tmp_path / 'acq')
    synth.write_acquisition(spec, root)
    st = Small(StitchingParameters(input_folder=root, output_format='.ome.tiff'), ome_tiff_layout='pyramid', ome_tiff_compression='jpeg')
    with pytest.raises(ValueError, match='uint8'):
        st.run()
