"""``--ome-tiff-layout pyramid`` end to end: a 3 x 3 acquisition of small tiles (2 channels x 3 z, registered) written as a pyramid
OME-TIFF -- 32 x 32 tiles, 3 levels -- has to hold, at every level, the voxels of the same run written as an .ome.zarr store; the
file's structure is the specified one; and the default layout is still the file write_ome_tiff makes of the fused region.  Below
that, ometiff.PyramidTiffWriter driven directly (as tests/test_pyramid_gpu.py drives omezarr.PlaneStreamWriter): a partly filled
last batch over stale planes, uint8 and uint16, the default 512 x 512 tile and a non-square one, write_pyramid_tiff, a uint8 RGB
acquisition, and the files opened by a reader that is not this project's."""
import dataclasses
import os

import numpy as np
import pytest

from helpers import load_case, spec_of
from image_stitcher_amd import ometiff, omezarr, synth
from image_stitcher_amd.stitcher import Stitcher
from image_stitcher_amd.stitcher_parameters import StitchingParameters
from oracle import stitch_oracle as O
from test_pyramid_mean_gpu import mean_pyramid

pytestmark = pytest.mark.gpu

SPEC = synth.GridSpec(rows=3, cols=3, tile_h=96, tile_w=128, ov_y=20, ov_x=28, channels=tuple(synth.DEFAULT_CHANNELS[:2]), nz=3,
                      seed=11, missing=((8, 1, 0, 0),))      # (no file for the last FOV in one plane: tiles of zeros there)
LEVELS, TILE = 3, 32


class Small(Stitcher):
    """The stitcher with 32 x 32 chunks / tiles and three pyramid levels, which a canvas this small would not get."""

    def parse_acquisition_metadata(self):
        super().parse_acquisition_metadata()
        self.chunks = (1, 1, 1, TILE, TILE)

    def calculate_output_dimensions(self, timepoint, region):
        out = super().calculate_output_dimensions(timepoint, region)
        self.num_pyramid_levels = LEVELS
        return out


@pytest.fixture(scope='module')
def acquisition(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('pyr') / 'acq')
    synth.write_acquisition(SPEC, root)
    return root


def run(root, fmt, **kw):
    st = Small(StitchingParameters(input_folder=root, output_format=fmt, use_registration=True), **kw)
    st.run()
    return st, os.path.join(st.output_folder, '0_stitched')


@pytest.fixture(scope='module')
def stores(acquisition):
    """The same run as .ome.zarr, per pyramid method: {method: {'' | '_mip': [level arrays (1, C, Z, Y, X)]}}."""
    cache = {}

    def get(method):
        if method not in cache:
            _, folder = run(acquisition, '.ome.zarr', pyramid_method=method, z_projection='max')
            cache[method] = {tag: [omezarr.read_array(os.path.join(folder, f'R0_stitched{tag}.ome.zarr', str(lv)))
                                   for lv in range(LEVELS)] for tag in ('', '_mip')}
        return cache[method]
    return get


def _val(tags, tag):
    return int(tags[tag][2][0])


@pytest.mark.parametrize('compression', ['deflate', 'none'])
@pytest.mark.parametrize('method', ['nearest', 'mean'])
def test_every_level_equals_the_store(acquisition, stores, method, compression, capsys):
    st, folder = run(acquisition, '.ome.tiff', pyramid_method=method, z_projection='max', ome_tiff_layout='pyramid',
                     ome_tiff_compression=compression)
    out = capsys.readouterr().out
    for tag in ('', '_mip'):
        path = os.path.join(folder, f'R0_stitched{tag}.ome.tiff')
        want = stores(method)[tag]
        levels, xml = ometiff.read_pyramid_tiff(path)
        assert len(levels) == LEVELS
        _, nc, nz = want[0].shape[:3]
        assert (nc, nz) == ((2, 3) if tag == '' else (2, 1))
        for lv in range(LEVELS):
            assert want[lv].any() and len(levels[lv]) == nc * nz
            for c in range(nc):
                for z in range(nz):
                    assert np.array_equal(levels[lv][c * nz + z], want[lv][0, c, z]), (tag, lv, c, z)
        # structure
        buf, ifds = ometiff.read_pyramid_structure(path)
        assert len(ifds) == nc * nz
        zero = None
        for k, top in enumerate(ifds):
            assert (270 in top) == (k == 0) and len(top['sub']) == LEVELS - 1 and top[330][0] == 18
            for lv, t in enumerate([top] + top['sub']):
                assert _val(t, 254) == (1 if lv else 0)
                assert (_val(t, 257), _val(t, 256)) == want[lv].shape[3:]
                assert _val(t, 258) == 16 and _val(t, 259) == (8 if compression == 'deflate' else 1) and _val(t, 262) == 1
                assert _val(t, 277) == 1 and _val(t, 339) == 1 and (_val(t, 322), _val(t, 323)) == (TILE, TILE)
                assert (_val(t, 317) == 2) if compression == 'deflate' else (317 not in t)
                assert t[324][0] == t[325][0] == 16
                gy, gx = -(-want[lv].shape[3] // TILE), -(-want[lv].shape[4] // TILE)
                assert t[324][1] == t[325][1] == gy * gx
                plane = want[lv][0, k // nz, k % nz]
                for i in range(gy * gx):      # a tile of zeros points at the one zero tile, every other at bytes of its own
                    iy, ix = divmod(i, gx)
                    if not plane[iy * TILE:(iy + 1) * TILE, ix * TILE:(ix + 1) * TILE].any():
                        zero = zero or (int(t[324][2][i]), int(t[325][2][i]))
                        assert (int(t[324][2][i]), int(t[325][2][i])) == zero
        assert zero is None or zero[0] == 16
        if tag == '':
            assert zero is not None      # (the plane with the missing corner file)
        offsets = np.concatenate([t[324][2] for top in ifds for t in [top] + top['sub']])
        real = offsets[offsets != 16]
        assert len(set(real.tolist())) == len(real)
        # the OME-XML is the planes layout's
        name = 'R0_t0' + tag
        shape = (1, nc, nz) + want[0].shape[3:]
        assert xml == ometiff.ome_xml(shape, np.uint16, st.monochrome_channels, st.monochrome_colors, st.pixel_size_um, st._dz_um(), name)
        assert f'[ome-tiff] R0_stitched{tag}.ome.tiff: {LEVELS} levels, tiles {TILE} x {TILE}, ' in out


def test_the_pyramid_is_smaller_than_the_planes_with_deflate(acquisition):
    _, folder = run(acquisition, '.ome.tiff', ome_tiff_layout='pyramid')
    _, raw = run(acquisition, '.ome.tiff', ome_tiff_layout='pyramid', ome_tiff_compression='none')
    a, b = (os.path.getsize(os.path.join(f, 'R0_stitched.ome.tiff')) for f in (folder, raw))
    print(f'deflate {a} bytes, none {b} bytes')
    assert a < b


def test_composite_is_served_by_the_writer(acquisition):
    """--composite of the stack: the PNG of the pyramid TIFF run is the store run's."""
    pngs = []
    for fmt, kw in (('.ome.zarr', {}), ('.ome.tiff', dict(ome_tiff_layout='pyramid'))):
        _, folder = run(acquisition, fmt, composite=True, **kw)
        with open(os.path.join(folder, 'R0_stitched_composite.png'), 'rb') as fh:
            pngs.append(fh.read())
    assert pngs[0] == pngs[1] and len(pngs[0]) > 100


def test_edf_depth_and_their_composite_go_through_the_writer(acquisition):
    """--z-projection focus --focus-depth-map --composite: the _edf and _depth files hold the stores' levels (the depth's by
    nearest under either method), and the picture made from the projection is the store run's."""
    kw = dict(z_projection='focus', focus_depth_map=True, composite=True, pyramid_method='mean')
    _, zfolder = run(acquisition, '.ome.zarr', **kw)
    _, folder = run(acquisition, '.ome.tiff', ome_tiff_layout='pyramid', **kw)
    for tag in ('_edf', '_depth'):
        levels, _ = ometiff.read_pyramid_tiff(os.path.join(folder, f'R0_stitched{tag}.ome.tiff'))
        assert len(levels) == LEVELS
        for lv in range(LEVELS):
            want = omezarr.read_array(os.path.join(zfolder, f'R0_stitched{tag}.ome.zarr', str(lv)))
            assert want.any() and len(levels[lv]) == want.shape[1]
            for c in range(want.shape[1]):
                assert np.array_equal(levels[lv][c], want[0, c, 0]), (tag, lv, c)
    with open(os.path.join(folder, 'R0_stitched_edf_composite.png'), 'rb') as a, \
            open(os.path.join(zfolder, 'R0_stitched_edf_composite.png'), 'rb') as b:
        assert a.read() == b.read()


def test_the_planes_layout_is_unchanged(acquisition, tmp_path):
    """Without the flag: the file of write_ome_tiff of the fused region, byte for byte, and its XML the pyramid's."""
    st, folder = run(acquisition, '.ome.tiff')
    with open(os.path.join(folder, 'R0_stitched.ome.tiff'), 'rb') as fh:
        got = fh.read()
    region = st.stitch_region(0, 'R0')
    region = region.cpu().numpy() if hasattr(region, 'cpu') else np.asarray(region)
    path = str(tmp_path / 'want.ome.tiff')
    ometiff.write_ome_tiff(path, region, pixel_size_um=st.pixel_size_um, dz_um=st._dz_um(), channel_names=st.monochrome_channels,
                           channel_colors=st.monochrome_colors, name='R0_t0')
    with open(path, 'rb') as fh:
        assert fh.read() == got
    planes, xml = ometiff.read_ome_tiff(path)
    _, pfolder = run(acquisition, '.ome.tiff', ome_tiff_layout='pyramid')
    levels, pxml = ometiff.read_pyramid_tiff(os.path.join(pfolder, 'R0_stitched.ome.tiff'))
    assert pxml == xml
    assert all(np.array_equal(a, b) for a, b in zip(levels[0], planes)) and len(levels[0]) == len(planes) == 6


def test_one_writer_serves_regions_of_one_geometry(tmp_path):
    """Two wells: the second file goes through the first one's writer (retarget), and both are complete."""
    spec = dataclasses.replace(SPEC, regions=('A1', 'A2'), nz=1, missing=())
    root = str(tmp_path / 'acq')
    synth.write_acquisition(spec, root)
    _, folder = run(root, '.ome.tiff', ome_tiff_layout='pyramid')
    _, zfolder = run(root, '.ome.zarr')
    for region in ('A1', 'A2'):
        levels, _ = ometiff.read_pyramid_tiff(os.path.join(folder, f'{region}_stitched.ome.tiff'))
        for lv in range(LEVELS):
            want = omezarr.read_array(os.path.join(zfolder, f'{region}_stitched.ome.zarr', str(lv)))
            for c in range(2):
                assert np.array_equal(levels[lv][c], want[0, c, 0]), (region, lv, c)


# ---------------------------------------------------------------------------------------------------- the writer driven directly
W_SHAPE, W_LEVELS, W_BATCH, W_ZERO = (1, 7, 1, 333, 1201), 4, 3, 4
W_META = dict(pixel_size_um=0.5, dz_um=1.5, channel_names=[f'c{k}' for k in range(7)], channel_colors=[0x00FF00] * 7, name='w')
STALE = 0x5A


def _w_image(dtype):
    """Seven planes: cumulative sums of small differences (dynamic blocks under the predictor) and uniform noise (stored blocks)
    alternate; plane W_ZERO is all zero."""
    rng = np.random.default_rng(8)
    top = int(np.iinfo(dtype).max)
    img = rng.integers(0, top + 1, W_SHAPE).astype(dtype)
    img[0, 1::2] = np.cumsum(rng.integers(-40, 41, (3,) + W_SHAPE[2:]), axis=-1).astype(np.int64).astype(dtype)
    img[0, W_ZERO] = 0
    return img


@pytest.fixture(scope='module')
def w_cases():
    """{dtype name: (image, {method: its 4 levels})}: computed once, shared, left unchanged."""
    out = {}
    for dtype in ('uint16', 'uint8'):
        img = _w_image(dtype)
        out[dtype] = (img, {'nearest': O.pyramid_nearest(img, W_LEVELS), 'mean': mean_pyramid(img, W_LEVELS)})
        assert [lv.shape[3:] for lv in out[dtype][1]['mean']] == [(333, 1201), (166, 600), (83, 300), (41, 150)]
        assert not np.array_equal(out[dtype][1]['mean'][1], out[dtype][1]['nearest'][1])
    return out


def _drive(path, img, method, compression, tile):
    """3, 3 and 1 planes through the two slots of a writer whose device level buffers all held the stale pattern before."""
    import torch
    shapes = omezarr.level_shapes(img.shape, W_LEVELS)
    planes = torch.from_numpy(img.reshape((-1,) + img.shape[3:])).cuda()
    coords = [(0, c, 0) for c in range(W_SHAPE[1])]
    with ometiff.PyramidTiffWriter(path, shapes, img.dtype, meta=W_META, chunks=(1, 1, 1) + tuple(tile), batch=W_BATCH,
                                   compression=compression, device=planes.device, pyramid_method=method, verbose=False) as w:
        assert len(w._dev) == 2 and all(len(slot) == W_LEVELS for slot in w._dev)
        for slot in w._dev:
            for level in slot:
                level.view(torch.uint8).fill_(STALE)
        for b0 in range(0, len(coords), W_BATCH):
            m = min(W_BATCH, len(coords) - b0)
            w.acquire(m).copy_(planes[b0:b0 + m])
            w.submit(coords[b0:b0 + m])
        with pytest.raises(ValueError):
            w.acquire(W_BATCH + 1)
    return w


def _check_file(path, img, want, compression, tile):
    levels, xml = ometiff.read_pyramid_tiff(path)
    assert len(levels) == W_LEVELS
    assert xml == ometiff.ome_xml(img.shape, img.dtype, W_META['channel_names'], W_META['channel_colors'], 0.5, 1.5, 'w')
    for lv in range(W_LEVELS):
        assert len(levels[lv]) == W_SHAPE[1]
        for k in range(W_SHAPE[1]):
            assert np.array_equal(levels[lv][k], want[lv][0, k, 0]), (lv, k)
    _, ifds = ometiff.read_pyramid_structure(path)
    assert len(ifds) == W_SHAPE[1]
    zero_len = None
    for k, top in enumerate(ifds):
        for lv, t in enumerate([top] + top['sub']):
            assert (_val(t, 323), _val(t, 322)) == tuple(tile) and _val(t, 258) == 8 * img.dtype.itemsize
            assert _val(t, 259) == (8 if compression == 'deflate' else 1)
            gy, gx = -(-want[lv].shape[3] // tile[0]), -(-want[lv].shape[4] // tile[1])
            assert t[324][1] == t[325][1] == gy * gx
            if k == W_ZERO:      # every tile of the all-zero plane points at the one zero tile behind the header
                assert (t[324][2] == 16).all() and len(set(t[325][2].tolist())) == 1
                zero_len = int(t[325][2][0])
    real = np.concatenate([t[324][2] for top in ifds for t in [top] + top['sub']])
    real = real[real != 16]
    assert len(set(real.tolist())) == len(real) and real.min() >= 16 + zero_len


@pytest.fixture(scope='module')
def w_files(tmp_path_factory, w_cases):
    """The files of the multi-batch runs with 64 x 64 tiles, written once: (dtype, compression, method) -> (path, writer)."""
    folder, cache = tmp_path_factory.mktemp('writer'), {}

    def get(dtype, compression, method):
        key = (dtype, compression, method)
        if key not in cache:
            path = str(folder / f'{dtype}_{compression}_{method}.ome.tiff')
            cache[key] = (path, _drive(path, w_cases[dtype][0], method, compression, (64, 64)))
        return cache[key]
    return get


@pytest.mark.parametrize('method', ['nearest', 'mean'])
@pytest.mark.parametrize('compression', ['deflate', 'none'])
@pytest.mark.parametrize('dtype', ['uint16', 'uint8'])
def test_writer_multi_batch(w_cases, w_files, dtype, compression, method):
    """Three batches through two slots, the last one partly filled: every level of the file is the reference's, the all-zero plane
    costs no tile, and the planes behind the last batch's one plane -- stale planes of the first batch -- were encoded as zeros."""
    img, want = w_cases[dtype]
    path, w = w_files(dtype, compression, method)
    assert w.bytes_written == os.path.getsize(path)
    _check_file(path, img, want[method], compression, (64, 64))
    if compression == 'deflate':      # slot 0 took batches 0 and 2: its encoders' last offsets are batch 2's
        for enc in w._enc[0]:
            off = enc.offsets.cpu().numpy()
            per = enc.n_chunks // W_BATCH
            assert off[per] > 0 and (off[per:] == off[per]).all(), 'a plane behind the last batch has streams'
            assert int(enc.status.item()) == 0


@pytest.mark.parametrize('compression', ['deflate', 'none'])
@pytest.mark.parametrize('tile', [(512, 512), (16, 48)], ids=['default-512', 't16x48'])
def test_writer_tile_shapes(tmp_path, w_cases, tile, compression):
    """The default tile (levels 2 and 3 are smaller than one tile; a 512 x 512 uint16 tile is 32 segments) and a non-square one."""
    img, want = w_cases['uint16']
    if tile == (512, 512):
        assert all(s[0] < 512 and s[1] < 512 for s in [want['nearest'][lv].shape[3:] for lv in (2, 3)])
    path = str(tmp_path / 't.ome.tiff')
    _drive(path, img, 'nearest', compression, tile)
    _check_file(path, img, want['nearest'], compression, tile)


@pytest.mark.parametrize('dtype', ['uint16', 'uint8'])
def test_write_pyramid_tiff_from_numpy_and_from_the_device(tmp_path, w_cases, dtype):
    import torch
    img, want = w_cases[dtype]
    blobs = []
    for k, image in enumerate((img, torch.from_numpy(img).cuda())):
        path = ometiff.write_pyramid_tiff(str(tmp_path / f'w{k}.ome.tiff'), image, meta=W_META, num_levels=3,
                                          chunks=(1, 1, 1, 64, 64), pyramid_method='mean', verbose=False)
        with open(path, 'rb') as fh:
            blobs.append(fh.read())
    assert blobs[0] == blobs[1] and len(blobs[0]) > 1000
    levels, _ = ometiff.read_pyramid_tiff(path)
    assert len(levels) == 3
    for lv in range(3):
        for k in range(W_SHAPE[1]):
            assert np.array_equal(levels[lv][k], want['mean'][lv][0, k, 0]), (lv, k)


@pytest.mark.parametrize('compression', ['deflate', 'none'])
@pytest.mark.parametrize('dtype', ['uint16', 'uint8'])
def test_an_outside_reader_opens_the_files(w_cases, w_files, dtype, compression):
    """Pillow (libtiff) lists the top-level IFDs only: 7 frames, each level 0 of its plane."""
    pytest.importorskip('PIL')
    from PIL import Image
    img, _ = w_cases[dtype]
    path, _ = w_files(dtype, compression, 'nearest')
    with Image.open(path) as im:
        assert im.n_frames == W_SHAPE[1]
        for k in range(W_SHAPE[1]):
            im.seek(k)
            assert im.mode == ('I;16' if dtype == 'uint16' else 'L') and im.size == (W_SHAPE[4], W_SHAPE[3])
            assert np.array_equal(np.array(im), img[0, k, 0]), k


def test_uint8_rgb_acquisition_end_to_end(tmp_path):
    """uint8 RGB files (three colour planes and a fluorescence channel): the pyramid TIFF holds the store's voxels at every level."""
    root = str(tmp_path / 'acq')
    synth.write_acquisition(spec_of(load_case('coord_rgb')[0]), root)

    def go(fmt, **kw):
        st = Small(StitchingParameters(input_folder=root, output_format=fmt), **kw)
        st.run()
        return os.path.join(st.output_folder, '0_stitched')

    folder, zfolder = go('.ome.tiff', ome_tiff_layout='pyramid'), go('.ome.zarr')
    levels, _ = ometiff.read_pyramid_tiff(os.path.join(folder, 'R0_stitched.ome.tiff'))
    assert len(levels) == LEVELS
    for lv in range(LEVELS):
        want = omezarr.read_array(os.path.join(zfolder, 'R0_stitched.ome.zarr', str(lv)))
        assert want.dtype == np.uint8 and want.any() and want.shape[1] == 4 and want.shape[2] == 1
        assert len(levels[lv]) == 4 and levels[lv][0].dtype == np.uint8
        for c in range(4):
            assert np.array_equal(levels[lv][c], want[0, c, 0]), (lv, c)
