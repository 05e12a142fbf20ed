"""--background-subtract tophat on the device: sq_tophat_tiles against the numpy definition (tests/tophat_ref.py), and whole
runs against runs on files that were filtered beforehand.  Every comparison is equality."""
import hashlib
import os
import random
import shutil

import numpy as np
import pytest

import tophat_ref
from helpers import flatfields_for, load_case, spec_of
from image_stitcher_amd import native, omezarr, synth, tiffio
from image_stitcher_amd.ometiff import read_ome_tiff
from image_stitcher_amd.stitcher import Stitcher
from image_stitcher_amd.stitcher_parameters import StitchingParameters
from image_stitcher_amd import stitcher_cli

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# (shape, radius).  The kernel's own sizes: strips of 256 columns up to R = 64 and of 128 above (and for planes up to 128
# wide), column segments of 2R+1, row segments of at least max(64, 4R) rows, blocks of up to 32 rows, three LDS sizes.
BIG_R = (1, 2, 7, 63, 64, 65, 127)
CASES = [((1, 1), 4), ((1, 300), 4), ((300, 1), 4), ((5, 7), 4), ((33, 31), 16), ((33, 31), 15)] + \
        [((257, 255), r) for r in BIG_R] + [((130, 1301), r) for r in BIG_R] + [((512, 640), 50)] + \
        [((6, 5), 2), ((70, 257), 4), ((70, 129), 65)]      # narrower than a vector; one column past a strip of 256 and of 128


def _dev(a):
    import torch
    return torch.from_numpy(a).to(DEV)


@pytest.mark.parametrize('dtype', ['uint8', 'uint16'])
@pytest.mark.parametrize('shape,radius', CASES)
def test_kernel_equals_the_definition(shape, radius, dtype):
    planes = tophat_ref.sample_planes(dtype, *shape)      # [3, 2, H, W]
    want = tophat_ref.tophat(planes, radius)
    got = native.tophat_tiles(_dev(planes), radius)
    np.testing.assert_array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize('dtype', ['uint8', 'uint16'])
def test_views_scratch_guard_and_repeatability(dtype):
    import torch
    h, w, radius = 70, 131, 9
    planes = tophat_ref.sample_planes(dtype, h, w).reshape(6, h, w)
    big = _dev(planes)
    view = big[::2]                                        # every other plane: plane stride 2 H W
    need = native.tophat_scratch_bytes(3, h, w, dtype)
    scratch = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    native.tophat_tiles(view, radius, scratch[:need])
    got = big.cpu().numpy()
    np.testing.assert_array_equal(got[::2], tophat_ref.tophat(planes[::2], radius))
    np.testing.assert_array_equal(got[1::2], planes[1::2])                       # the planes between: untouched
    assert bool((scratch[need:] == 0xA5).all())                                  # nothing past the scratch's declared size
    # rows with a pitch: the columns beyond the planes' width stay as they are
    wide = _dev(np.concatenate([planes, np.full((6, h, 5), 9, planes.dtype)], axis=2))
    native.tophat_tiles(wide[:, :, :w], radius)
    np.testing.assert_array_equal(wide.cpu().numpy()[:, :, :w], tophat_ref.tophat(planes, radius))
    assert (wide.cpu().numpy()[:, :, w:] == 9).all()
    # the same call twice on fresh copies: the same bytes
    a = native.tophat_tiles(_dev(planes), radius).cpu().numpy()
    b = native.tophat_tiles(_dev(planes), radius).cpu().numpy()
    assert a.tobytes() == b.tobytes()


def test_refusals():
    import torch
    t = torch.zeros((2, 8, 8), dtype=torch.uint16, device=DEV)
    for radius in (0, 128, -3, 1.5):
        with pytest.raises(ValueError):
            native.tophat_tiles(t, radius)
    with pytest.raises(ValueError):
        native.tophat_tiles(t.to(torch.float32), 3)
    with pytest.raises(ValueError):
        native.tophat_tiles(t, 3, scratch=torch.empty(16, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        native.tophat_tiles(t.permute(0, 2, 1), 3)          # rows that are not contiguous
    with pytest.raises(ValueError):
        native.tophat_tiles(t[:1].expand(3, 8, 8), 3)       # planes on top of each other
    with pytest.raises(ValueError):
        native.tophat_tiles(torch.zeros((2, 4, 8, 8), dtype=torch.uint16, device=DEV)[:, :3], 3)      # no uniform plane stride
    assert not t.cpu().numpy().any()      # nothing was launched


# ---------------------------------------------------------------------------------------------------- whole runs
def _filter_files(root, radius):
    """Every tile file of the acquisition replaced by its top-hat (what a user did before handing the files over)."""
    n = 0
    for folder, _, names in os.walk(root):
        for name in names:
            if name.lower().endswith(('.tif', '.tiff')):
                path = os.path.join(folder, name)
                tiffio.write_tiff(path, tophat_ref.tophat_image(tiffio.read_image(path), radius))
                n += 1
    assert n > 0


def _run(root, *extra):
    random.seed(1234)
    stitcher_cli.main(['-i', root, '--normalization', 'none', *extra])
    base = os.path.dirname(root)
    outs = [d for d in os.listdir(base) if d.startswith(os.path.basename(root) + '_stitched_')]
    assert len(outs) == 1
    return os.path.join(base, outs[0], '0_stitched')


def _hashes(out):
    """{relative path: digest} of every file of the stores (chunks and metadata), the histogram sidecars and the pictures."""
    found = {}
    for folder, _, names in os.walk(out):
        for name in names:
            rel = os.path.relpath(os.path.join(folder, name), out)
            if '.ome.zarr' in rel or rel.endswith(('_histogram.npy', '_stats.json', '.png')):
                with open(os.path.join(folder, name), 'rb') as fh:
                    found[rel] = hashlib.sha256(fh.read()).hexdigest()
    return found


def _pair(tmp_path, spec):
    roots = [str(tmp_path / k / 'acq') for k in ('raw', 'filtered')]
    for r in roots:
        synth.write_acquisition(spec, r)
    return roots


U8_SPEC = dict(rows=2, cols=3, tile_h=72, tile_w=100, ov_y=11, ov_x=17, nz=2, dtype='uint8',
               channels=tuple(synth.DEFAULT_CHANNELS[:2]), seed=21)


@pytest.mark.parametrize('case', ['coord_3x4_small', 'coord_rgb', 'uint8'])
def test_run_equals_a_run_on_filtered_files(tmp_path, case):
    spec = synth.GridSpec(**U8_SPEC) if case == 'uint8' else spec_of(load_case(case)[0])
    raw, filtered = _pair(tmp_path, spec)
    _filter_files(filtered, 5)
    got = _run(raw, '--background-subtract', 'tophat', '--background-radius', '5')
    want = _run(filtered)
    a, b = _hashes(got), _hashes(want)
    assert a and a == b
    assert any(not os.path.basename(k).startswith('.') for k in a)      # chunk files were compared
    note = [n for n in os.listdir(got) if n.endswith('_stitched_background.json')]
    assert note and not [n for n in os.listdir(want) if n.endswith('_background.json')]
    import json
    with open(os.path.join(got, note[0])) as fh:
        meta = json.load(fh)
    assert meta['method'] == 'tophat' and meta['radius'] == 5
    level0 = omezarr.read_array(os.path.join(got, sorted(d for d in os.listdir(got) if d.endswith('.ome.zarr'))[0], '0'))
    assert level0.any()


def test_run_with_projection_windows_composite_and_mean_pyramid(tmp_path):
    spec = synth.GridSpec(rows=2, cols=3, tile_h=96, tile_w=128, ov_y=17, ov_x=23, nz=3,
                          channels=tuple(synth.DEFAULT_CHANNELS[:2]), seed=11)
    raw, filtered = _pair(tmp_path, spec)
    _filter_files(filtered, 5)
    extra = ('--z-projection', 'focus', '--contrast-limits', 'percentile', '--composite', '--pyramid-method', 'mean')
    a = _hashes(_run(raw, '--background-subtract', 'tophat', '--background-radius', '5', *extra))
    b = _hashes(_run(filtered, *extra))
    assert a == b
    assert any('_edf.ome.zarr' in k for k in a) and any(k.endswith('.png') for k in a) and any(k.endswith('_histogram.npy') for k in a)


def test_run_to_ome_tiff(tmp_path):
    spec = spec_of(load_case('coord_3x4_small')[0])
    raw, filtered = _pair(tmp_path, spec)
    _filter_files(filtered, 5)
    got = _run(raw, '--background-subtract', 'tophat', '--background-radius', '5', '-f', '.ome.tiff')
    want = _run(filtered, '-f', '.ome.tiff')
    names = sorted(n for n in os.listdir(want) if n.endswith('.ome.tiff'))
    assert names and names == sorted(n for n in os.listdir(got) if n.endswith('.ome.tiff'))
    for n in names:
        pa, xa = read_ome_tiff(os.path.join(got, n))
        pb, xb = read_ome_tiff(os.path.join(want, n))
        assert xa == xb
        np.testing.assert_array_equal(np.stack(pa), np.stack(pb))


def test_default_is_untouched(tmp_path):
    spec = spec_of(load_case('coord_3x4_small')[0])
    a, b = _pair(tmp_path, spec)
    ha, hb = _hashes(_run(a, '--background-subtract', 'none', '--background-radius', '9')), _hashes(_run(b))
    assert ha and ha == hb


def _prepared(root, info, **kw):
    p = info['params']
    params = StitchingParameters(input_folder=root, use_registration=p['use_registration'], apply_flatfield=p['apply_flatfield'],
                                 registration_channel=p['registration_channel'], registration_z_level=p['registration_z_level'],
                                 scan_pattern=info['spec']['scan_pattern'])
    st = Stitcher(params, normalization=None, **kw)
    st.get_timepoints()
    st.extract_acquisition_parameters()
    st.get_pixel_size()
    st.parse_acquisition_metadata()
    flats = flatfields_for(info, st.num_c)
    if flats:
        st.flatfields = flats
    return st


def test_with_flatfield(tmp_path):
    """The filter runs on the raw tile, before the divide: clip((I - O) / flat)."""
    info, _ = load_case('coord_ff32')
    assert info['params']['apply_flatfield']
    raw, filtered = _pair(tmp_path, spec_of(info))
    _filter_files(filtered, 6)
    got = _prepared(raw, info, background_subtract='tophat', background_radius=6).stitch_region(0, 'R0')
    want = _prepared(filtered, info).stitch_region(0, 'R0')
    np.testing.assert_array_equal(got, want)
    assert got.any() and not np.array_equal(got, _prepared(raw, info).stitch_region(0, 'R0'))


def test_with_registration(tmp_path):
    """Registration reads raw tiles: the same shifts with and without the option; level 0 is the oracle's fusion of
    reference-filtered tiles at those shifts."""
    from oracle import stitch_oracle as O
    info, _ = load_case('reg_3x4_small')
    root = str(tmp_path / 'acq')
    synth.write_acquisition(spec_of(info), root)
    plain = _prepared(root, info)
    plain.calculate_shifts(0, 'R0')
    st = _prepared(root, info, background_subtract='tophat', background_radius=4)
    st.calculate_shifts(0, 'R0')
    assert (tuple(st.h_shift), tuple(st.v_shift)) == (tuple(plain.h_shift), tuple(plain.v_shift))
    assert list(st.h_shift) == info['h_shift'] and list(st.v_shift) == info['v_shift']
    acq = O.parse_acquisition(root, tiffio.read_image)
    want = O.stitch_region(acq, 0, 'R0', lambda p: tophat_ref.tophat_image(tiffio.read_image(p), 4), True,
                           dict(h_shift=tuple(st.h_shift), v_shift=tuple(st.v_shift)))
    np.testing.assert_array_equal(st.stitch_region(0, 'R0'), want)


def test_row_bands(tmp_path):
    """A row band stages whole tiles, so two bands give the store of one whole call."""
    info, _ = load_case('coord_3x4_small')
    roots = _pair(tmp_path, spec_of(info))
    stores = []
    for k, root in enumerate(roots):
        st = _prepared(root, info, background_subtract='tophat', background_radius=5)
        st.chunks = (1, 1, 1, 64, 64)      # bands are whole chunk rows: (0, 128) and (128, 240) of the 240-row canvas
        os.makedirs(os.path.join(st.output_folder, '0_stitched'), exist_ok=True)
        if k == 0:
            stores.append(st.stream_region_to_zarr(0, 'R0'))
        else:
            _, height = st.calculate_output_dimensions(0, 'R0')
            assert height > 128
            st.create_region_store(0, 'R0')
            for band in ((0, 128), (128, height)):
                stores[1:] = [st.stream_region_to_zarr(0, 'R0', create=False, row_band=band)]
    a, b = (omezarr.read_array(os.path.join(s, '0')) for s in stores)
    np.testing.assert_array_equal(a, b)
    want = _prepared(roots[0], info).stitch_region(0, 'R0')
    assert a.any() and not np.array_equal(a, want)
