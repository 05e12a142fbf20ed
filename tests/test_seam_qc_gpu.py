"""--seam-qc on the device: sq_seam_stats against the numpy definition (tests/seam_qc_ref.py) word for word, and whole runs
whose CSV is the reference's table of the tile FILES at the run's rectangles, with the planted displacements recovered.  Every
comparison is equality."""
import dataclasses
import functools
import hashlib
import json
import os
import random

import numpy as np
import pytest

import despeckle_ref
import seam_qc_ref as R
import tophat_ref
from image_stitcher_amd import native, placement, seamqc, stitcher_cli, synth, tiffio
from image_stitcher_amd.ometiff import read_ome_tiff
from image_stitcher_amd.stitcher import Stitcher
from image_stitcher_amd.stitcher_parameters import StitchingParameters

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
H, W = 40, 72      # the kernel tests' tiles: a core of up to 40 rows spans two of the kernel's 32-row pieces


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to(DEV)


def _core(ref, mov, d, h, w, radius):
    """The record of tiles ``ref`` and ``mov`` at offset d = o_mov - o_ref: the overlap inset by the radius."""
    dy, dx = d
    hc, wc = h - abs(dy) - 2 * radius, w - abs(dx) - 2 * radius
    assert hc >= 1 and wc >= 1
    return [ref, mov, max(dy, 0) + radius, max(dx, 0) + radius, max(-dy, 0) + radius, max(-dx, 0) + radius, hc, wc]


def _records(radius, h=H, w=W):
    """Core widths of 1, 63, 64 and 65 and a core height of 1; negative dy and dx; the full overlap (more than 32 rows: two
    pieces); ref windows that end in the tile's last row and column, mov windows whose halo does; ref above mov in the list,
    below it, and the same tile."""
    r = radius
    recs = [_core(0, 1, (0, w - 2 * r - 1), h, w, r), _core(1, 2, (3, w - 2 * r - 63), h, w, r),
            _core(4, 3, (-5, -(w - 2 * r - 64)), h, w, r), _core(2, 5, (2, -(w - 2 * r - 65)), h, w, r),
            _core(0, 3, (h - 2 * r - 1, 0), h, w, r), _core(5, 0, (-(h - 2 * r - 1), -4), h, w, r), _core(1, 4, (0, 0), h, w, r),
            _core(3, 3, (1, -1), h, w, r),
            [2, 4, h - 7, w - 9, r, r, 7, 9],                          # the ref window ends in the last row and column
            [4, 1, 0, 0, h - r - 5, w - r - 6, 5, 6],                  # the mov window's halo does
            [5, 2, 0, 2, r, r, h - 2 * r, w - 2 * r - 2]]                # as tall as a mov window can be
    return np.array(recs, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _tiles(dtype, m=1, n=6, h=H, w=W):
    top = int(np.iinfo(np.dtype(dtype)).max)
    rng = np.random.default_rng(m * 1009 + n * 31 + h + w)
    out = rng.integers(0, top + 1, (m, n, h, w)).astype(dtype)
    out[0, n // 2, :, ::2] = top      # the largest products
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _reference(dtype, radius, m=1):
    ref = R.words_of(_tiles(dtype, m), _records(radius), radius)
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize('radius', [0, 1, 2, 3])
@pytest.mark.parametrize('dtype', ['uint8', 'uint16'])
def test_kernel_equals_the_definition(dtype, radius):
    import torch
    recs = _records(radius)
    assert {1, 63, 64, 65} <= set(recs[:, 7].tolist()) and 1 in recs[:, 6].tolist() and recs[:, 6].max() > 32
    tiles = _dev(_tiles(dtype))
    out = torch.full((1, len(recs), native.seam_words(radius)), -12345, dtype=torch.int64, device=DEV)      # garbage: overwritten
    got = native.seam_stats(tiles, recs, radius, out=out)
    assert got.data_ptr() == out.data_ptr()
    np.testing.assert_array_equal(got.cpu().numpy(), _reference(dtype, radius))
    fresh = native.seam_stats(tiles, recs.view(native.OVERLAP_DTYPE).reshape(-1), radius)      # records; out made by the wrapper
    assert fresh.dtype == torch.int64 and tuple(fresh.shape) == (1, len(recs), native.seam_words(radius))
    np.testing.assert_array_equal(fresh.cpu().numpy(), _reference(dtype, radius))


@pytest.mark.parametrize('dtype', ['uint8', 'uint16'])
def test_cores_wider_and_taller_than_a_piece(dtype):
    """The kernel cuts a core into pieces of 32 rows x 256 columns: widths of 255, 256, 257 and 513, heights of 32, 33, 64, 65."""
    h, w, radius = 72, 530, 2
    tiles = _tiles(dtype, 1, 2, h, w)
    recs = np.array([[0, 1, 2, 2, 2, 2, 32, 255], [0, 1, 3, 5, 2, 3, 33, 256], [1, 0, 0, 0, 4, 9, 64, 257],
                     [0, 1, 5, 11, 2, 2, 65, 513], _core(0, 1, (0, 0), h, w, radius)], dtype=np.int32)
    got = native.seam_stats(_dev(tiles), recs, radius)
    np.testing.assert_array_equal(got.cpu().numpy(), R.words_of(tiles, recs, radius))


@pytest.mark.parametrize('dtype', ['uint8', 'uint16'])
@pytest.mark.parametrize('m', [1, 3, 7])
def test_plane_counts(m, dtype):
    got = native.seam_stats(_dev(_tiles(dtype, m)), _records(2), 2)
    np.testing.assert_array_equal(got.cpu().numpy(), _reference(dtype, 2, m))


@pytest.mark.parametrize('dtype', ['uint8', 'uint16'])
def test_views_pitches_offsets_and_repeatability(dtype):
    import torch
    top = int(np.iinfo(np.dtype(dtype)).max)
    radius, m = 3, 3
    planes, want, recs = _tiles(dtype, m), _reference(dtype, 3, 3), _records(3)
    # rows of pitch W + 5 and tiles of H + 3 rows, the padding poisoned with the dtype's maximum; a base 1 row and 2 columns in
    padded = np.full((m, 6, H + 3, W + 5), top, planes.dtype)
    padded[:, :, 1:H + 1, 2:W + 2] = planes
    view = _dev(padded)[:, :, 1:H + 1, 2:W + 2]
    assert not view.is_contiguous() and view.data_ptr() != view.untyped_storage().data_ptr()
    np.testing.assert_array_equal(native.seam_stats(view, recs, radius).cpu().numpy(), want)
    # every other tile and every other plane of a larger stack
    big = np.full((2 * m, 12, H + 3, W + 5), top, planes.dtype)
    big[1::2, ::2, 1:H + 1, 2:W + 2] = planes
    view = _dev(big)[1::2, ::2, 1:H + 1, 2:W + 2]
    np.testing.assert_array_equal(native.seam_stats(view, recs, radius).cpu().numpy(), want)
    # the same call twice, into garbage: the same words
    out = torch.full((m, len(recs), native.seam_words(radius)), 2 ** 62, dtype=torch.int64, device=DEV)
    a = native.seam_stats(view, recs, radius, out=out).cpu().numpy().copy()
    b = native.seam_stats(view, recs, radius, out=out).cpu().numpy()
    assert a.tobytes() == b.tobytes() == want.tobytes()
    # a table uploaded once serves later calls
    table = native.seam_pairs_to_device(recs, DEV)
    np.testing.assert_array_equal(native.seam_stats(view, recs, radius, pairs_dev=table).cpu().numpy(), want)


def test_words_beyond_32_bits_do_not_wrap():
    """Two 1024 x 1024 tiles of 65535s at d = (0, 0), R = 1: n = 1022^2 and every sum of products is n * 65535^2, about 2^52; a
    32-bit partial sum anywhere in the kernel shows."""
    import torch
    tiles = torch.full((1, 2, 1024, 1024), 65535, dtype=torch.uint16, device=DEV)
    got = native.seam_stats(tiles, np.array([_core(0, 1, (0, 0), 1024, 1024, 1)]), 1).cpu().numpy()
    n = 1022 * 1022
    assert n * 65535 ** 2 > 2 ** 51
    assert got[0, 0].tolist() == [n * 65535, n * 65535 ** 2, 0] + [n * 65535, n * 65535 ** 2, n * 65535 ** 2] * 9


def test_four_tiles_of_2048_squared():
    """One plane of 2 x 2 tiles of 2048 x 2048 with 10 % overlap, R = 3: the four edge seams and the two corners."""
    rng = np.random.default_rng(77)
    tiles = rng.integers(0, 65536, (1, 4, 2048, 2048)).astype(np.uint16)
    tiles[0, 1, :, :300] = 65535
    step = 2048 - 205
    rects = {0: (0, 0, 2048, 2048, 0, 0), 1: (0, 0, 2048, 2048, 2, step), 2: (0, 0, 2048, 2048, step, -1),
             3: (0, 0, 2048, 2048, step + 1, step + 3)}
    seams = seamqc.region_seams(rects, 2048, 2048, 3, 256)
    assert len(seams) == 6
    recs = seamqc.pair_table(seams, {f: f for f in rects})
    got = native.seam_stats(_dev(tiles), recs, 3).cpu().numpy()
    np.testing.assert_array_equal(got, R.words_of(tiles, recs, 3))


def test_refusals():
    import torch
    tiles = _dev(_tiles('uint16'))
    recs = _records(2)
    out = torch.full((1, len(recs), native.seam_words(2)), 7, dtype=torch.int64, device=DEV)
    one = np.array([[0, 1, 3, 3, 3, 3, 10, 10]], dtype=np.int32)
    out1 = torch.full((1, 1, native.seam_words(2)), 7, dtype=torch.int64, device=DEV)
    for bad in ([[0, 6, 3, 3, 3, 3, 10, 10]], [[-1, 1, 3, 3, 3, 3, 10, 10]],          # a tile index out of range
                [[0, 1, 3, 3, 1, 3, 10, 10]], [[0, 1, 3, 3, 3, 1, 10, 10]],           # a mov window nearer than R to an edge
                [[0, 1, 3, 3, H - 11, 3, 10, 10]], [[0, 1, 3, 3, 3, W - 11, 10, 10]],
                [[0, 1, H - 9, 3, 3, 3, 10, 10]]):                                    # a ref window that leaves its tile
        with pytest.raises(native.NativeError):
            native.seam_stats(tiles, np.array(bad, dtype=np.int32), 2, out=out1)
    native.seam_stats(tiles, np.array([[0, 1, 3, 3, 1, 1, 10, 10]], dtype=np.int32), 1)      # (fine at R = 1)
    for radius in (4, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            native.seam_stats(tiles, one, radius)
    with pytest.raises(ValueError):
        native.seam_stats(tiles, recs, 2, out=out[:, :2])                                  # a wrong shape
    with pytest.raises(ValueError):
        native.seam_stats(tiles, recs, 3, out=out)                                         # the words of another radius
    with pytest.raises(ValueError):
        native.seam_stats(tiles, recs, 2, out=out.to(torch.int32))
    with pytest.raises(ValueError):
        native.seam_stats(tiles, recs, 2, out=torch.zeros(tuple(out.shape), dtype=torch.int64))      # another device
    with pytest.raises(ValueError):
        native.seam_stats(tiles.cpu(), recs, 2)                                            # a host tensor
    with pytest.raises(ValueError):
        native.seam_stats(tiles[0], recs, 2)                                               # not [m, n, H, W]
    with pytest.raises(ValueError):
        native.seam_stats(tiles.to(torch.float32), recs, 2)
    with pytest.raises(ValueError):
        native.seam_stats(tiles.permute(0, 1, 3, 2), recs, 2)                              # rows that are not contiguous
    with pytest.raises(ValueError):
        native.seam_stats(tiles, recs[:, :7], 2)
    with pytest.raises(ValueError):
        native.seam_stats(tiles, recs, 2, pairs_dev=native.seam_pairs_to_device(recs[:3], DEV))
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7).all() and (out1.cpu().numpy() == 7).all()      # nothing was launched
    # no pairs, no planes: fine
    empty = native.seam_stats(tiles, np.zeros((0, 8), dtype=np.int32), 2)
    assert tuple(empty.shape) == (1, 0, native.seam_words(2))
    assert tuple(native.seam_stats(tiles[:0], recs, 2).shape) == (0, len(recs), native.seam_words(2))
    np.testing.assert_array_equal(native.seam_stats(tiles, recs, 2, out=out).cpu().numpy(), _reference('uint16', 2))


# ---------------------------------------------------------------------------------------------------- whole runs
TRUTH = synth.GridSpec(rows=3, cols=4, tile_h=48, tile_w=64, ov_y=12, ov_x=16, jy=0, jx=0, tile_jitter_px=1, seed=5,
                       blank_fovs=(7,))
FIXTURE = synth.GridSpec(rows=3, cols=4, tile_h=64, tile_w=96, ov_y=8, ov_x=12, nz=3, channels=tuple(synth.DEFAULT_CHANNELS[:2]),
                         seed=5, blank_fovs=(7,))
RGB = synth.GridSpec(rows=2, cols=3, tile_h=64, tile_w=96, ov_y=8, ov_x=12, nz=2, dtype='uint8', seed=9,
                     channels=('BF LED matrix full_RGB', synth.DEFAULT_CHANNELS[1]), rgb_channels=('BF LED matrix full_RGB',))


def _tile_files(root):
    """[(path, fov, z, channel name)] of the acquisition's timepoint 0, named as the stitcher names them."""
    found = []
    for name in sorted(os.listdir(os.path.join(root, '0'))):
        if name.lower().endswith(('.tif', '.tiff')):
            parts = name.split('_', 3)
            channel = os.path.splitext(parts[3])[0].replace('_', ' ').replace('full ', 'full_')
            found.append((os.path.join(root, '0', name), int(parts[1]), int(parts[2]), channel))
    assert found
    return found


def _entries(root, transform=None):
    """([(fov, z, output channel, plane)] of the FILES, the output channel order); ``transform``: what is done to a file's image
    before its planes are taken."""
    entries, outputs = [], {}
    for path, fov, z, channel in _tile_files(root):
        img = tiffio.read_image(path)
        if transform is not None:
            img = transform(img)
        if img.ndim == 3 and img.shape[2] == 3:
            base = channel.split('_')[0]
            parts = [(f'{base}_{c}', img[:, :, i]) for i, c in enumerate('RGB')]
        else:
            parts = [(channel, img[0] if img.ndim == 3 else img)]
        outputs[channel] = [name for name, _ in parts]
        entries += [(fov, z, name, plane) for name, plane in parts]
    order = [name for channel in sorted(outputs) for name in outputs[channel]]
    return entries, order


def _prepared(root, params=None, **kw):
    st = Stitcher(StitchingParameters(input_folder=root, **(params or {})), normalization=None, **kw)
    st.get_timepoints()
    st.extract_acquisition_parameters()
    st.get_pixel_size()
    st.parse_acquisition_metadata()
    return st


def _rects(st):
    """{fov: rectangle} of region R0 at the stitcher's current placement."""
    st.calculate_output_dimensions(0, 'R0')      # (sets the grid positions the rectangles are counted from)
    return {int(key[2]): tuple(int(v) for v in st._tile_rect(info)) for key, info in st.get_region_data(0, 'R0').items()}


def _expected(root, rects, radius=2, min_pixels=256, min_ncc=0.5, transform=None, unmeasured=()):
    entries, order = _entries(root, transform)
    h, w = entries[0][3].shape
    return R.table_of(entries, order, rects, h, w, radius, min_pixels, min_ncc, unmeasured=unmeasured), order


def _run(root, *extra):
    random.seed(1234)
    stitcher_cli.main(['-i', root, '--normalization', 'none', *extra])
    base = os.path.dirname(root)
    outs = [d for d in os.listdir(base) if d.startswith(os.path.basename(root) + '_stitched_')]
    assert len(outs) == 1
    return os.path.join(base, outs[0], '0_stitched')


def _report(out):
    with open(os.path.join(out, 'R0_stitched_seam_qc.csv')) as fh:
        text = fh.read()
    with open(os.path.join(out, 'R0_stitched_seam_qc.json')) as fh:
        note = json.load(fh)
    assert text.endswith('\n')
    return text, [line.split(',') for line in text.splitlines()], note


def _qc_files(folder):
    return sorted(n for _, _, names in os.walk(folder) for n in names if '_seam_qc.' in n)


def _check_json(note, rows, order, radius, min_pixels, min_ncc):
    """The JSON agrees with the CSV."""
    head, body = rows[0], rows[1:]
    col = {k: i for i, k in enumerate(head)}
    assert note['rows'] == len(body)
    assert (note['settings']['seam_qc_radius'], note['settings']['seam_qc_min_pixels'], note['settings']['seam_qc_min_ncc']) == \
        (radius, min_pixels, min_ncc)
    flagged = [dict(channel=r[col['channel']], z_level=int(r[col['z_level']]), ref_fov=int(r[col['ref_fov']]),
                    mov_fov=int(r[col['mov_fov']]), flags=r[col['flags']]) for r in body if r[col['flags']]]
    assert note['flagged'] == flagged
    for f in seamqc.FLAGS:
        assert note['flag_counts'][f] == sum(1 for r in body if f in r[col['flags']].split('|'))
    assert list(note['median_ncc']) == order == list(note['best_histogram'])
    for name in order:
        good = [r for r in body if r[col['channel']] == name and r[col['ncc']] != '']
        for z in sorted({int(r[col['z_level']]) for r in body if r[col['channel']] == name}):
            ncc = [float(r[col['ncc']]) for r in good if int(r[col['z_level']]) == z]
            assert note['median_ncc'][name][str(z)] == (float(np.median(ncc)) if ncc else None)
        hist = {}
        for r in good:
            k = f"{r[col['best_dy']]},{r[col['best_dx']]}"
            hist[k] = hist.get(k, 0) + 1
        assert note['best_histogram'][name] == hist


def _truth(spec, rows):
    """{(ref_fov, mov_fov): (o_mov - o_ref of the scene) - (dy, dx) of the row}: the residual a seam should report."""
    col = {k: i for i, k in enumerate(rows[0])}
    want = {}
    for r in rows[1:]:
        f, g = int(r[col['ref_fov']]), int(r[col['mov_fov']])
        of, og = spec.origin(f // spec.cols, f % spec.cols), spec.origin(g // spec.cols, g % spec.cols)
        want[(f, g)] = (og[0] - of[0] - int(r[col['dy']]), og[1] - of[1] - int(r[col['dx']]))
    return want


def _best(rows):
    col = {k: i for i, k in enumerate(rows[0])}
    return {(int(r[col['ref_fov']]), int(r[col['mov_fov']]), int(r[col['z_level']]), r[col['channel']]):
            (r[col['best_dy']], r[col['best_dx']], r[col['flags']]) for r in rows[1:]}


@pytest.mark.parametrize('dtype', ['uint16', 'uint8'])
def test_coordinate_placement_reports_the_planted_jitter(tmp_path, dtype, capsys):
    spec = dataclasses.replace(TRUTH, dtype=dtype)
    root = str(tmp_path / 'acq')
    synth.write_acquisition(spec, root)
    out = _run(root, '--seam-qc', '--seam-qc-radius', '3', '--seam-qc-min-pixels', '300')
    assert _qc_files(out) == ['R0_stitched_seam_qc.csv', 'R0_stitched_seam_qc.json']
    text, rows, note = _report(out)
    want, order = _expected(root, _rects(_prepared(root)), 3, 300)
    assert rows == want
    _check_json(note, rows, order, 3, 300, 0.5)
    truth = _truth(spec, rows)
    assert len(truth) == 17      # the edge seams of a 3 x 4 grid; the corners have fewer than 300 pixels
    blank = 0
    for (f, g, z, ch), (by, bx, flags) in _best(rows).items():
        if 7 in (f, g):
            assert (by, bx, flags) == ('', '', 'featureless')
            blank += 1
        else:
            assert (int(by), int(bx)) == truth[(f, g)] and 'featureless' not in flags
            assert ('shifted' in flags) == (truth[(f, g)] != (0, 0))
    assert blank == 3 == note['flag_counts']['featureless']
    assert '[seam-qc] region R0 timepoint 0: 17 seams' in capsys.readouterr().out


def test_registered_placement_agrees_and_coordinate_placement_reports_the_drift(tmp_path):
    reg = dataclasses.replace(FIXTURE, nz=1)
    root = str(tmp_path / 'reg' / 'acq')
    synth.write_acquisition(reg, root)
    st = _prepared(root, dict(use_registration=True), seam_qc=True, seam_qc_radius=3, seam_qc_min_pixels=100)
    st.calculate_shifts(0, 'R0')
    st.stitch_region(0, 'R0')
    rows = [line.split(',') for line in seamqc.csv_text(st.seam_qc_table[(0, 'R0')]).splitlines()]
    want, _ = _expected(root, _rects(st), 3, 100)
    assert rows == want
    truth = _truth(reg, rows)
    textured = {k: v for k, v in _best(rows).items() if 7 not in k[:2]}
    assert len(textured) == 2 * 14 and all(truth[k[:2]] == (0, 0) for k in textured)      # the lattice is the scene's
    assert all((int(by), int(bx), flags) == (0, 0, '') for by, bx, flags in textured.values())
    # the same grid with a drift of (2, -1) per step, placed by its coordinates: every textured seam reports it
    drift = dataclasses.replace(FIXTURE, nz=1, jy=2, jx=-1)
    root = str(tmp_path / 'drift' / 'acq')
    synth.write_acquisition(drift, root)
    out = _run(root, '--seam-qc', '--seam-qc-radius', '3', '--seam-qc-min-pixels', '50')      # (a core of one row of 90 counts)
    _, rows, _ = _report(out)
    assert rows == _expected(root, _rects(_prepared(root)), 3, 50)[0]
    truth = _truth(drift, rows)
    textured = {k: v for k, v in _best(rows).items() if 7 not in k[:2]}
    assert len(textured) == 2 * 14
    for k, (by, bx, flags) in textured.items():
        want_e = truth[k[:2]]
        assert max(abs(want_e[0]), abs(want_e[1])) <= 3 and want_e != (0, 0)
        assert (int(by), int(bx)) == want_e and 'shifted' in flags.split('|')
    assert {truth[k[:2]][0] for k in textured if k[1] == k[0] + 1} == {2}       # side by side: the y drift per column step


def test_filters_come_first_and_the_flatfield_after(tmp_path):
    """The sums are taken of the planes the fusion reads: the table is the reference's on files despeckled and top-hatted
    beforehand, and the flatfield divide changes nothing in it."""
    spec = dataclasses.replace(FIXTURE, nz=1)
    roots = [str(tmp_path / k / 'acq') for k in ('filtered', 'flat')]
    for r in roots:
        synth.write_acquisition(spec, r)
    filters = ('--seam-qc', '--despeckle', 'both', '--background-subtract', 'tophat', '--background-radius', '5')
    a = _report(_run(roots[0], *filters))
    b = _report(_run(roots[1], *filters, '-ff'))
    assert a[0] == b[0] and a[2] == b[2]
    want, order = _expected(roots[0], _rects(_prepared(roots[0])),
                            transform=lambda img: tophat_ref.tophat_image(despeckle_ref.despeckle_image(img, 1000, 'both'), 5))
    assert a[1] == want and len(want) > 1
    _check_json(a[2], a[1], order, 2, 256, 0.5)
    assert want != _expected(roots[0], _rects(_prepared(roots[0])))[0]      # (the filters do change the planes)


def _hashes(out):
    """{relative path: digest} of everything a run wrote but the report itself."""
    found = {}
    for folder, _, names in os.walk(out):
        for name in names:
            if '_seam_qc.' not in name:
                with open(os.path.join(folder, name), 'rb') as fh:
                    found[os.path.relpath(os.path.join(folder, name), out)] = hashlib.sha256(fh.read()).hexdigest()
    return found


@pytest.mark.parametrize('extra', [(), ('-f', '.ome.tiff'), ('--z-projection', 'focus-only')], ids=['zarr', 'tiff', 'focus-only'])
def test_outputs_are_unchanged_and_default_writes_no_report(tmp_path, extra):
    roots = [str(tmp_path / k / 'acq') for k in ('with', 'without')]
    for r in roots:
        synth.write_acquisition(FIXTURE, r)
    with_qc, without = _run(roots[0], '--seam-qc', *extra), _run(roots[1], '--seam-qc-radius', '1', *extra)
    assert _qc_files(with_qc) == ['R0_stitched_seam_qc.csv', 'R0_stitched_seam_qc.json']
    assert _qc_files(str(tmp_path / 'without')) == []
    a, b = _hashes(with_qc), _hashes(without)
    if extra[:1] == ('-f',):      # (the OME-XML names no file of the run; compared plane by plane as well)
        for name in (n for n in os.listdir(without) if n.endswith('.ome.tiff')):
            pa, xa = read_ome_tiff(os.path.join(with_qc, name))
            pb, xb = read_ome_tiff(os.path.join(without, name))
            assert xa == xb
            np.testing.assert_array_equal(np.stack(pa), np.stack(pb))
    assert a and a == b
    want, _ = _expected(roots[0], _rects(_prepared(roots[0])))
    assert _report(with_qc)[1] == want and len(want) == 1 + 17 * 6


def test_row_bands_list_every_seam_once(tmp_path):
    """A row band stages whole tiles: the seams both bands reach are measured twice, give the same words and are listed once."""
    root = str(tmp_path / 'acq')
    synth.write_acquisition(FIXTURE, root)
    st = _prepared(root, seam_qc=True)
    st.chunks = (1, 1, 1, 64, 64)      # bands are whole chunk rows
    os.makedirs(os.path.join(st.output_folder, '0_stitched'), exist_ok=True)
    _, height = st.calculate_output_dimensions(0, 'R0')
    assert height > 128
    st.create_region_store(0, 'R0')
    for band in ((0, 128), (128, height)):
        st.stream_region_to_zarr(0, 'R0', create=False, row_band=band)
    rows = st.seam_qc_table[(0, 'R0')]
    assert len(rows) == 17 * 6 == len({(r['ref_fov'], r['mov_fov'], r['z_level'], r['channel']) for r in rows})
    want, _ = _expected(root, _rects(st))
    assert _report(os.path.join(st.output_folder, '0_stitched'))[1] == want      # the single call's table: the files'
    assert not st._seam_qc_pending and all('unmeasured' not in r['flags'] for r in rows)
    # without the option nothing is kept, allocated or written
    plain = _prepared(root)
    plain.stitch_region(0, 'R0')
    assert plain.seam_qc_table == {} and not plain._seam_qc_pending and plain._seam_qc_words == {} and plain._seam_qc_tables == {}
    assert _qc_files(plain.output_folder) == []


def test_a_band_edge_on_a_seam_line_leaves_its_seams_unmeasured(tmp_path):
    """Registered overwrite rectangles are cropped at the seam lines: with the band edge on the line between tile rows 0 and 1
    no call stages a tile of row 0 together with one of row 1."""
    spec = dataclasses.replace(FIXTURE, nz=1, jy=0, jx=0, channels=tuple(synth.DEFAULT_CHANNELS[:1]))
    root = str(tmp_path / 'acq')
    synth.write_acquisition(spec, root)
    st = _prepared(root, dict(use_registration=True), seam_qc=True, seam_qc_min_pixels=100)
    st.calculate_shifts(0, 'R0')
    rects = _rects(st)
    line = {rects[f][4] + rects[f][2] for f in range(4)}
    assert len(line) == 1 and {rects[f][4] for f in range(4, 8)} == line      # row 0 ends where row 1 begins
    line = line.pop()
    _, height = st.calculate_output_dimensions(0, 'R0')
    bands = ((0, line), (line, height))
    for band in bands:
        st.stitch_planes(0, 'R0', row_band=band)
    staged = [{f for f, r in rects.items() if placement.clip_rect_to_rows(r, *band) is not None} for band in bands]
    assert staged == [{0, 1, 2, 3}, set(range(4, 12))]
    rows = [line_.split(',') for line_ in seamqc.csv_text(st.seam_qc_table[(0, 'R0')]).splitlines()]
    split = {(f, f + 4) for f in range(4)}
    assert rows == _expected(root, rects, 2, 100, unmeasured=split)[0]
    col = {k: i for i, k in enumerate(rows[0])}
    assert {(int(r[col['ref_fov']]), int(r[col['mov_fov']])) for r in rows[1:] if 'unmeasured' in r[col['flags']]} == split
    assert len(rows) == 1 + 17


def test_rgb_files_give_three_planes_rows(tmp_path):
    root = str(tmp_path / 'acq')
    synth.write_acquisition(RGB, root)
    out = _run(root, '--seam-qc')
    _, rows, note = _report(out)
    want, order = _expected(root, _rects(_prepared(root)))
    assert rows == want
    assert order == ['BF LED matrix full_R', 'BF LED matrix full_G', 'BF LED matrix full_B', synth.DEFAULT_CHANNELS[1]]
    assert len(rows) == 1 + 7 * 2 * 4      # the seven edge seams of a 2 x 3 grid, two z levels, four output channels
    _check_json(note, rows, order, 2, 256, 0.5)
