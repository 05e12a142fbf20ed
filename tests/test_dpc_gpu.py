"""--dpc on the device: sq_dpc_tiles against the numpy definition (tests/dpc_ref.py), and whole runs against runs without the
option on a folder that also holds the DPC files made beforehand.  Every comparison is equality."""
import functools
import hashlib
import json
import os
import random

import numpy as np
import pytest

import dpc_ref
from image_stitcher_amd import native, omezarr, synth
from image_stitcher_amd.ometiff import read_ome_tiff
from image_stitcher_amd.stitcher import Stitcher
from image_stitcher_amd.stitcher_parameters import StitchingParameters
from image_stitcher_amd import stitcher_cli

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LEFT, RIGHT, FLUO = 'BF LED matrix left half', 'BF LED matrix right half', 'Fluorescence 488 nm Ex'

# The kernel's own sizes: a thread owns one 16-byte vector of columns (8 uint16 / 16 uint8) and walks down 8 rows; a workgroup is
# tx vectors wide (a power of two up to 256: strips of 2048 uint16 / 4096 uint8 columns) and 256 / tx runs of 8 rows tall.
#   (65, 17)    tx = 4 (uint16) / 2 (uint8): many runs of rows in one workgroup, one row past a run
#   (33, 2049)  uint16: one column past a strip; (3, 4100): uint8: four columns past a strip, uint16: three strips
SHAPES = [(1, 1), (1, 300), (300, 1), (3, 5), (33, 31), (257, 255), (65, 17), (33, 2049), (3, 4100)]
GAINS = (1, 3, 16)
N_PLANES = 5
LAYOUTS = ('dense', 'pitched', 'offset', 'in_place')


@functools.lru_cache(maxsize=None)
def _planes(dtype, h, w):
    """(left, right) [5, H, W]: uniform random full-range values, the planted pixels in the first and last row and column."""
    dt = np.dtype(dtype)
    top = int(np.iinfo(dt).max)
    rng = np.random.default_rng(h * 10007 + w + top)
    left = rng.integers(0, top + 1, (N_PLANES, h, w)).astype(dt)
    right = rng.integers(0, top + 1, (N_PLANES, h, w)).astype(dt)
    pl, pr = dpc_ref.planted(dtype)
    for a, p in ((left, pl), (right, pr)):
        a[:, 0, :] = np.resize(p, w)
        a[:, -1, :] = np.resize(p[::-1], w)
        a[:, :, 0] = np.resize(np.roll(p, 3), h)
        a[:, :, -1] = np.resize(np.roll(p, 7), h)
    left.setflags(write=False)
    right.setflags(write=False)
    return left, right


@functools.lru_cache(maxsize=None)
def _reference(dtype, h, w, gain):
    out = dpc_ref.dpc_image(*_planes(dtype, h, w), gain)
    out.setflags(write=False)
    return out


def _buffer(n, h, w, pitch, offset, fill, dtype):
    """A flat device buffer of ``fill`` and its view [n, h, w]: rows ``pitch`` apart, planes one row more than a plane apart,
    the first element ``offset`` elements into the allocation."""
    import torch
    rows = h + 1
    flat = torch.from_numpy(np.full(offset + n * rows * pitch + 8, fill, dtype=np.dtype(dtype))).to(DEV)
    view = flat[offset:offset + n * rows * pitch].view(n, rows, pitch)[:, :h, :w]
    return flat, view


def _outside(flat, n, h, w, pitch, offset):
    """The elements of a ``_buffer`` that its view does not cover."""
    host = flat.cpu().numpy()
    mask = np.ones(host.shape, dtype=bool)
    body = mask[offset:offset + n * (h + 1) * pitch].reshape(n, h + 1, pitch)
    body[:, :h, :w] = False
    return host[mask]


@pytest.mark.parametrize('dtype', ['uint8', 'uint16'])
@pytest.mark.parametrize('shape', SHAPES)
def test_kernel_equals_the_definition(shape, dtype):
    import torch
    h, w = shape
    left_np, right_np = _planes(dtype, h, w)
    guard = int(np.iinfo(np.dtype(dtype)).max) // 3
    for layout in LAYOUTS:
        lp, rp, op = (w + 3, w + 5, w + 7) if layout == 'pitched' else (w, w, w)
        off = 1 if layout == 'offset' else 0
        for n in (0, 1, N_PLANES):
            for gain in GAINS:
                lflat, left = _buffer(n, h, w, lp, off, guard, dtype)
                rflat, right = _buffer(n, h, w, rp, off, guard, dtype)
                left.copy_(torch.from_numpy(left_np[:n].copy()))
                right.copy_(torch.from_numpy(right_np[:n].copy()))
                if layout == 'in_place':
                    oflat, out, opitch = lflat, left, lp
                    got = native.dpc_tiles(left, right, gain)
                    assert got is left
                else:
                    oflat, out = _buffer(n, h, w, op, off, guard, dtype)
                    opitch = op
                    got = native.dpc_tiles(left, right, gain, out=out)
                    assert got is out
                    np.testing.assert_array_equal(left.cpu().numpy(), left_np[:n])      # the inputs are left as they were
                if layout == 'offset' and n:
                    assert all(t.data_ptr() % 16 for t in (left, right, out))
                np.testing.assert_array_equal(right.cpu().numpy(), right_np[:n])
                np.testing.assert_array_equal(out.cpu().numpy(), _reference(dtype, h, w, gain)[:n])
                # pitch columns, stride rows and the elements around the planes: as they were
                assert (_outside(oflat, n, h, w, opitch, off) == guard).all()
                assert (_outside(rflat, n, h, w, rp, off) == guard).all()


@pytest.mark.parametrize('dtype', ['uint8', 'uint16'])
def test_repeatability_views_and_refusals(dtype):
    import torch
    h, w, gain = 70, 131, 3
    left_np, right_np = _planes(dtype, h, w)
    want = _reference(dtype, h, w, gain)
    dev = lambda a: torch.from_numpy(np.array(a)).to(DEV)
    # two launches: the same bytes
    runs = [native.dpc_tiles(dev(left_np), dev(right_np), gain).cpu().numpy().tobytes() for _ in range(2)]
    assert runs[0] == runs[1] == want.tobytes()
    # every other plane of a stack as left, a 4-D stack as all three
    big = dev(np.repeat(left_np, 2, axis=0))
    out = native.dpc_tiles(big[::2], dev(right_np), gain, out=dev(np.zeros((N_PLANES, h, w), dtype=left_np.dtype)))
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    four = native.dpc_tiles(dev(left_np[:4].reshape(2, 2, h, w)), dev(right_np[:4].reshape(2, 2, h, w)), gain)
    np.testing.assert_array_equal(four.cpu().numpy().reshape(4, h, w), want[:4])
    # the wrapper's refusals: nothing is launched
    left, right = dev(left_np), dev(right_np)
    for bad in (0, 17, -1, 1.5, True, None):
        with pytest.raises(ValueError):
            native.dpc_tiles(left, right, bad)
    with pytest.raises(ValueError):
        native.dpc_tiles(left, right[:2])                                      # another shape
    with pytest.raises(ValueError):
        native.dpc_tiles(left, right.to(torch.float32))                        # another dtype
    with pytest.raises(ValueError):
        native.dpc_tiles(left.to(torch.float32), right.to(torch.float32))
    with pytest.raises(ValueError):
        native.dpc_tiles(left, right.cpu())                                    # another device
    with pytest.raises(ValueError):
        native.dpc_tiles(left.permute(0, 2, 1), right.permute(0, 2, 1))        # rows that are not contiguous
    with pytest.raises(ValueError):
        native.dpc_tiles(left[:4], right[:4], out=left[1:])                    # out overlaps left without being left
    with pytest.raises(ValueError):
        native.dpc_tiles(left, right, out=right)                               # out is right
    with pytest.raises(ValueError):
        native.dpc_tiles(left[:4], right[:4], out=right[1:])
    with pytest.raises(ValueError):
        native.dpc_tiles(left[:4], left[1:])                                   # in place with a right that overlaps it
    # the library itself refuses a partial overlap, and leaves out untouched
    es = left.element_size()
    args = (N_PLANES - 1, h, w, h * w, w, h * w, w, h * w, w, native.sq_dtype_of(np.dtype(dtype)), gain, None)
    L = native.lib()
    for out_ptr in (left.data_ptr() + w * es, left.data_ptr() + h * w * es, right.data_ptr() + es, right.data_ptr()):
        assert L.sq_dpc_tiles(left.data_ptr(), right.data_ptr(), out_ptr, *args) == -1      # SQ_ERR_INVALID
    assert L.sq_dpc_tiles(left.data_ptr(), right.data_ptr(), left.data_ptr(), N_PLANES - 1, h, w, h * w, w + 1, h * w, w,
                          h * w, w, native.sq_dtype_of(np.dtype(dtype)), gain, None) == -1  # the same base, another pitch
    torch.cuda.synchronize()
    np.testing.assert_array_equal(left.cpu().numpy(), left_np)
    np.testing.assert_array_equal(right.cpu().numpy(), right_np)


# ---------------------------------------------------------------------------------------------------- whole runs
SPEC16 = dict(rows=2, cols=3, tile_h=72, tile_w=100, ov_y=11, ov_x=17, nz=2, channels=(LEFT, RIGHT, FLUO), seed=21)
SPEC8 = dict(SPEC16, dtype='uint8')


def _run(root, *extra):
    random.seed(1234)
    stitcher_cli.main(['-i', root, '--normalization', 'none', *extra])
    base = os.path.dirname(root)
    outs = [d for d in os.listdir(base) if d.startswith(os.path.basename(root) + '_stitched_')]
    assert len(outs) == 1
    return os.path.join(base, outs[0], '0_stitched')


def _notes(out):
    return sorted(n for n in os.listdir(out) if n.endswith('_stitched_dpc.json')) if os.path.isdir(out) else []


def _hashes(out):
    """{relative path: digest} of every file a run wrote for the timepoint -- stores, sidecars, reports, pictures -- but the
    note of the option itself."""
    found = {}
    for folder, _, names in os.walk(out):
        for name in names:
            if not name.endswith('_stitched_dpc.json'):
                with open(os.path.join(folder, name), 'rb') as fh:
                    found[os.path.relpath(os.path.join(folder, name), out)] = hashlib.sha256(fh.read()).hexdigest()
    return found


def _roots(tmp_path, spec, gain=1, kinds=('raw', 'with_files', 'plain')):
    roots = [str(tmp_path / k / 'acq') for k in kinds]
    for r in roots:
        synth.write_acquisition(spec, r)
    pairs = spec.rows * spec.cols * spec.nz - sum(1 for m in spec.missing if m[2] in (0, 1))
    assert dpc_ref.write_dpc_files(roots[1], LEFT, RIGHT, gain) == pairs
    return roots


def _three_runs(tmp_path, spec, extra=(), dpc_extra=(), gain=1, with_plain=True):
    """(hashes of the run with --dpc, of the same run without it on the folder that holds the DPC files, of the same run
    without it on the original -- None where ``extra`` names the derived channel, which the original lacks); the note exists
    only in the first."""
    raw, with_files, plain = _roots(tmp_path, spec, gain)
    got = _run(raw, '--dpc', *dpc_extra, *extra)
    want = _run(with_files, *extra)
    unchanged = _run(plain, *extra) if with_plain else None
    assert _notes(got) == ['R0_stitched_dpc.json'] and not _notes(want) and not (with_plain and _notes(unchanged))
    with open(os.path.join(got, 'R0_stitched_dpc.json')) as fh:
        note = json.load(fh)
    assert note == {'left': LEFT, 'right': RIGHT, 'gain': gain, 'channel': 'DPC', 'definition': native.DPC_DEFINITION}
    assert 'floor' in note['definition'] and '\n' not in note['definition']
    return _hashes(got), _hashes(want), _hashes(unchanged) if with_plain else None


def test_run_equals_a_run_on_a_folder_with_the_dpc_files(tmp_path):
    a, b, c = _three_runs(tmp_path, synth.GridSpec(**SPEC16), ('-r',))
    assert a and a == b and a != c
    assert any('.ome.zarr' in k and not os.path.basename(k).startswith('.') for k in a)      # chunk files were compared
    # the clamps are exercised: about 1 % of the tile pixels in each at gain 1
    spec = synth.GridSpec(**SPEC16)
    d = dpc_ref.dpc_image(spec.tile(0, 0, ch=0), spec.tile(0, 0, ch=1), 1)
    assert (d == 0).any() and (d == 65535).any() and ((d > 0) & (d < 65535)).mean() > 0.9


def test_run_uint8_with_gain(tmp_path):
    a, b, c = _three_runs(tmp_path, synth.GridSpec(**SPEC8), ('-r',), ('--dpc-gain', '4'), gain=4)
    assert a and a == b and a != c


def test_run_with_guided_focus_windows_composite_report_and_despeckle(tmp_path):
    extra = ('--z-projection', 'focus', '--focus-guide-channel', 'DPC', '--focus-depth-map',
             '--contrast-limits', 'percentile', '--composite', '--pyramid-method', 'mean',
             '--tile-qc', '--despeckle', 'both', '--despeckle-threshold', '40')
    a, b, _ = _three_runs(tmp_path, synth.GridSpec(**SPEC16), extra, with_plain=False)
    assert a and a == b
    for part in ('_edf.ome.zarr', '_depth.ome.zarr', '_tile_qc.csv', '_tile_qc.json', '_histogram.npy', '_stats.json', '.png',
                 '_despeckle.json'):
        assert any(part in k for k in a), part


def test_run_with_feather_fusion(tmp_path):
    a, b, c = _three_runs(tmp_path, synth.GridSpec(**SPEC16), ('--fusion-mode', 'feather'))
    assert a and a == b and a != c


def test_run_to_ome_tiff(tmp_path):
    raw, with_files, plain = _roots(tmp_path, synth.GridSpec(**SPEC16))
    got = _run(raw, '--dpc', '-f', '.ome.tiff')
    want = _run(with_files, '-f', '.ome.tiff')
    unchanged = _run(plain, '-f', '.ome.tiff')
    assert _notes(got) and not _notes(want) and not _notes(unchanged)
    names = sorted(n for n in os.listdir(want) if n.endswith('.ome.tiff'))
    assert names and names == sorted(n for n in os.listdir(got) if n.endswith('.ome.tiff'))
    for n in names:
        pa, xa = read_ome_tiff(os.path.join(got, n))
        pb, xb = read_ome_tiff(os.path.join(want, n))
        pc, xc = read_ome_tiff(os.path.join(unchanged, n))
        assert xa == xb and xa != xc and 'DPC' in xa
        np.testing.assert_array_equal(np.stack(pa), np.stack(pb))
        assert len(pa) == len(pc) + 2      # one more channel of two z planes


def test_run_with_a_missing_right_file(tmp_path):
    spec = synth.GridSpec(**SPEC16, missing=((4, 1, 1, 0),))      # fov 4, z 1, the right half: no DPC tile there
    a, b, c = _three_runs(tmp_path, spec)
    assert a and a == b and a != c


def _level0(out):
    stores = [n for n in os.listdir(out) if n.endswith('_stitched.ome.zarr')]
    assert len(stores) == 1
    return omezarr.read_array(os.path.join(out, stores[0], '0'))


def test_flatfield_leaves_the_derived_channel_alone(tmp_path):
    """-ff: the derived channel is fused without a gain, and the file channels get the gains of a run without the option."""
    spec = synth.GridSpec(**SPEC16)
    roots = [str(tmp_path / k / 'acq') for k in ('both', 'dpc', 'ff')]
    for r in roots:
        synth.write_acquisition(spec, r)
    ff = ('-ff', '--flatfield-estimator', 'mean')
    both, dpc, flat = _level0(_run(roots[0], '--dpc', *ff)), _level0(_run(roots[1], '--dpc')), _level0(_run(roots[2], *ff))
    assert both.shape[1] == dpc.shape[1] == 4 and flat.shape[1] == 3      # (t, c, z, y, x); DPC sorts third
    np.testing.assert_array_equal(both[:, 2], dpc[:, 2])
    np.testing.assert_array_equal(both[:, [0, 1, 3]], flat)
    assert not np.array_equal(both[:, [0, 1, 3]], dpc[:, [0, 1, 3]])      # (the gains do change the file channels)
    with open(os.path.join(os.path.dirname(_run_folder(roots[0])), 'flatfield_info.json')) as fh:
        assert set(json.load(fh)['channels']) == {LEFT, RIGHT, FLUO}


def _run_folder(root):
    base = os.path.dirname(root)
    outs = [d for d in os.listdir(base) if d.startswith(os.path.basename(root) + '_stitched_')]
    assert len(outs) == 1
    return os.path.join(base, outs[0], '0_stitched')


def test_only_planes_and_row_band(tmp_path):
    root = str(tmp_path / 'acq')
    synth.write_acquisition(synth.GridSpec(**SPEC16), root)
    st = Stitcher(StitchingParameters(input_folder=root), normalization=None, dpc=True)
    st.get_timepoints()
    st.extract_acquisition_parameters()
    st.get_pixel_size()
    st.parse_acquisition_metadata()
    c = st.monochrome_channels.index('DPC')
    derived = [c * st.num_z + z for z in range(st.num_z)]
    full, ids = st.stitch_planes(0, 'R0')
    full = full.cpu().numpy()
    assert ids == list(range(st.num_c * st.num_z)) and full[derived].any()
    _, height = st.calculate_output_dimensions(0, 'R0')
    y0, y1 = 37, height - 20
    band, band_ids = st.stitch_planes(0, 'R0', only_planes=derived, row_band=(y0, y1))
    assert band_ids == derived
    np.testing.assert_array_equal(band.cpu().numpy(), full[derived][:, y0:y1])
    # the derived planes are the definition applied to the fused halves wherever one tile alone covers a pixel: the top-left
    # tile's own corner
    l = st.monochrome_channels.index(LEFT) * st.num_z
    r = st.monochrome_channels.index(RIGHT) * st.num_z
    np.testing.assert_array_equal(full[derived[0], :40, :60], dpc_ref.dpc_image(full[l, :40, :60], full[r, :40, :60], 1))
    assert [k for k in st._buffer_cache if k[0] == 'dpc']
    plain = Stitcher(StitchingParameters(input_folder=root), normalization=None)
    plain.get_timepoints()
    plain.extract_acquisition_parameters()
    plain.get_pixel_size()
    plain.parse_acquisition_metadata()
    plain.stitch_planes(0, 'R0')
    assert plain._buffer_cache and not [k for k in plain._buffer_cache if k[0] == 'dpc']      # off: nothing is allocated
    assert not _notes(os.path.join(plain.output_folder, '0_stitched')) and _notes(os.path.join(st.output_folder, '0_stitched'))
