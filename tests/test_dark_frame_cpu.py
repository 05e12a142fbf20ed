"""--dark-frame without a device: the two statements of the definition (tests/dark_ref.py, image_stitcher_amd/darkframe.py)
against each other and against a per-pixel loop, the option's checks and parsers, the single-file reader's order, the run
grouping of the param table, the frame-making tool, and the chain's unchanged byte counts.  Every comparison is equality."""
import importlib.util
import itertools
import os
import re

import numpy as np
import pytest

import affine_ref
import bin_ref
import dark_cases
import dark_ref
import shift_ref
import warp_ref
from image_stitcher_amd import darkframe, native, stitcher_cli, synth, tiffio
from image_stitcher_amd.stitcher import Stitcher
from image_stitcher_amd.stitcher_parameters import StitchingParameters
from image_stitcher_amd.tilechain import BUFFERS, TileChain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _small(dtype):
    return [(h, w) for h, w in dark_cases.shapes(dtype) if h * w <= 600]


# ---------------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize('dtype', dark_cases.DTYPES)
def test_loop_equals_the_vectorised_form_and_the_host_module(dtype):
    shapes = _small(dtype)
    assert len(shapes) >= 10
    for (h, w), p in itertools.product(shapes, dark_cases.pedestals(dtype)):
        planes, frames = dark_cases.planes(dtype, h, w), dark_cases.frames(dtype, h, w)
        for fi in range(len(frames)):
            want = dark_cases.reference(dtype, h, w, ('frame', fi), p)
            for i in range(len(planes)):
                np.testing.assert_array_equal(dark_ref.loop(planes[i], frames[fi], p), want[i], err_msg=f'{(h, w)} P={p} frame {fi}')
                got = darkframe.dark_image(planes[i], frames[fi], p)
                assert got.dtype == planes.dtype
                np.testing.assert_array_equal(got, want[i])
        for c in dark_cases.constants(dtype):
            want = dark_cases.reference(dtype, h, w, ('constant', c), p)
            for i in (0, 1, 4):
                np.testing.assert_array_equal(dark_ref.loop(planes[i], c, p), want[i], err_msg=f'{(h, w)} P={p} constant {c}')
                np.testing.assert_array_equal(darkframe.dark_image(planes[i], c, p), want[i])


@pytest.mark.parametrize('dtype', dark_cases.DTYPES)
def test_host_module_on_every_shape(dtype):
    for (h, w), p in itertools.product(dark_cases.shapes(dtype), dark_cases.pedestals(dtype)):
        planes, frames = dark_cases.planes(dtype, h, w), dark_cases.frames(dtype, h, w)
        for fi in (2, 3):
            want = dark_cases.reference(dtype, h, w, ('frame', fi), p)
            np.testing.assert_array_equal(np.stack([darkframe.dark_image(pl, frames[fi], p) for pl in planes]), want)


@pytest.mark.parametrize('dtype', dark_cases.DTYPES)
def test_the_clamp_at_both_ends(dtype):
    m = dark_cases.top(dtype)
    img = np.array([[0, 1, 5, m - 1, m]], dtype=dtype)
    for fn in (dark_ref.dark_image, darkframe.dark_image, dark_ref.loop):
        assert fn(img, np.array([[1, 1, 6, 0, 0]], dtype=dtype), 0).tolist() == [[0, 0, 0, m - 1, m]]      # below 0 -> 0
        assert fn(img, 0, m).tolist() == [[m, m, m, m, m]]                                                   # above M -> M
        assert fn(img, m, 0).tolist() == [[0, 0, 0, 0, 0]]
        assert fn(img, m, m).tolist() == img.tolist()
        assert fn(img, 3, 1).tolist() == [[0, 0, 3, m - 3, m - 2]]
        assert fn(img, 1, 3).tolist() == [[2, 3, 7, m, m]]
    # the sum is taken in a wider signed type: neither end wraps
    assert dark_ref.dark_image(np.array([[0]], dtype), np.array([[m]], dtype), 0)[0, 0] == 0
    assert dark_ref.dark_image(np.array([[m]], dtype), np.array([[0]], dtype), m)[0, 0] == m


@pytest.mark.parametrize('dtype', dark_cases.DTYPES)
def test_identity(dtype):
    for (h, w), p in itertools.product(dark_cases.shapes(dtype), dark_cases.pedestals(dtype)):
        planes = dark_cases.planes(dtype, h, w)
        np.testing.assert_array_equal(dark_ref.dark_image(planes, p, p), planes)
        np.testing.assert_array_equal(dark_ref.dark_image(planes, np.full((h, w), p, dtype), p), planes)
        first = planes[0]
        assert darkframe.dark_image(first, p, p) is first      # nothing is computed
        assert darkframe.is_identity(p, p) and darkframe.is_identity(None, p) and not darkframe.is_identity(p + 1, p)


def test_rgb_per_colour_plane_and_page_stacks():
    h, w = 37, 53
    planes, frames = dark_cases.planes('uint8', h, w), dark_cases.frames('uint8', h, w)
    rgb = np.ascontiguousarray(np.moveaxis(planes[[0, 3, 4]], 0, 2))
    per_plane = [frames[2], None, 7]
    for fn in (dark_ref.dark_image, darkframe.dark_image):
        got = fn(rgb, per_plane, 5)
        assert got.shape == rgb.shape and got.dtype == rgb.dtype
        np.testing.assert_array_equal(got[:, :, 0], dark_ref.dark_image(planes[0], frames[2], 5))
        np.testing.assert_array_equal(got[:, :, 1], rgb[:, :, 1])                                  # no frame: the file's plane
        np.testing.assert_array_equal(got[:, :, 2], dark_ref.dark_image(planes[4], 7, 5))
    page = dark_cases.planes('uint16', h, w)[:1]
    frame = dark_cases.frames('uint16', h, w)[3]
    got = darkframe.dark_image(page, frame, 9)
    assert got.shape == (1, h, w)
    np.testing.assert_array_equal(got, dark_ref.dark_image(page, frame, 9))
    with pytest.raises(ValueError):
        darkframe.dark_image(rgb, [1, 2], 0)
    with pytest.raises(ValueError):
        darkframe.dark_image(planes[0].astype(np.float32), 1, 0)
    with pytest.raises(ValueError):
        darkframe.dark_image(planes[0], frames[2][:, :-1], 0)
    for bad in (-1, 256, 1.0, True, None):
        with pytest.raises(ValueError):
            darkframe.dark_image(planes[0], 3, bad)


def test_modules_are_written_apart():
    with open(os.path.join(ROOT, 'tests', 'dark_ref.py')) as fh:
        assert not re.search(r'^\s*(from|import)\s+\S*(darkframe|image_stitcher_amd)', fh.read(), re.M)
    with open(os.path.join(ROOT, 'image-stitcher_amd', 'darkframe.py')) as fh:
        assert not re.search(r'^\s*(from|import)\s+\S*dark_ref', fh.read(), re.M)


# ---------------------------------------------------------------------------------------------------- the option
def test_parse_source_and_command_line():
    assert darkframe.parse_source('0') == 0 and darkframe.parse_source('100') == 100 and darkframe.parse_source('007') == 7
    assert darkframe.parse_source('dark/f.npy') == 'dark/f.npy' and darkframe.parse_source('F.TIFF') == 'F.TIFF'
    assert darkframe.parse_source('100.tif') == '100.tif'
    for bad in ('', '-1', '1.5', '1e2', '+3', 'frame.png', 'frame', None, 5):
        with pytest.raises(ValueError):
            darkframe.parse_source(bad)
    args = stitcher_cli.parse_args(['-i', 'x', '--dark-frame', '*', '100', '--dark-frame', 'Fluorescence 488 nm Ex', 'd.npy',
                                    '--dark-pedestal', '10'])
    assert stitcher_cli.dark_frames_of(args.dark_frame) == {'*': 100, 'Fluorescence 488 nm Ex': 'd.npy'}
    assert args.dark_pedestal == 10
    plain = stitcher_cli.parse_args(['-i', 'x'])
    assert stitcher_cli.dark_frames_of(plain.dark_frame) is None and plain.dark_pedestal == 0
    with pytest.raises(ValueError, match="'B'.*twice"):
        stitcher_cli.dark_frames_of([['B', '1'], ['B', '2']])
    with pytest.raises(ValueError):
        stitcher_cli.dark_frames_of([['B', 'x.png']])
    with pytest.raises(SystemExit):
        stitcher_cli.parse_args(['-i', 'x', '--dark-pedestal', '1.5'])


def test_check_option():
    assert darkframe.check_option(None) == ({}, 0) and darkframe.check_option({}, 5) == ({}, 5)
    frame = np.zeros((4, 4), np.uint16)
    got, p = darkframe.check_option({'A': 3, '*': frame, 'B': 'x.npy', 'C': np.int64(9)}, np.int32(2))
    assert got['A'] == 3 and got['*'] is frame and got['B'] == 'x.npy' and got['C'] == 9 and p == 2 and type(p) is int
    for bad in ({'A': -1}, {'A': 1.0}, {'A': True}, {'A': None}, {'A': 'x.png'}, {'A': np.zeros((4,), np.uint16)},
                {'A': np.zeros((4, 4), np.float32)}, {'A': np.zeros((2, 4, 4), np.uint8)}, {5: 1}, [('A', 1)], 'A', 7):
        with pytest.raises(ValueError):
            darkframe.check_option(bad)
    for bad in (-1, 65536, 1.0, True, None, '3'):
        with pytest.raises(ValueError):
            darkframe.check_option({'A': 1}, bad)


def test_load_frame(tmp_path):
    frame = np.array(dark_cases.frames('uint16', 37, 53)[3])
    npy, tif = str(tmp_path / 'f.npy'), str(tmp_path / 'f.tiff')
    np.save(npy, frame)
    tiffio.write_tiff(tif, frame)
    for source in (npy, tif, frame):
        got = darkframe.load_frame(source, (37, 53), 'uint16', 'A')
        np.testing.assert_array_equal(got, frame)
        assert got.flags.c_contiguous
    assert darkframe.load_frame(65535, (37, 53), 'uint16') == 65535 and darkframe.load_frame(255, (3, 3), np.uint8) == 255
    with pytest.raises(ValueError, match='256.*0..255'):
        darkframe.load_frame(256, (37, 53), 'uint8', 'A')
    with pytest.raises(ValueError, match='no such file'):
        darkframe.load_frame(str(tmp_path / 'missing.npy'), (37, 53), 'uint16', 'A')
    with pytest.raises(ValueError, match=r"'A'.*\(37, 53\).*exactly their shape and dtype"):
        darkframe.load_frame(npy, (37, 54), 'uint16', 'A')
    with pytest.raises(ValueError, match='exactly their shape and dtype'):
        darkframe.load_frame(npy, (37, 53), 'uint8', 'A')
    with pytest.raises(ValueError, match='exactly their shape and dtype'):
        darkframe.load_frame(frame.astype(np.uint8), (37, 53), 'uint16', 'A')
    note = darkframe.frame_note(npy, frame)
    assert note['path'] == npy and len(note['sha256']) == 64
    assert (note['min'], note['max'], note['mean']) == (int(frame.min()), 65535, int(frame.astype(np.int64).sum()) // frame.size)
    assert darkframe.frame_note(7, 7) == {'constant': 7}


C405, C488, C561 = synth.DEFAULT_CHANNELS[:3]
SPEC = dict(rows=2, cols=2, tile_h=64, tile_w=64, ov_y=24, ov_x=24, nz=1, channels=(C405, C488, C561), seed=37)


def _prepared(root, params=None, **kw):
    st = Stitcher(StitchingParameters(input_folder=root, **(params or {})), normalization=None, **kw)
    st.get_timepoints()
    st.extract_acquisition_parameters()
    st.get_pixel_size()
    st.parse_acquisition_metadata()
    return st


def test_refusals_once_the_metadata_is_parsed(tmp_path, capsys):
    root = str(tmp_path / 'acq')
    synth.write_acquisition(synth.GridSpec(**SPEC), root)
    good = np.full((64, 64), 90, np.uint16)
    np.save(str(tmp_path / 'good.npy'), good)
    with pytest.raises(ValueError, match="'no such channel'.*not a channel"):
        _prepared(root, dark_frames={'no such channel': 1})
    with pytest.raises(ValueError, match="'DPC'"):
        _prepared(root, dark_frames={'DPC': 1})
    with pytest.raises(ValueError, match='exactly their shape and dtype'):
        _prepared(root, dark_frames={C488: np.zeros((64, 65), np.uint16)})
    with pytest.raises(ValueError, match='exactly their shape and dtype'):
        _prepared(root, dark_frames={C488: np.zeros((64, 64), np.uint8)})
    with pytest.raises(ValueError, match='no such file'):
        _prepared(root, dark_frames={'*': str(tmp_path / 'missing.tif')})
    with pytest.raises(ValueError, match='dark_pedestal'):
        Stitcher(StitchingParameters(input_folder=root), dark_frames={C488: 1}, dark_pedestal=65536)
    with pytest.raises(ValueError, match='dark_frames'):
        Stitcher(StitchingParameters(input_folder=root), dark_frames={C488: 65536 * 2.0})
    dpc_root = str(tmp_path / 'dpc' / 'acq')
    left, right = 'BF LED matrix left half', 'BF LED matrix right half'
    synth.write_acquisition(synth.GridSpec(**dict(SPEC, channels=(left, right, C488))), dpc_root)
    with pytest.raises(ValueError, match="'DPC'.*read from no file"):
        _prepared(dpc_root, dpc=True, dark_frames={'DPC': 1})
    st = _prepared(dpc_root, dpc=True, dark_frames={left: 100, right: good}, dark_pedestal=3)
    assert st._dark_params == {st.monochrome_channels.index(left): (-1, 100), st._dpc_index: (-1, 100),
                               st.monochrome_channels.index(right): (0, 0)}
    assert st._dark_right == (0, 0) and st._dark_stack.shape == (1, 64, 64)
    # uint8 files: constants and the pedestal are held to 255
    u8_root = str(tmp_path / 'u8' / 'acq')
    synth.write_acquisition(synth.GridSpec(**dict(SPEC, dtype='uint8')), u8_root)
    with pytest.raises(ValueError, match='256.*0..255'):
        _prepared(u8_root, dark_frames={C488: 256})
    with pytest.raises(ValueError, match='dark_pedestal 256'):
        _prepared(u8_root, dark_frames={C488: 1}, dark_pedestal=256)
    # '*' with an override; the registration channel takes its frame; equal frames are uploaded once; the identity is dropped
    capsys.readouterr()
    st = _prepared(root, params=dict(use_registration=True, registration_channel=C405),
                   dark_frames={'*': str(tmp_path / 'good.npy'), C561: 5, C488: good.copy()}, dark_pedestal=5)
    assert capsys.readouterr().out.count('[dark-frame]') == 1
    idx = st.monochrome_channels.index
    assert st._dark_params == {idx(C405): (0, 0), idx(C488): (0, 0)} and st._dark_stack.shape == (1, 64, 64)
    assert sorted(st._dark_note) == sorted([C405, C488, C561]) and st._dark_note[C561] == {'constant': 5}
    assert st._dark_right is None
    off = _prepared(root)
    assert off._dark_params == {} and off._dark_stack is None and off.dark_frames == {}
    assert '[dark-frame]' not in capsys.readouterr().out


def test_read_tile_file_subtracts_first_then_warps_shifts_and_bins(tmp_path):
    root = str(tmp_path / 'acq')
    synth.write_acquisition(synth.GridSpec(**SPEC), root)
    rng = np.random.default_rng(5)
    frame = rng.integers(8000, 16000, (64, 64)).astype(np.uint16)
    D, S, A = 20000, (77, -200), (300, -4000, 4000, 300)
    st = _prepared(root, dark_frames={C488: frame, C561: 9000, C405: 7}, dark_pedestal=7, distortion_correction=D, tile_binning=2,
                   channel_shifts={C488: S, C561: (-300, 40)}, channel_affines={C561: A})
    for channel, dark in ((C488, frame), (C561, 9000), (C405, 7)):
        info = next(v for v in st.get_region_data(0, 'R0').values() if v['channel'] == channel)
        raw = tiffio.read_image(info['filepath'])
        want = warp_ref.warp_file_image(dark_ref.dark_file_image(raw, dark, 7), D)
        if channel == C488:
            want = shift_ref.shift_file_image(want, *S)
        elif channel == C561:
            want = affine_ref.affine_file_image(want, (-300, 40), A)
        want = bin_ref.bin_file_image(want, 2, 'mean')
        np.testing.assert_array_equal(st._read_tile_file(info['filepath'], channel), want, err_msg=channel)
        np.testing.assert_array_equal(st.get_tile(0, 'R0', info['x'], info['y'], channel, 0), want)
    # alone: the file minus its frame; a channel whose frame is the identity, and a read without a channel, give the file
    alone = _prepared(root, dark_frames={C488: frame, C405: 7}, dark_pedestal=7)
    for channel in (C488, C405, C561):
        info = next(v for v in alone.get_region_data(0, 'R0').values() if v['channel'] == channel)
        raw = tiffio.read_image(info['filepath'])
        want = dark_ref.dark_file_image(raw, frame, 7) if channel == C488 else raw
        np.testing.assert_array_equal(alone._read_tile_file(info['filepath'], channel), want)
        assert (want != raw).mean() > 0.5 or channel != C488
        np.testing.assert_array_equal(alone._read_tile_file(info['filepath']), raw)


# ---------------------------------------------------------------------------------------------------- the param table's runs
def test_param_runs():
    p = 5
    same = (-1, p)
    assert darkframe.param_runs([], p) == []
    assert darkframe.param_runs([same] * 4, p) == []
    assert darkframe.param_runs([(0, 0)] * 3, p) == [(0, 3, 0, 0)]
    table = [(0, 0), (0, 0), same, same, (1, 0), same, (-1, 4), (-1, 4), (-1, 6), (0, 0)]
    assert darkframe.param_runs(table, p) == [(0, 2, 0, 0), (4, 5, 1, 0), (6, 8, -1, 4), (8, 9, -1, 6), (9, 10, 0, 0)]
    # the pedestal decides what the identity is
    assert darkframe.param_runs([(-1, 4), same], 4) == [(1, 2, -1, 5)]
    # every plane lies in exactly one run or in an identity gap
    covered = sorted(i for a, b, _, _ in darkframe.param_runs(table, p) for i in range(a, b))
    assert covered == [i for i, pair in enumerate(table) if pair != same]


# ---------------------------------------------------------------------------------------------------- the tool
def test_dark_frame_make(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location('dark_frame_make', os.path.join(ROOT, 'tools', 'dark_frame_make.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rng = np.random.default_rng(11)
    folder = tmp_path / 'dark' / '0'
    os.makedirs(folder)
    stacks = {}
    for token in ('Fluorescence_488_nm_Ex', 'Fluorescence_561_nm_Ex'):
        stacks[token] = rng.integers(90, 120, (5, 19, 23)).astype(np.uint16)
        stacks[token][:, 3, 4] = 65535      # a warm pixel
        for i, img in enumerate(stacks[token]):
            tiffio.write_tiff(str(folder / f'R0_{i}_0_{token}.tiff'), img)
    out = str(tmp_path / 'frame.npy')
    frame = tool.main(['-i', str(tmp_path / 'dark'), '-o', out, '--channel', 'Fluorescence 488 nm Ex'])
    want = ((stacks['Fluorescence_488_nm_Ex'].astype(np.int64).sum(0) + 2) // 5).astype(np.uint16)
    np.testing.assert_array_equal(frame, want)
    np.testing.assert_array_equal(np.load(out), want)
    assert frame.dtype == np.uint16 and frame[3, 4] == 65535
    printed = capsys.readouterr().out
    assert f'--dark-frame "Fluorescence 488 nm Ex" {out}' in printed and '5 exposures' in printed
    # all files, to a .tiff; the rounding is half up: (1 + 2 + 2) -> (5 + 1) // 3 = 2, (1 + 1 + 2) -> (4 + 1) // 3 = 1
    both = tool.main(['-i', str(tmp_path / 'dark'), '-o', str(tmp_path / 'all.tiff')])
    all_imgs = np.concatenate(list(stacks.values())).astype(np.int64)
    np.testing.assert_array_equal(both, ((all_imgs.sum(0) + 5) // 10).astype(np.uint16))
    np.testing.assert_array_equal(tiffio.read_image(str(tmp_path / 'all.tiff')).reshape(19, 23), both)
    assert '--dark-frame "*"' in capsys.readouterr().out
    small = tmp_path / 'small'
    os.makedirs(small)
    for i, v in enumerate(([1, 1], [2, 1], [2, 2])):
        tiffio.write_tiff(str(small / f'd{i}.tif'), np.array([v], np.uint8))
    assert tool.main(['-i', str(small), '-o', str(tmp_path / 's.npy')]).tolist() == [[2, 1]]
    tiffio.write_tiff(str(small / 'other.tif'), np.zeros((2, 2), np.uint8))
    with pytest.raises(ValueError):
        tool.main(['-i', str(small), '-o', str(tmp_path / 's.npy')])
    with pytest.raises(ValueError, match='no dark exposure'):
        tool.main(['-i', str(small), '-o', str(tmp_path / 's.npy'), '--channel', 'nothing'])


# ---------------------------------------------------------------------------------------------------- the chain
FH, FW, NUM_Z = 97, 131, 2
GRID = list(itertools.product((0, 20000), (1, 2), ('none', 'hot'), (False, True), (False, True), ('uint8', 'uint16')))


def _chain(ppm, k, despeckle, tophat, dpc, dtype, **kw):
    return TileChain(distortion_ppm=ppm, binning=k, binning_method='mean', dpc_planes=range(2 * NUM_Z, 3 * NUM_Z) if dpc else (),
                     dpc_gain=1, despeckle=despeckle, despeckle_threshold=40, tophat_radius=5 if tophat else None,
                     seam_qc_radius=2, file_shape=(FH, FW), tile_shape=(FH // k, FW // k), dtype=dtype, num_z=NUM_Z, **kw)


def test_chain_buffers_and_bytes_do_not_change():
    assert not any('dark' in b[0] for b in BUFFERS) and len(BUFFERS) == 9
    for ppm, k, despeckle, tophat, dpc, dtype in GRID:
        plain = _chain(ppm, k, despeckle, tophat, dpc, dtype)
        on = _chain(ppm, k, despeckle, tophat, dpc, dtype, dark_params={0: (0, 0), 3: (-1, 100)}, dark_frames=object(),
                    dark_pedestal=7, dark_derived=(0, 0))
        for other in (on, _chain(ppm, k, despeckle, tophat, dpc, dtype, dark_params=None),
                      _chain(ppm, k, despeckle, tophat, dpc, dtype, dark_params={}, dark_pedestal=9)):
            assert other.buffers == plain.buffers
            for n in (1, 6):
                assert other.writer_plane_bytes(n) == plain.writer_plane_bytes(n)
                for derived in (False, True):
                    assert other.plane_bytes(n, derived) == plain.plane_bytes(n, derived)
    b = np.dtype('uint16').itemsize
    assert _chain(0, 1, 'none', False, False, 'uint16', dark_params={0: (0, 0)}).plane_bytes(6, False) == 6 * FH * FW * b


def test_plane_darks():
    chain = _chain(0, 1, 'none', False, False, 'uint16', dark_params={0: (0, 0), 3: (-1, 100)}, dark_pedestal=7, dark_derived=(-1, 7))
    assert chain.plane_darks([0, 1, 2]) == [(0, 0), (0, 0), (-1, 7)]
    assert chain.plane_darks([2, 3, 4, 5]) is None and chain.plane_darks([]) is None and chain.plane_darks(None) is None
    assert chain.plane_darks([5, 6]) == [(-1, 7), (-1, 100)]
    assert chain.dark_derived is None      # the right halves' pair is the identity: no launch
    assert _chain(0, 1, 'none', False, False, 'uint16', dark_derived=(-1, 3)).dark_derived == (-1, 3)
    assert _chain(0, 1, 'none', False, False, 'uint16').plane_darks([0, 1]) is None


# ---------------------------------------------------------------------------------------------------- the documents
def test_documents_header_and_sources():
    doc = stitcher_cli.__doc__
    for flag in ('--dark-frame', '--dark-pedestal'):
        assert '``' + flag + '``' in doc and any(names == (flag,) for names, _ in stitcher_cli.FLAGS)
    help_text = dict((names[0], kw['help']) for names, kw in stitcher_cli.FLAGS)['--dark-frame']
    assert '_stitched_dark_frame.json' in help_text and 'clamp(I - D + P' in help_text
    with open(os.path.join(ROOT, 'include', 'squidstitch.h')) as fh:
        header = fh.read()
    assert re.search(r'int\s+sq_dark_tiles\s*\(', header) and 'clamp(I(y, x) - D(y, x) + P, 0, M)' in header
    assert re.search(r'#define\s+SQ_DARK_IMAGES_PER_THREAD\s+(\d+)\b', header).group(1) == str(native.SQ_DARK_IMAGES_PER_THREAD)
    assert dark_cases.IPT == native.SQ_DARK_IMAGES_PER_THREAD
    assert re.search(r'#define\s+SQ_VERSION\s+108\b', header)
    assert 'sq_dark_tiles' in native.EXPORTS and len(native.EXPORTS['sq_dark_tiles'][1]) == 15
    with open(os.path.join(ROOT, 'image-stitcher_amd', 'csrc', 'Makefile')) as fh:
        assert re.search(r'^SRCS\s*=.*\bdark\.hip\b', fh.read(), re.M)
    with open(os.path.join(ROOT, 'image-stitcher_amd', 'csrc', 'dark.hip')) as fh:
        kernel = fh.read()
    assert 'tests/dark_ref.py' in kernel and 'asm' not in kernel
    for name, words in (('README.md', ('--dark-frame', '--dark-pedestal', 'dark_frame_make.py')),
                        ('DESIGN.md', ('5.4n', 'sq_dark_tiles', 'clamp(I - D + P, 0, M)')),
                        ('INTEGRATION.md', ('sq_dark_tiles',))):
        with open(os.path.join(ROOT, name)) as fh:
            text = fh.read()
        for word in words:
            assert word in text, (name, word)
    if os.path.exists(os.path.join(ROOT, 'image-stitcher_amd', 'csrc', 'libsquidstitch.so')):
        assert hasattr(native.lib(), 'sq_dark_tiles')
