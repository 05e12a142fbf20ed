"""--channel-shift on the device: sq_shift_tiles against the numpy definition (tests/shift_ref.py), and whole runs with the option
against runs without it on a folder whose files of the shifted channels were translated beforehand.  Every comparison is
equality, but the scan tool's measurement (one step of its resolution)."""
import hashlib
import importlib.util
import json
import os
import random

import numpy as np
import pytest

import bin_ref
import shift_cases
import shift_ref
import stream_cases as SC
import warp_ref
from image_stitcher_amd import channelshift, native, stitcher_cli, synth, tiffio
from image_stitcher_amd.stitcher import Stitcher
from image_stitcher_amd.stitcher_parameters import StitchingParameters

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the cached planes are read-only)


def _full(shape, value, dtype):
    return _dev(np.full(shape, value, dtype=np.dtype(dtype)))


# ---------------------------------------------------------------------------------------------------- the kernel
# (the shapes and the kernel's own sizes they are chosen from: tests/shift_cases.py)
@pytest.mark.parametrize('dtype', shift_cases.DTYPES)
@pytest.mark.parametrize('shift', shift_cases.SHIFTS)
def test_kernel_equals_the_definition(shift, dtype):
    for h, w in shift_cases.shapes(dtype):
        planes = shift_cases.planes(dtype, h, w)
        src = _dev(planes)
        want = shift_cases.reference(dtype, h, w, shift)
        got = native.shift_tiles(src, shift)
        assert got.dtype == src.dtype and tuple(got.shape) == planes.shape
        host = got.cpu().numpy()
        for i, name in enumerate(shift_cases.PLANE_NAMES):
            np.testing.assert_array_equal(host[i], want[i], err_msg=f'{(h, w)} S={shift} {name}')
        np.testing.assert_array_equal(src.cpu().numpy(), planes)      # the source is left as it was
        if shift == (0, 0):
            np.testing.assert_array_equal(host, planes)                # the identity


@pytest.mark.parametrize('dtype', shift_cases.DTYPES)
def test_grid_edges(dtype):
    """Two planes at the three edges of the strip / segment grid: narrower than one vector; one vector more than a workgroup is
    wide (two strips); and, at that width, one row more than a workgroup's rows (two segments)."""
    wide = shift_cases.STRIP[dtype] + shift_cases.VEC[dtype]
    for h, w in ((3, 5), (3, wide), (shift_cases.RPT + 1, wide)):
        planes = shift_cases.planes(dtype, h, w, 2)
        got = native.shift_tiles(_dev(planes), shift_cases.MIXED).cpu().numpy()
        np.testing.assert_array_equal(got, shift_cases.reference(dtype, h, w, shift_cases.MIXED, 2), err_msg=f'{(h, w)}')


@pytest.mark.parametrize('dtype', shift_cases.DTYPES)
def test_a_table_of_shifts_with_several_runs(dtype):
    h, w, n = shift_cases.MANY
    assert h > shift_cases.RPT
    planes = shift_cases.planes(dtype, h, w, n)
    # runs of equal pairs: two shifted planes, two zero, one shifted, one zero, one shifted (seven planes, five grids)
    table = [(77, -200), (77, -200), (0, 0), (0, 0), shift_cases.MIXED, (0, 0), (-16384, 255)]
    got = native.shift_tiles(_dev(planes), table).cpu().numpy()
    for i, pair in enumerate(table):
        np.testing.assert_array_equal(got[i], shift_cases.reference(dtype, h, w, pair, n)[i], err_msg=f'plane {i} {pair}')
    np.testing.assert_array_equal(got[2], planes[2])
    # a stack with two leading dimensions: one pair per index of the first, for all planes under it
    stack = _dev(planes[:6].reshape(2, 3, h, w))
    pairs = [(0, 0), (128, -128)]
    got = native.shift_tiles(stack, pairs).cpu().numpy()
    np.testing.assert_array_equal(got[0], planes[:3])
    np.testing.assert_array_equal(got[1], shift_cases.reference(dtype, h, w, (128, -128), n)[3:6])
    # ... and one pair for every plane of it; numpy integers are taken
    got = native.shift_tiles(stack, (np.int64(128), np.int32(-128))).cpu().numpy().reshape(6, h, w)
    np.testing.assert_array_equal(got, shift_cases.reference(dtype, h, w, (128, -128), n)[:6])
    for bad in ([(1, 1)], [(1, 1)] * 3, [(1, 1), (1,)], [(1, 1), (1.0, 1)], 5, None, [(1, 1), (True, 1)]):
        with pytest.raises(ValueError):
            native.shift_tiles(stack, bad)


def test_more_planes_than_one_launch_takes():
    """65535 planes go into one grid: one plane more, of 1 x 1 pixels, through the C entry -- as one run, and as a table whose
    runs end inside and at the split."""
    import ctypes
    import torch
    n = 65535 + 1
    src = torch.arange(n, dtype=torch.int32, device=DEV).remainder(251).to(torch.uint8)
    out = torch.full((2 * n,), 255, dtype=torch.uint8, device=DEV)
    L = native.lib()
    one = (ctypes.c_int32 * 2)(16384, -16384)
    assert L.sq_shift_tiles(src.data_ptr(), out.data_ptr(), n, 1, 1, 1, 1, 1, 1, native.SQ_U8, one, n, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:n], src) and bool((out[n:] == 255).all())      # 1 x 1: the identity, plane for plane
    out.fill_(255)
    table = (ctypes.c_int32 * 8)(0, 0, 77, -200, 77, -200, 0, 0)             # four pairs of 16384 planes each
    assert L.sq_shift_tiles(src.data_ptr(), out.data_ptr(), n, 1, 1, 1, 1, 1, 1, native.SQ_U8, table, n // 4, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:n], src) and bool((out[n:] == 255).all())
    # two columns: the half-pixel blend of every plane's pair, and its replicated edge
    pairs = torch.arange(2 * n, dtype=torch.int32, device=DEV).remainder(241).to(torch.uint8)
    out.fill_(255)
    half = (ctypes.c_int32 * 2)(0, 128)
    assert L.sq_shift_tiles(pairs.data_ptr(), out.data_ptr(), n, 1, 2, 2, 2, 2, 2, native.SQ_U8, half, n, None) == 0
    torch.cuda.synchronize()
    a, b = pairs[0::2].to(torch.int32), pairs[1::2].to(torch.int32)
    want = torch.stack([(a + b + 1) >> 1, b], dim=1).to(torch.uint8).reshape(-1)
    assert shift_ref.loop(np.array([[10, 201]], np.uint8), 0, 128).tolist() == [[106, 201]]
    assert torch.equal(out, want)


@pytest.mark.parametrize('dtype', shift_cases.DTYPES)
@pytest.mark.parametrize('shift', [shift_cases.MIXED, (-300, 16384)])
def test_views_pitches_offsets_guard_and_repeatability(shift, dtype):
    import torch
    h, w = 9, 37
    planes = shift_cases.planes(dtype, h, w)
    n_planes = len(planes)
    tdtype = native.torch_dtype_of(np.dtype(dtype))
    fill = int(np.iinfo(np.dtype(dtype)).max) // 3
    want = shift_cases.reference(dtype, h, w, shift)
    # every other plane of a stack, as source and as destination; the planes between stay as they are
    big = _dev(planes)
    out_big = _full((n_planes + 1, h, w), fill, dtype)
    got = native.shift_tiles(big[::2], shift, out=out_big[1::2])
    assert got.data_ptr() == out_big[1::2].data_ptr()
    np.testing.assert_array_equal(out_big.cpu().numpy()[1::2], want[::2])
    assert (out_big.cpu().numpy()[::2] == fill).all()
    np.testing.assert_array_equal(big.cpu().numpy(), planes)
    # a pitched source and a pitched destination: the columns beyond w of dst stay as they are
    wide_src = _dev(np.concatenate([planes, np.full((n_planes, h, 5), 7, planes.dtype)], axis=2))
    wide_dst = _full((n_planes, h, w + 3), fill, dtype)
    native.shift_tiles(wide_src[:, :, :w], shift, out=wide_dst[:, :, :w])
    np.testing.assert_array_equal(wide_dst.cpu().numpy()[:, :, :w], want)
    assert (wide_dst.cpu().numpy()[:, :, w:] == fill).all()
    # a source and a destination that each start at an element offset, through every phase of 16 bytes -- 8 uint16 / 16 uint8
    # -- plus one beyond it: the destination's phase decides between the 16-byte store and the element stores, and the source's
    # phase puts the span's 16-byte load on every alignment an element allows.  Both are views of wider buffers whose row pitch
    # is a multiple of 16 bytes.
    vec = 16 // planes.itemsize
    pitch = (w + vec - 1) // vec * vec + vec
    n_el = n_planes * h * pitch
    padded = np.full((n_planes, h, pitch), 7, planes.dtype)
    padded[:, :, :w] = planes
    padded_dev = _dev(padded).reshape(-1)
    for s_off in list(range(vec)) + [vec + 3]:
        buf = _full((n_el + 2 * vec + 8,), 0, dtype)
        buf[s_off:n_el + s_off] = padded_dev
        src_off = buf[s_off:n_el + s_off].view(n_planes, h, pitch)[:, :, :w]
        assert (src_off.data_ptr() // planes.itemsize) % vec == s_off % vec
        for d_off in list(range(vec)) + [vec + 1]:
            obuf = _full((n_el + 2 * vec + 8,), fill, dtype)
            out_off = obuf[d_off:n_el + d_off].view(n_planes, h, pitch)
            got = native.shift_tiles(src_off, shift, out=out_off[:, :, :w])
            np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f'src offset {s_off}, dst offset {d_off}')
            host = obuf.cpu().numpy()
            assert (host[:d_off] == fill).all() and (host[n_el + d_off:] == fill).all()
            assert (host[d_off:n_el + d_off].reshape(n_planes, h, pitch)[:, :, w:] == fill).all()      # between w and the pitch
    np.testing.assert_array_equal(buf[s_off:n_el + s_off].cpu().numpy(), padded.reshape(-1))
    # a guard band of 0xA5 in front of and behind out stays intact
    nbytes = want.size * planes.itemsize
    raw = torch.full((4096 + nbytes + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    out = raw[4096:4096 + nbytes].view(tdtype).view(n_planes, h, w)
    native.shift_tiles(_dev(planes), shift, out=out)
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    assert bool((raw[:4096] == 0xA5).all()) and bool((raw[4096 + nbytes:] == 0xA5).all())
    # the same call twice: the same bytes
    runs = [native.shift_tiles(_dev(planes), shift).cpu().numpy().tobytes() for _ in range(2)]
    assert runs[0] == runs[1] == want.tobytes()


def test_refusals():
    import ctypes
    import torch
    t_np = np.arange(3 * 8 * 12, dtype=np.uint16).reshape(3, 8, 12)
    t = _dev(t_np)
    out = _full((3, 8, 12), 7, 'uint16')
    for bad in ((16385, 0), (0, -16385), (2.0, 1), (True, 1), (None, 1), ('2', 1)):
        with pytest.raises(ValueError):
            native.shift_tiles(t, bad, out=out)
    with pytest.raises(ValueError):
        native.shift_tiles(t.to(torch.float32), (2, 2), out=out)                      # a wrong dtype
    with pytest.raises(ValueError):
        native.shift_tiles(t.permute(0, 2, 1), (2, 2))                                # rows that are not contiguous
    with pytest.raises(ValueError):
        native.shift_tiles(t, (2, 2), out=out[:2])                                    # another shape
    with pytest.raises(ValueError):
        native.shift_tiles(t, (2, 2), out=_full((3, 8, 12), 7, 'uint8'))              # another dtype
    with pytest.raises(ValueError):
        native.shift_tiles(t, (2, 2), out=torch.zeros((3, 8, 12), dtype=torch.uint16))            # another device
    assert (out.cpu().numpy() == 7).all()      # nothing was launched
    # an out that shares memory with tiles
    before = t.cpu().numpy()
    for src, dst in ((t, t), (t[:2], t[1:]), (t[::2], t[1:3])):
        with pytest.raises(ValueError, match='out of place'):
            native.shift_tiles(src, (2, 2), out=dst)
    np.testing.assert_array_equal(t.cpu().numpy(), before)
    # the library itself refuses what the wrapper would let through, with its own message
    L = native.lib()
    pair = (ctypes.c_int32 * 6)(77, -200, 77, -200, 77, -200)

    def call(src=t.data_ptr(), dst=out.data_ptr(), n=3, h=8, w=12, sps=96, sp=12, dps=96, dp=12, dtype=native.SQ_U16, table=pair,
             per=3):
        return L.sq_shift_tiles(src, dst, n, h, w, sps, sp, dps, dp, dtype, table, per, None)

    assert call() == 0 and call(per=1) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), shift_ref.shift_image(t_np, 77, -200))
    assert call(table=(ctypes.c_int32 * 2)(0, 0)) == 0                   # (0, 0) is accepted: an exact copy
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), t_np)
    out.copy_(_full((3, 8, 12), 7, 'uint16'))
    torch.cuda.synchronize()
    assert call(n=0) == 0 and call(n=0, src=None, dst=None, table=None) == 0      # no image: SQ_OK, nothing launched
    for bad in (dict(table=(ctypes.c_int32 * 2)(16385, 0)), dict(table=(ctypes.c_int32 * 2)(0, -16385)), dict(table=None),
                dict(per=2), dict(per=0), dict(per=-1), dict(dtype=native.SQ_F32), dict(dtype=0), dict(sp=11), dict(dp=11),
                dict(sps=95), dict(dps=95), dict(src=None), dict(dst=None), dict(src=t.data_ptr() + 1),
                dict(dst=out.data_ptr() + 1), dict(n=-1), dict(dst=t.data_ptr() + 96 * 2), dict(dst=t.data_ptr()),
                dict(src=out.data_ptr(), n=1, per=1), dict(h=0), dict(w=0), dict(h=-1)):
        assert call(**bad) == -1, bad      # SQ_ERR_INVALID
    assert call(dst=t.data_ptr()) == -1 and 'overlap' in L.sq_last_error().decode()
    assert call(table=(ctypes.c_int32 * 2)(16385, 0)) == -1 and '16384' in L.sq_last_error().decode()
    for big in (dict(h=65536, sps=65536 * 12, dps=65536 * 12), dict(w=65536, sp=65536, dp=65536, sps=8 * 65536, dps=8 * 65536)):
        assert call(**big) == native.SQ_ERR_UNSUPPORTED, big
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7).all()
    np.testing.assert_array_equal(t.cpu().numpy(), before)


# ---------------------------------------------------------------------------------------------------- off the default stream
def _stream_call(shifts):
    def call(ctx, inp, out, stream):
        native.shift_tiles(inp['tiles'], shifts, out=out['out'], stream=stream)
        return {'out': out['out']}
    return call


def _stream_case(dtype, shifts):
    top = int(np.iinfo(dtype).max)
    shape = (4, 50, 70)
    real = {'tiles': np.random.default_rng(410).integers(0, top + 1, shape).astype(dtype)}
    poison = {'tiles': np.random.default_rng(411).integers(0, top + 1, shape).astype(dtype)}
    canary = {'out': np.full(shape, 7, dtype)}
    return SC.Case(f'shift-tiles-{np.dtype(dtype).name}', real, poison, canary, _stream_call(shifts),
                   lambda a, strict: {'out': np.stack([shift_ref.shift_image(p, *s) for p, s in zip(a['tiles'], shifts)])})


STREAM_CASES = {c.name: c for c in (_stream_case(np.uint16, [(77, -200), (77, -200), (0, 0), (-900, 128)]),
                                    _stream_case(np.uint8, [shift_cases.MIXED] * 4))}


@pytest.fixture(scope='module')
def streams():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    st = SC.Streams.open(torch.device('cuda:0'))
    if st.S is None:
        pytest.fail(f'no two of {SC.MAX_DRAWS} torch streams make progress while the other, the copy stream or the default '
                    'stream is lagged: they share hardware queues, and every stream race would stay hidden')
    assert st.lag_ms_seen >= 0.9 * SC.LAG_MS, f'the lag lasts {st.lag_ms_seen} ms, not {SC.LAG_MS}'
    return st


@pytest.fixture(scope='module')
def prepared(streams):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = SC.Prepared(STREAM_CASES[name], streams)
        return cache[name]
    return get


@pytest.mark.parametrize('mode', ['A', 'B'])
@pytest.mark.parametrize('name', sorted(STREAM_CASES))
def test_waits_for_its_stream(streams, prepared, name, mode):
    p = prepared(name)
    r = SC.experiment_e1(p.case, p.ctx, p.want, streams, mode)
    assert r.probe_full, f'{name}: the probe did not read the poison in full: the lag had ended when the call began'
    assert r.mismatch is None, f'E1-{mode} {r.mismatch}'


@pytest.mark.parametrize('name', sorted(STREAM_CASES))
def test_touches_no_other_stream(streams, prepared, name):
    p = prepared(name)
    r = SC.experiment_e2(p.case, p.ctx, p.want, streams)
    assert r.event_pending, (f"{name}: the other stream's event was complete when the outputs had been read (the call took "
                             f'{r.host_ms:.2f} ms on the host): the call waited for that stream, or its lag is too short')
    assert r.first is None, f'E2, the other stream still lagged: {r.first}'
    assert r.after is None, f'E2, after the other stream has drained: {r.after}'


# ---------------------------------------------------------------------------------------------------- whole runs
NOTE = '_stitched_channel_shift.json'
WARP_NOTE, BIN_NOTE = '_stitched_distortion.json', '_stitched_binning.json'
LEFT, RIGHT, FLUO = 'BF LED matrix left half', 'BF LED matrix right half', 'Fluorescence 488 nm Ex'
C405, C488, C561 = synth.DEFAULT_CHANNELS[:3]
# a synthetic 2 x 2 grid of 64 x 64 tiles with two z levels and three channels; the first channel is the registration channel
SPEC = dict(rows=2, cols=2, tile_h=64, tile_w=64, ov_y=24, ov_x=24, nz=2, channels=(C405, C488, C561), seed=37)
SHIFTS = {C488: (77, -200), C561: (-3 * 256, 2 * 256 + 128)}      # 1/256 px
FLAGS = ['--channel-shift', C488, '0.3', '-0.78125', '--channel-shift', C561, '-3', '2.5']
D = 20000


def _channel_of(name):
    return os.path.splitext(name.split('_', 3)[3])[0].replace('_', ' ')


def premake_folder(root, shifts, ppm=0, then_bin=1):
    """F -> F' in place: every tile file corrected by its definition (ppm), the files of the channels of ``shifts`` translated
    by the definition, and then, for the run with --tile-binning too, binned by its definition, the sensor pixel multiplied."""
    moved = 0
    for folder, _, names in os.walk(root):
        for name in names:
            if name.lower().endswith(('.tif', '.tiff')):
                path = os.path.join(folder, name)
                img = tiffio.read_image(path)
                new = warp_ref.warp_file_image(img, ppm) if ppm else img
                channel = _channel_of(name)
                if channel in shifts:
                    before = new
                    new = shift_ref.shift_file_image(new, *shifts[channel])
                    moved += int((new != before).any())
                if then_bin > 1:
                    new = bin_ref.bin_file_image(new, then_bin, 'mean')
                tiffio.write_tiff(path, new)
    assert moved > 0      # F' is not F
    if then_bin > 1:
        path = os.path.join(root, 'acquisition parameters.json')
        with open(path) as fh:
            ap = json.load(fh)
        ap['sensor_pixel_size_um'] = ap['sensor_pixel_size_um'] * then_bin
        with open(path, 'w') as fh:
            json.dump(ap, fh, indent=2)
    return moved


def _two_roots(tmp_path, spec=None, shifts=SHIFTS, ppm=0, then_bin=1):
    spec = spec or synth.GridSpec(**SPEC)
    a, b = str(tmp_path / 'with_flag' / 'acq'), str(tmp_path / 'premade' / 'acq')
    for r in (a, b):
        synth.write_acquisition(spec, r)
    premake_folder(b, shifts, ppm, then_bin)
    return a, b


def _cli(root, *extra):
    """One run through the command line -> its output folder."""
    random.seed(1234)
    stitcher_cli.main(['-i', root, '--normalization', 'none', *extra])
    base = os.path.dirname(root)
    outs = [d for d in os.listdir(base) if d.startswith(os.path.basename(root) + '_stitched_')]
    assert len(outs) == 1
    return os.path.join(base, outs[0])


def _api(root, **kw):
    """One run of a Stitcher made by hand -> the Stitcher."""
    random.seed(1234)
    st = Stitcher(StitchingParameters(input_folder=root), normalization=None, **kw)
    st.run()
    return st


def _prepared(root, batch_bytes_limit=None, params=None, **kw):
    st = Stitcher(StitchingParameters(input_folder=root, **(params or {})), normalization=None, **kw)
    if batch_bytes_limit is not None:
        st.batch_bytes_limit = batch_bytes_limit
    st.get_timepoints()
    st.extract_acquisition_parameters()
    st.get_pixel_size()
    st.parse_acquisition_metadata()
    return st


def _tree(out, skip=(NOTE,)):
    """{relative path: digest} of every file of an output tree but the options' own notes."""
    found = {}
    for folder, _, names in os.walk(out):
        for name in names:
            if not name.endswith(tuple(skip)):
                with open(os.path.join(folder, name), 'rb') as fh:
                    found[os.path.relpath(os.path.join(folder, name), out)] = hashlib.sha256(fh.read()).hexdigest()
    return found


def _notes(out, note=NOTE):
    return sorted(os.path.relpath(os.path.join(folder, n), out) for folder, _, names in os.walk(out) for n in names if n.endswith(note))


def _same_trees(got, want, skip=(NOTE,)):
    a, b = _tree(got, skip), _tree(want, skip)
    assert a and sorted(a) == sorted(b)
    differ = [k for k in a if a[k] != b[k]]
    assert not differ, differ[:10]
    assert any('.ome.zarr' in k and not os.path.basename(k).startswith('.') for k in a) or any(k.endswith('.ome.tiff') for k in a)
    assert _notes(got) and not _notes(want)
    return a


@pytest.mark.parametrize('fmt', ['.ome.zarr', '.ome.tiff'])
def test_flag_on_f_equals_no_flag_on_f_prime(tmp_path, capsys, fmt):
    a, b = _two_roots(tmp_path)
    capsys.readouterr()
    got = _cli(a, '-f', fmt, *FLAGS)
    assert capsys.readouterr().out.count('[channel-shift]') == 1
    want = _cli(b, '-f', fmt)
    assert '[channel-shift]' not in capsys.readouterr().out
    _same_trees(got, want)
    assert _notes(got) == [os.path.join('0_stitched', 'R0' + NOTE)]
    with open(os.path.join(got, '0_stitched', 'R0' + NOTE)) as fh:
        note = json.load(fh)
    assert note['channels'] == {C488: {'shift_256': [77, -200], 'shift_px': [77 / 256, -200 / 256]},
                                C561: {'shift_256': [-768, 640], 'shift_px': [-3.0, 2.5]}}
    assert note['tile_shape'] == [64, 64] and note['order'] == 'after the distortion correction, before the binning'
    # ... and the run on F without the flag is another tree
    third = str(tmp_path / 'plain' / 'acq')
    synth.write_acquisition(synth.GridSpec(**SPEC), third)
    plain = _tree(_cli(third, '-f', fmt))
    assert sorted(plain) == sorted(_tree(got)) and plain != _tree(got)


@pytest.mark.parametrize('mode', ['overwrite', 'feather'])
def test_registration_and_device_basic_flatfield(tmp_path, mode):
    """-r -ff: the registration channel is the frame and takes no shift; the flatfield estimate's samples and get_tile shift on
    the host with the same arithmetic."""
    a, b = _two_roots(tmp_path)
    flags = ('-r', '-ff', '--flatfield-estimator', 'basic', '--fusion-mode', mode)
    tree = _same_trees(_cli(a, *flags, *FLAGS), _cli(b, *flags))
    assert 'shift_table.json' in tree and 'flatfield_info.json' in tree
    st_a, st_b = _prepared(a, channel_shifts=SHIFTS), _prepared(b)
    for channel in (C405, C488, C561):
        info = next(v for v in st_a.get_region_data(0, 'R0').values() if v['channel'] == channel and v['z_level'] == 1)
        np.testing.assert_array_equal(st_a.get_tile(0, 'R0', info['x'], info['y'], channel, 1),
                                      st_b.get_tile(0, 'R0', info['x'], info['y'], channel, 1))


def test_with_distortion_correction_and_binning(tmp_path):
    """Correct, shift, bin, all in sensor pixels: a run on bin_2(shift(warp(F)))."""
    a, b = _two_roots(tmp_path, ppm=D, then_bin=2)
    flags = ('--z-projection', 'max', '--composite')
    got = _cli(a, '--distortion-correction', str(D), '--tile-binning', '2', *flags, *FLAGS)
    want = _cli(b, *flags)
    tree = _same_trees(got, want, skip=(NOTE, WARP_NOTE, BIN_NOTE))
    assert any('_mip' in k for k in tree) and any(k.endswith('.png') for k in tree)
    assert _notes(got, WARP_NOTE) and _notes(got, BIN_NOTE)


def test_with_tile_qc_and_seam_qc(tmp_path):
    a, b = _two_roots(tmp_path)
    kw = dict(tile_qc=True, seam_qc=True, seam_qc_min_pixels=16)
    got, want = _api(a, channel_shifts=SHIFTS, **kw), _api(b, **kw)
    tree = _same_trees(got.output_folder, want.output_folder)
    for part in ('_tile_qc.csv', '_tile_qc.json', '_seam_qc.csv', '_seam_qc.json'):
        assert any(part in k for k in tree), part
    assert got.tile_qc_table and got.tile_qc_table == want.tile_qc_table      # the report describes F''s files
    assert got.seam_qc_table and got.seam_qc_table == want.seam_qc_table


def test_uint8_rgb_files(tmp_path):
    """The names come out of the output channels: <base>_R, <base>_G, <base>_B, each with a pair of its own."""
    spec = synth.GridSpec(rows=2, cols=2, tile_h=64, tile_w=64, ov_y=24, ov_x=24, channels=('BF LED matrix full_RGB', C488),
                          rgb_channels=('BF LED matrix full_RGB',), dtype='uint8', seed=41)
    st = _prepared_names(tmp_path, spec)
    base = [n for n in st if n.endswith('_R')][0][:-2]
    shifts = {f'{base}_R': (77, -200), f'{base}_B': (-256, 300)}
    a, b = str(tmp_path / 'with_flag' / 'acq'), str(tmp_path / 'premade' / 'acq')
    for r in (a, b):
        synth.write_acquisition(spec, r)
    moved = 0
    for folder, _, names in os.walk(b):
        for name in names:
            if name.endswith('.tiff'):
                img = tiffio.read_image(os.path.join(folder, name))
                if img.ndim == 3 and img.shape[2] == 3:
                    tiffio.write_tiff(os.path.join(folder, name), shift_ref.shift_file_image(img, [77, 0, -256], [-200, 0, 300]))
                    moved += 1
    assert moved == 4
    got, want = _api(a, channel_shifts=shifts), _api(b)
    _same_trees(got.output_folder, want.output_folder)


def _prepared_names(tmp_path, spec):
    root = str(tmp_path / 'names' / 'acq')
    synth.write_acquisition(spec, root)
    return _prepared(root).monochrome_channels


# ---------------------------------------------------------------------------------------------------- the launch order
RECORDED = ('warp_tiles', 'shift_tiles', 'bin_tiles', 'dpc_tiles', 'fuse_planes')


def _record(monkeypatch):
    """Wrap the chain's head and the fusion's entry points: their names in call order, the originals still called."""
    calls = []

    def wrap(name):
        original = getattr(native, name)

        def recorded(*args, **kw):
            calls.append(name)
            return original(*args, **kw)
        return recorded

    for name in RECORDED:
        monkeypatch.setattr(native, name, wrap(name))
    return calls


def _chunks(calls):
    chunks, run = [], []
    for name in calls:
        run.append(name)
        if name == 'fuse_planes':
            chunks.append(run)
            run = []
    assert not run, f"launches behind the last fusion: {run}"
    return chunks


def test_launch_order_with_every_head_option(tmp_path, monkeypatch):
    root = str(tmp_path / 'acq')
    synth.write_acquisition(synth.GridSpec(**dict(SPEC, channels=(LEFT, RIGHT, FLUO))), root)
    st = _prepared(root, batch_bytes_limit=1, distortion_correction=D, tile_binning=2, dpc=True, channel_shifts={FLUO: (77, -200)})
    calls = _record(monkeypatch)
    canvas, ids = st.stitch_planes(0, 'R0')
    fluo = st.monochrome_channels.index(FLUO)
    assert ids == list(range(8)) and st._dpc_index == 2 and fluo == 3
    # the head of every chunk: corrected, shifted only where the chunk holds a shifted plane, binned; the right halves of the
    # derived planes are corrected and binned, never shifted
    want = [['warp_tiles'] + (['shift_tiles'] if p // st.num_z == fluo else []) + ['bin_tiles'] +
            (['warp_tiles', 'bin_tiles', 'dpc_tiles'] if p // st.num_z == st._dpc_index else []) + ['fuse_planes'] for p in ids]
    assert _chunks(calls) == want
    assert calls.count('shift_tiles') == st.num_z
    keys = [k for k in st._buffer_cache if k[0] == 'shift']
    assert keys == [('shift', 1, 4, 64, 64, '<u2')]      # ONE buffer of the files' shape for both ingest slots
    assert canvas.cpu().numpy().any()


def test_launch_order_alone_and_off(tmp_path, monkeypatch):
    root = str(tmp_path / 'acq')
    synth.write_acquisition(synth.GridSpec(**SPEC), root)
    st = _prepared(root, batch_bytes_limit=1, channel_shifts={C561: (0, 256), C405: (0, 0)})
    assert st.channel_shifts == {C561: (0, 256)}
    calls = _record(monkeypatch)
    _, ids = st.stitch_planes(0, 'R0')
    last = st.monochrome_channels.index(C561)
    assert _chunks(calls) == [(['shift_tiles'] if p // st.num_z == last else []) + ['fuse_planes'] for p in ids]
    # off -- no option, an empty mapping, all-zero pairs: never called, no buffer, no note
    off_root = str(tmp_path / 'off' / 'acq')
    synth.write_acquisition(synth.GridSpec(**SPEC), off_root)
    for kw in ({}, dict(channel_shifts={}), dict(channel_shifts={C488: (0, 0)})):
        off = _prepared(off_root, batch_bytes_limit=1, **kw)
        del calls[:]
        off.stitch_planes(0, 'R0')
        assert calls == ['fuse_planes'] * 6
        assert [k[0] for k in off._buffer_cache] == ['ingest']
        assert not _notes(off.output_folder)


def test_a_whole_chunk_is_one_launch(tmp_path, monkeypatch):
    """All six planes in one chunk, two of them shifted: one shift launch over the chunk, which copies the other four."""
    a, b = _two_roots(tmp_path, shifts={C488: (77, -200)})
    st, plain = _prepared(a, channel_shifts={C488: (77, -200)}), _prepared(b)
    calls = _record(monkeypatch)
    canvas, ids = st.stitch_planes(0, 'R0')
    assert calls == ['shift_tiles', 'fuse_planes'] and len(ids) == 6
    want, _ = plain.stitch_planes(0, 'R0')
    assert bool((canvas == want).all())


# ---------------------------------------------------------------------------------------------------- refused with the metadata
def test_refusals_once_the_metadata_is_parsed(tmp_path):
    root = str(tmp_path / 'acq')
    synth.write_acquisition(synth.GridSpec(**SPEC), root)
    with pytest.raises(ValueError, match="'no such channel'.*not a channel"):
        _prepared(root, channel_shifts={'no such channel': (1, 1)})
    # with -r: the resolved registration channel -- named, defaulted, or an unknown name that falls back to the first
    for params in (dict(registration_channel=C488), dict(), dict(registration_channel='nothing')):
        reg = params.get('registration_channel', C405) if params.get('registration_channel') != 'nothing' else C405
        with pytest.raises(ValueError, match=f"'{reg}'.*registration channel"):
            _prepared(root, params=dict(use_registration=True, **params), channel_shifts={reg: (1, 0)})
        _prepared(root, params=dict(use_registration=True, **params), channel_shifts={reg: (0, 0), C561: (5, 5)})
    _prepared(root, channel_shifts={C405: (1, 0)})      # without -r no channel is the frame
    dpc_root = str(tmp_path / 'dpc' / 'acq')
    synth.write_acquisition(synth.GridSpec(**dict(SPEC, channels=(LEFT, RIGHT, FLUO))), dpc_root)
    for name in ('DPC', LEFT, RIGHT):
        with pytest.raises(ValueError, match=f"'{name}'.*--dpc"):
            _prepared(dpc_root, dpc=True, channel_shifts={name: (1, 0)})
    _prepared(dpc_root, dpc=True, channel_shifts={FLUO: (1, 0)})
    _prepared(dpc_root, channel_shifts={LEFT: (1, 0)})      # without --dpc the halves are channels like any other
    for bad in ({C488: (1.0, 2)}, {C488: (True, 2)}, {C488: (16385, 0)}, {C488: '12'}):
        with pytest.raises(ValueError):
            Stitcher(StitchingParameters(input_folder=root), channel_shifts=bad)
    with pytest.raises(SystemExit):
        stitcher_cli.main(['-i', root, '--channel-shift', C488, '1', '1', '--channel-shift', C488, '2', '2'])


# ---------------------------------------------------------------------------------------------------- finding the shifts
def test_scan_tool_measures_a_displaced_channel_and_its_result_undoes_it(tmp_path, capsys):
    """The second channel is the first one displaced by (3, -2) px -- a point at (y, x) of the first lies at (y + 3, x - 2) of
    the second; made with the definition at S = (-768, 512).  The tool prints (3, -2) within one step of its resolution, and a
    run with that line makes the two channels' planes equal away from a 4-pixel border of every tile."""
    mod_spec = importlib.util.spec_from_file_location('channel_shift_scan', os.path.join(ROOT, 'tools', 'channel_shift_scan.py'))
    tool = importlib.util.module_from_spec(mod_spec)
    mod_spec.loader.exec_module(tool)
    spec = synth.GridSpec(rows=2, cols=2, tile_h=128, tile_w=160, ov_y=36, ov_x=44, channels=(C405, C488), seed=43)
    root = str(tmp_path / 'acq')
    synth.write_acquisition(spec, root)
    n = 0
    for folder, _, names in os.walk(root):
        for name in names:
            if name.endswith('.tiff') and _channel_of(name) == C488:
                first = tiffio.read_image(os.path.join(folder, name.replace(C488.replace(' ', '_'), C405.replace(' ', '_'))))
                tiffio.write_tiff(os.path.join(folder, name), shift_ref.shift_image(first, -768, 512))
                n += 1
    assert n == 4
    capsys.readouterr()
    rows = tool.main(['-i', root, '--reference', C405, '--fovs', '3'])
    printed = capsys.readouterr().out
    assert len(rows) == 1
    name, dy, dx, agree, fields = rows[0]
    assert name == C488 and fields == 3 and agree == 3
    assert abs(dy - 3) <= 0.1 + 1e-9 and abs(dx + 2) <= 0.1 + 1e-9, (dy, dx)
    line = f'--channel-shift "{C488}" {dy:.1f} {dx:.1f}'
    assert line in printed and 'beads, brightfield' in printed
    st = _prepared(root, channel_shifts={C488: (channelshift.parse_pixels(f'{dy:.1f}'), channelshift.parse_pixels(f'{dx:.1f}'))})
    canvas, ids = st.stitch_planes(0, 'R0')
    planes = canvas.cpu().numpy()
    assert len(ids) == 2
    # every canvas pixel that any tile covers with its 4-pixel border is left out
    bad = np.zeros(planes.shape[1:], bool)
    inner = np.zeros((128, 160), bool)
    inner[4:-4, 4:-4] = True
    for info in st.get_region_data(0, 'R0').values():
        sy, sx, h, w, y, x = (int(v) for v in st._tile_rect(info))
        bad[y:y + h, x:x + w] |= ~inner[sy:sy + h, sx:sx + w]
    assert (~bad).mean() > 0.6
    assert (planes[0][~bad] == planes[1][~bad]).all() and planes[0][~bad].any()
    # ... and without the option they differ there
    plain, _ = _prepared(root).stitch_planes(0, 'R0')
    plain = plain.cpu().numpy()
    assert (plain[0][~bad] != plain[1][~bad]).mean() > 0.5
