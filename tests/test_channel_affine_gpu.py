"""--channel-affine on the device: sq_affine_tiles against the numpy definition (tests/affine_ref.py), and whole runs with the
option against runs without it on a folder whose files of the mapped channels were transformed beforehand.  Every comparison is
equality, but the scan tool's measurement (whose bounds the test states)."""
import hashlib
import importlib.util
import json
import os
import random

import numpy as np
import pytest

import affine_cases
import affine_ref
import bin_ref
import shift_cases
import stream_cases as SC
import warp_ref
from image_stitcher_amd import channelshift, native, stitcher_cli, synth, tiffio
from image_stitcher_amd.stitcher import Stitcher
from image_stitcher_amd.stitcher_parameters import StitchingParameters

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZERO = affine_cases.ZERO
ROT1 = affine_cases.PARAMS[2]       # rotation by 1 degree
ROT02 = affine_cases.PARAMS[3]      # rotation by -0.2 degree with +0.3 %, and a shift
LARGEST = affine_cases.PARAMS[-2]


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the cached planes are read-only)


def _full(shape, value, dtype):
    return _dev(np.full(shape, value, dtype=np.dtype(dtype)))


def _six(s, a):
    return tuple(s) + tuple(a)


# ---------------------------------------------------------------------------------------------------- the kernel
# (the shapes and the kernel's own sizes they are chosen from: tests/affine_cases.py)
@pytest.mark.parametrize('dtype', affine_cases.DTYPES)
@pytest.mark.parametrize('case', range(len(affine_cases.PARAMS)))
def test_kernel_equals_the_definition(case, dtype):
    s, a = affine_cases.PARAMS[case]
    for h, w in affine_cases.shapes(dtype):
        planes = affine_cases.planes(dtype, h, w)
        src = _dev(planes)
        want = affine_cases.reference(dtype, h, w, s, a)
        got = native.affine_tiles(src, _six(s, a))
        assert got.dtype == src.dtype and tuple(got.shape) == planes.shape
        host = got.cpu().numpy()
        for i, name in enumerate(affine_cases.PLANE_NAMES):
            np.testing.assert_array_equal(host[i], want[i], err_msg=f'{(h, w)} S={s} A={a} {name}')
        np.testing.assert_array_equal(src.cpu().numpy(), planes)      # the source is left as it was
        if (s, a) == ((0, 0), ZERO):
            np.testing.assert_array_equal(host, planes)                # the identity


@pytest.mark.parametrize('dtype', affine_cases.DTYPES)
def test_grid_edges(dtype):
    """Two planes at the three edges of the strip / segment grid: narrower than one vector; one vector more than a workgroup is
    wide (two strips); and, at that width, one row more than a workgroup's rows (two segments)."""
    wide = affine_cases.STRIP[dtype] + affine_cases.VEC[dtype]
    for h, w in ((3, 5), (3, wide), (affine_cases.ROWS + 1, wide)):
        planes = affine_cases.planes(dtype, h, w, 2)
        got = native.affine_tiles(_dev(planes), _six(*ROT02)).cpu().numpy()
        np.testing.assert_array_equal(got, affine_cases.reference(dtype, h, w, *ROT02, 2), err_msg=f'{(h, w)}')


@pytest.mark.parametrize('dtype', affine_cases.DTYPES)
def test_a_table_of_tuples_with_several_runs(dtype):
    h, w, n = affine_cases.MANY
    assert h > affine_cases.ROWS and n == affine_cases.WALK + 1
    planes = affine_cases.planes(dtype, h, w, n)
    # runs of equal tuples: two mapped planes, two zero, eleven of another map, one shifted only, one of the first map again
    # (seventeen planes, five grids; no run ends where a thread's walk over 16 planes would)
    table = [_six(*ROT02)] * 2 + [(0,) * 6] * 2 + [_six(*ROT1)] * 11 + [_six(affine_cases.MIXED, ZERO)] + [_six(*ROT02)]
    got = native.affine_tiles(_dev(planes), table).cpu().numpy()
    for i, t in enumerate(table):
        np.testing.assert_array_equal(got[i], affine_cases.reference(dtype, h, w, t[:2], t[2:], n)[i], err_msg=f'plane {i} {t}')
    np.testing.assert_array_equal(got[2], planes[2])
    # one tuple for all seventeen planes: a walk of sixteen and a walk of one
    got = native.affine_tiles(_dev(planes), _six(*LARGEST)).cpu().numpy()
    np.testing.assert_array_equal(got, affine_cases.reference(dtype, h, w, *LARGEST, n))
    # a stack with two leading dimensions: one tuple per index of the first, for all planes under it
    stack = _dev(planes[:6].reshape(2, 3, h, w))
    tuples = [(0,) * 6, _six(*ROT1)]
    got = native.affine_tiles(stack, tuples).cpu().numpy()
    np.testing.assert_array_equal(got[0], planes[:3])
    np.testing.assert_array_equal(got[1], affine_cases.reference(dtype, h, w, *ROT1, n)[3:6])
    # ... and one tuple for every plane of it; numpy integers are taken
    got = native.affine_tiles(stack, tuple(np.int64(v) for v in _six(*ROT1))).cpu().numpy().reshape(6, h, w)
    np.testing.assert_array_equal(got, affine_cases.reference(dtype, h, w, *ROT1, n)[:6])
    good = _six(*ROT1)
    for bad in ([good], [good] * 3, [good, good[:5]], [good, (1.0,) + good[1:]], 5, None, [good, (True,) + good[1:]], good[:5]):
        with pytest.raises(ValueError):
            native.affine_tiles(stack, bad)


def test_more_planes_than_one_launch_takes():
    """65535 walks of 16 planes go into one grid: sixteen planes more, of 1 x 1 pixels, through the C entry -- as one run, and as
    a table whose runs end inside a launch and at the split."""
    import ctypes
    import torch
    per_launch = 65535 * affine_cases.WALK
    n = per_launch + 16
    assert n == 1 << 20
    src = torch.arange(n, dtype=torch.int32, device=DEV).remainder(251).to(torch.uint8)
    out = torch.full((2 * n,), 255, dtype=torch.uint8, device=DEV)
    L = native.lib()
    one = (ctypes.c_int32 * 6)(16384, -16384, 50000, -50000, 50000, -50000)
    assert L.sq_affine_tiles(src.data_ptr(), out.data_ptr(), n, 1, 1, 1, 1, 1, 1, native.SQ_U8, one, n, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:n], src) and bool((out[n:] == 255).all())      # 1 x 1: the identity, plane for plane
    out.fill_(255)
    # four tuples of 2^18 planes each: the run of the two equal ones ends inside a launch
    table = (ctypes.c_int32 * 24)(0, 0, 0, 0, 0, 0, 77, -200, 1, 2, 3, 4, 77, -200, 1, 2, 3, 4, 0, 0, 0, 0, 0, 0)
    assert L.sq_affine_tiles(src.data_ptr(), out.data_ptr(), n, 1, 1, 1, 1, 1, 1, native.SQ_U8, table, n // 4, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:n], src) and bool((out[n:] == 255).all())
    # two columns: the half-pixel blend of every plane's pair, and its replicated edge
    pairs = torch.arange(2 * n, dtype=torch.int32, device=DEV).remainder(241).to(torch.uint8)
    out.fill_(255)
    half = (ctypes.c_int32 * 6)(0, 128, 0, 0, 0, 0)
    assert L.sq_affine_tiles(pairs.data_ptr(), out.data_ptr(), n, 1, 2, 2, 2, 2, 2, native.SQ_U8, half, n, None) == 0
    torch.cuda.synchronize()
    a, b = pairs[0::2].to(torch.int32), pairs[1::2].to(torch.int32)
    want = torch.stack([(a + b + 1) >> 1, b], dim=1).to(torch.uint8).reshape(-1)
    assert affine_ref.loop(np.array([[10, 201]], np.uint8), (0, 128), ZERO).tolist() == [[106, 201]]
    assert torch.equal(out, want)


@pytest.mark.parametrize('dtype', affine_cases.DTYPES)
@pytest.mark.parametrize('params', [ROT02, ((-300, 16384), (-50000, 50000, 50000, -50000))])
def test_views_pitches_offsets_guard_and_repeatability(params, dtype):
    import torch
    h, w = 9, 37
    six = _six(*params)
    planes = affine_cases.planes(dtype, h, w)
    n_planes = len(planes)
    tdtype = native.torch_dtype_of(np.dtype(dtype))
    fill = int(np.iinfo(np.dtype(dtype)).max) // 3
    want = affine_cases.reference(dtype, h, w, *params)
    # every other plane of a stack, as source and as destination; the planes between stay as they are
    big = _dev(planes)
    out_big = _full((n_planes + 1, h, w), fill, dtype)
    got = native.affine_tiles(big[::2], six, out=out_big[1::2])
    assert got.data_ptr() == out_big[1::2].data_ptr()
    np.testing.assert_array_equal(out_big.cpu().numpy()[1::2], want[::2])
    assert (out_big.cpu().numpy()[::2] == fill).all()
    np.testing.assert_array_equal(big.cpu().numpy(), planes)
    # a pitched source and a pitched destination: the columns beyond w of dst stay as they are
    wide_src = _dev(np.concatenate([planes, np.full((n_planes, h, 5), 7, planes.dtype)], axis=2))
    wide_dst = _full((n_planes, h, w + 3), fill, dtype)
    native.affine_tiles(wide_src[:, :, :w], six, out=wide_dst[:, :, :w])
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
            got = native.affine_tiles(src_off, six, out=out_off[:, :, :w])
            np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f'src offset {s_off}, dst offset {d_off}')
            host = obuf.cpu().numpy()
            assert (host[:d_off] == fill).all() and (host[n_el + d_off:] == fill).all()
            assert (host[d_off:n_el + d_off].reshape(n_planes, h, pitch)[:, :, w:] == fill).all()      # between w and the pitch
    np.testing.assert_array_equal(buf[s_off:n_el + s_off].cpu().numpy(), padded.reshape(-1))
    # a plane stride that is no multiple of 16 bytes: rows on a boundary in one plane are off it in the next
    odd = _full((n_planes * (h * w + 1),), fill, dtype)
    odd_out = odd.as_strided((n_planes, h, w), (h * w + 1, w, 1))
    native.affine_tiles(_dev(planes), six, out=odd_out)
    np.testing.assert_array_equal(odd_out.cpu().numpy(), want)
    assert (odd.cpu().numpy().reshape(n_planes, h * w + 1)[:, -1] == fill).all()
    # a guard band of 0xA5 in front of and behind out stays intact
    nbytes = want.size * planes.itemsize
    raw = torch.full((4096 + nbytes + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    out = raw[4096:4096 + nbytes].view(tdtype).view(n_planes, h, w)
    native.affine_tiles(_dev(planes), six, out=out)
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    assert bool((raw[:4096] == 0xA5).all()) and bool((raw[4096 + nbytes:] == 0xA5).all())
    # the same call twice: the same bytes
    runs = [native.affine_tiles(_dev(planes), six).cpu().numpy().tobytes() for _ in range(2)]
    assert runs[0] == runs[1] == want.tobytes()


@pytest.mark.parametrize('dtype', affine_cases.DTYPES)
def test_zero_coefficients_equal_shift_tiles(dtype):
    import torch
    for h, w in ((37, 53), (affine_cases.ROWS + 1, affine_cases.STRIP[dtype] + 1), (5, affine_cases.VEC[dtype] + 1), (1, 300), (300, 1)):
        src = _dev(shift_cases.planes(dtype, h, w))
        for shift in shift_cases.SHIFTS:
            assert torch.equal(native.affine_tiles(src, _six(shift, ZERO)), native.shift_tiles(src, shift)), ((h, w), shift)


def test_refusals():
    import ctypes
    import torch
    t_np = np.arange(3 * 8 * 12, dtype=np.uint16).reshape(3, 8, 12)
    t = _dev(t_np)
    out = _full((3, 8, 12), 7, 'uint16')
    good = _six(*ROT02)
    for bad in ((16385, 0, 0, 0, 0, 0), (0, -16385, 0, 0, 0, 0), (0, 0, 50001, 0, 0, 0), (0, 0, 0, 0, 0, -50001), (2.0,) + good[1:],
                (True,) + good[1:], (None,) + good[1:], ('2',) + good[1:], good[:2] + (1.5,) + good[3:], good[:2], good + (0,)):
        with pytest.raises(ValueError):
            native.affine_tiles(t, bad, out=out)
    with pytest.raises(ValueError):
        native.affine_tiles(t.to(torch.float32), good, out=out)                       # a wrong dtype
    with pytest.raises(ValueError):
        native.affine_tiles(t.permute(0, 2, 1), good)                                 # rows that are not contiguous
    with pytest.raises(ValueError):
        native.affine_tiles(t, good, out=out[:2])                                     # another shape
    with pytest.raises(ValueError):
        native.affine_tiles(t, good, out=_full((3, 8, 12), 7, 'uint8'))               # another dtype
    with pytest.raises(ValueError):
        native.affine_tiles(t, good, out=torch.zeros((3, 8, 12), dtype=torch.uint16))             # another device
    assert (out.cpu().numpy() == 7).all()      # nothing was launched
    # an out that shares memory with tiles
    before = t.cpu().numpy()
    for src, dst in ((t, t), (t[:2], t[1:]), (t[::2], t[1:3])):
        with pytest.raises(ValueError, match='out of place'):
            native.affine_tiles(src, good, out=dst)
    np.testing.assert_array_equal(t.cpu().numpy(), before)
    # the library itself refuses what the wrapper would let through, with its own message
    L = native.lib()
    triple = (ctypes.c_int32 * 18)(*(good * 3))

    def six(*values):
        return (ctypes.c_int32 * 6)(*values)

    def call(src=t.data_ptr(), dst=out.data_ptr(), n=3, h=8, w=12, sps=96, sp=12, dps=96, dp=12, dtype=native.SQ_U16, table=triple,
             per=3):
        return L.sq_affine_tiles(src, dst, n, h, w, sps, sp, dps, dp, dtype, table, per, None)

    assert call() == 0 and call(per=1) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), affine_ref.affine_image(t_np, *ROT02))
    assert call(table=six(0, 0, 0, 0, 0, 0)) == 0                        # all zero is accepted: an exact copy
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), t_np)
    assert call(table=six(-16384, 16384, 50000, -50000, -50000, 50000)) == 0      # the ranges' ends are inside
    torch.cuda.synchronize()
    out.copy_(_full((3, 8, 12), 7, 'uint16'))
    torch.cuda.synchronize()
    assert call(n=0) == 0 and call(n=0, src=None, dst=None, table=None) == 0      # no image: SQ_OK, nothing launched
    for bad in (dict(table=six(16385, 0, 0, 0, 0, 0)), dict(table=six(0, -16385, 0, 0, 0, 0)), dict(table=six(0, 0, 50001, 0, 0, 0)),
                dict(table=six(0, 0, 0, -50001, 0, 0)), dict(table=six(0, 0, 0, 0, 50001, 0)), dict(table=six(0, 0, 0, 0, 0, -50001)),
                dict(table=None),
                dict(per=2), dict(per=0), dict(per=-1), dict(dtype=native.SQ_F32), dict(dtype=0), dict(sp=11), dict(dp=11),
                dict(sps=95), dict(dps=95), dict(src=None), dict(dst=None), dict(src=t.data_ptr() + 1),
                dict(dst=out.data_ptr() + 1), dict(n=-1), dict(dst=t.data_ptr() + 96 * 2), dict(dst=t.data_ptr()),
                dict(src=out.data_ptr(), n=1, per=1), dict(h=0), dict(w=0), dict(h=-1)):
        assert call(**bad) == -1, bad      # SQ_ERR_INVALID
    assert call(dst=t.data_ptr()) == -1 and 'overlap' in L.sq_last_error().decode()
    assert call(table=six(0, 0, 0, 0, 50001, 0)) == -1 and '50000' in L.sq_last_error().decode()
    assert call(table=six(16385, 0, 0, 0, 0, 0)) == -1 and '16384' in L.sq_last_error().decode()
    for big in (dict(h=65536, sps=65536 * 12, dps=65536 * 12), dict(w=65536, sp=65536, dp=65536, sps=8 * 65536, dps=8 * 65536)):
        assert call(**big) == native.SQ_ERR_UNSUPPORTED, big
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7).all()
    np.testing.assert_array_equal(t.cpu().numpy(), before)


# ---------------------------------------------------------------------------------------------------- off the default stream
def _stream_call(tuples):
    def call(ctx, inp, out, stream):
        native.affine_tiles(inp['tiles'], tuples, out=out['out'], stream=stream)
        return {'out': out['out']}
    return call


def _stream_case(dtype, tuples):
    top = int(np.iinfo(dtype).max)
    shape = (4, 50, 70)
    real = {'tiles': np.random.default_rng(510).integers(0, top + 1, shape).astype(dtype)}
    poison = {'tiles': np.random.default_rng(511).integers(0, top + 1, shape).astype(dtype)}
    canary = {'out': np.full(shape, 7, dtype)}
    return SC.Case(f'affine-tiles-{np.dtype(dtype).name}', real, poison, canary, _stream_call(tuples),
                   lambda a, strict: {'out': np.stack([affine_ref.affine_image(p, t[:2], t[2:]) for p, t in zip(a['tiles'], tuples)])})


STREAM_CASES = {c.name: c for c in (_stream_case(np.uint16, [_six(*ROT02), _six(*ROT02), (0,) * 6, _six(*ROT1)]),
                                    _stream_case(np.uint8, [_six(*LARGEST)] * 4))}


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
NOTE, SHIFT_NOTE = '_stitched_channel_affine.json', '_stitched_channel_shift.json'
WARP_NOTE, BIN_NOTE = '_stitched_distortion.json', '_stitched_binning.json'
LEFT, RIGHT, FLUO = 'BF LED matrix left half', 'BF LED matrix right half', 'Fluorescence 488 nm Ex'
C405, C488, C561 = synth.DEFAULT_CHANNELS[:3]
# a synthetic 2 x 2 grid of 64 x 64 tiles with two z levels and three channels; the first channel is the registration channel.
# Coefficients of a few 10^4 ppm: below 63 ppm nothing moves on a tile of 64 x 64.  One channel has a shift and an affine, one an
# affine alone.
SPEC = dict(rows=2, cols=2, tile_h=64, tile_w=64, ov_y=24, ov_x=24, nz=2, channels=(C405, C488, C561), seed=37)
SHIFTS = {C488: (77, -200)}
AFFINES = {C488: (20000, -30000, 30000, 20000), C561: (-15000, 40000, 0, 25000)}
FLAGS = ['--channel-shift', C488, '0.3', '-0.78125', '--channel-affine', C488, '20000', '-30000', '30000', '20000',
         '--channel-affine', C561, '-15000', '40000', '0', '25000']
D = 20000


def _channel_of(name):
    return os.path.splitext(name.split('_', 3)[3])[0].replace('_', ' ')


def premake_folder(root, shifts, affines, ppm=0, then_bin=1):
    """F -> F' in place: every tile file corrected by its definition (ppm), the files of the channels of ``shifts`` and
    ``affines`` mapped by the definition (one map of both), and then, for the run with --tile-binning too, binned by its
    definition, the sensor pixel multiplied."""
    moved = 0
    for folder, _, names in os.walk(root):
        for name in names:
            if name.lower().endswith(('.tif', '.tiff')):
                path = os.path.join(folder, name)
                img = tiffio.read_image(path)
                new = warp_ref.warp_file_image(img, ppm) if ppm else img
                channel = _channel_of(name)
                if channel in shifts or channel in affines:
                    before = new
                    new = affine_ref.affine_file_image(new, shifts.get(channel, (0, 0)), affines.get(channel, ZERO))
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


def _two_roots(tmp_path, spec=None, shifts=SHIFTS, affines=AFFINES, ppm=0, then_bin=1):
    spec = spec or synth.GridSpec(**SPEC)
    a, b = str(tmp_path / 'with_flag' / 'acq'), str(tmp_path / 'premade' / 'acq')
    for r in (a, b):
        synth.write_acquisition(spec, r)
    premake_folder(b, shifts, affines, ppm, then_bin)
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


def _tree(out, skip=(NOTE, SHIFT_NOTE)):
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


def _same_trees(got, want, skip=(NOTE, SHIFT_NOTE)):
    a, b = _tree(got, skip), _tree(want, skip)
    assert a and sorted(a) == sorted(b)
    differ = [k for k in a if a[k] != b[k]]
    assert not differ, differ[:10]
    assert any('.ome.zarr' in k and not os.path.basename(k).startswith('.') for k in a) or any(k.endswith('.ome.tiff') for k in a)
    assert _notes(got) and not _notes(want) and not _notes(want, SHIFT_NOTE)
    return a


@pytest.mark.parametrize('fmt', ['.ome.zarr', '.ome.tiff'])
def test_flag_on_f_equals_no_flag_on_f_prime(tmp_path, capsys, fmt):
    a, b = _two_roots(tmp_path)
    capsys.readouterr()
    got = _cli(a, '-f', fmt, *FLAGS)
    printed = capsys.readouterr().out
    assert printed.count('[channel-affine]') == 1 and printed.count('[channel-shift]') == 1
    want = _cli(b, '-f', fmt)
    printed = capsys.readouterr().out
    assert '[channel-affine]' not in printed and '[channel-shift]' not in printed
    _same_trees(got, want)
    assert _notes(got) == [os.path.join('0_stitched', 'R0' + NOTE)]
    with open(os.path.join(got, '0_stitched', 'R0' + NOTE)) as fh:
        note = json.load(fh)
    assert sorted(note['channels']) == [C488, C561]
    assert note['channels'][C488]['affine_ppm'] == [20000, -30000, 30000, 20000] and note['channels'][C488]['shift_256'] == [77, -200]
    assert note['channels'][C561]['affine_ppm'] == [-15000, 40000, 0, 25000] and note['channels'][C561]['shift_256'] == [0, 0]
    for name in (C488, C561):
        dv, du, _, _ = affine_ref.maps(64, 64, SHIFTS.get(name, (0, 0)), AFFINES[name])
        assert note['channels'][name]['max_abs_dv_256'] == int(np.abs(dv).max())
        assert note['channels'][name]['max_abs_du_256'] == int(np.abs(du).max())
    assert note['tile_shape'] == [64, 64]
    # the shift's own note is what a run with --channel-shift alone writes, byte for byte
    alone = str(tmp_path / 'shift_alone' / 'acq')
    synth.write_acquisition(synth.GridSpec(**SPEC), alone)
    shift_only = _cli(alone, '-f', fmt, *FLAGS[:4])
    assert not _notes(shift_only) and _notes(shift_only, SHIFT_NOTE) == _notes(got, SHIFT_NOTE) != []
    for rel in _notes(got, SHIFT_NOTE):
        with open(os.path.join(got, rel), 'rb') as f1, open(os.path.join(shift_only, rel), 'rb') as f2:
            assert f1.read() == f2.read()
    # ... and the run on F without the flags is another tree
    third = str(tmp_path / 'plain' / 'acq')
    synth.write_acquisition(synth.GridSpec(**SPEC), third)
    plain = _tree(_cli(third, '-f', fmt))
    assert sorted(plain) == sorted(_tree(got)) and plain != _tree(got) and plain != _tree(shift_only)


@pytest.mark.parametrize('mode', ['overwrite', 'feather'])
def test_registration_and_device_basic_flatfield(tmp_path, mode):
    """-r -ff: the registration channel is the frame and takes no map; the flatfield estimate's samples and get_tile map on
    the host with the same arithmetic."""
    a, b = _two_roots(tmp_path)
    flags = ('-r', '-ff', '--flatfield-estimator', 'basic', '--fusion-mode', mode)
    tree = _same_trees(_cli(a, *flags, *FLAGS), _cli(b, *flags))
    assert 'shift_table.json' in tree and 'flatfield_info.json' in tree
    st_a, st_b = _prepared(a, channel_shifts=SHIFTS, channel_affines=AFFINES), _prepared(b)
    plain = _prepared(a)
    for channel in (C405, C488, C561):
        info = next(v for v in st_a.get_region_data(0, 'R0').values() if v['channel'] == channel and v['z_level'] == 1)
        got = st_a.get_tile(0, 'R0', info['x'], info['y'], channel, 1)
        np.testing.assert_array_equal(got, st_b.get_tile(0, 'R0', info['x'], info['y'], channel, 1))
        assert (got != plain.get_tile(0, 'R0', info['x'], info['y'], channel, 1)).any() == (channel != C405)


def test_with_distortion_correction_and_binning(tmp_path):
    """Correct, shift + affine, bin, all in sensor pixels: a run on bin_2(affine(warp(F)))."""
    a, b = _two_roots(tmp_path, ppm=D, then_bin=2)
    flags = ('--z-projection', 'max', '--composite')
    got = _cli(a, '--distortion-correction', str(D), '--tile-binning', '2', *flags, *FLAGS)
    want = _cli(b, *flags)
    tree = _same_trees(got, want, skip=(NOTE, SHIFT_NOTE, WARP_NOTE, BIN_NOTE))
    assert any('_mip' in k for k in tree) and any(k.endswith('.png') for k in tree)
    assert _notes(got, WARP_NOTE) and _notes(got, BIN_NOTE)


def test_with_tile_qc_and_seam_qc(tmp_path):
    a, b = _two_roots(tmp_path)
    kw = dict(tile_qc=True, seam_qc=True, seam_qc_min_pixels=16)
    got, want = _api(a, channel_shifts=SHIFTS, channel_affines=AFFINES, **kw), _api(b, **kw)
    tree = _same_trees(got.output_folder, want.output_folder)
    for part in ('_tile_qc.csv', '_tile_qc.json', '_seam_qc.csv', '_seam_qc.json'):
        assert any(part in k for k in tree), part
    assert got.tile_qc_table and got.tile_qc_table == want.tile_qc_table      # the report describes F''s files
    assert got.seam_qc_table and got.seam_qc_table == want.seam_qc_table


def test_uint8_rgb_files(tmp_path):
    """The names come out of the output channels: <base>_R, <base>_G, <base>_B, each with tuples of its own."""
    spec = synth.GridSpec(rows=2, cols=2, tile_h=64, tile_w=64, ov_y=24, ov_x=24, channels=('BF LED matrix full_RGB', C488),
                          rgb_channels=('BF LED matrix full_RGB',), dtype='uint8', seed=41)
    names = _prepared_names(tmp_path, spec)
    base = [n for n in names if n.endswith('_R')][0][:-2]
    # R: a shift and an affine; G: a shift alone, which rides in the file's one map; B: an affine alone
    shifts = {f'{base}_R': (77, -200), f'{base}_G': (-256, 300)}
    affines = {f'{base}_R': (20000, -30000, 30000, 20000), f'{base}_B': (0, 40000, -40000, 0)}
    a, b = str(tmp_path / 'with_flag' / 'acq'), str(tmp_path / 'premade' / 'acq')
    for r in (a, b):
        synth.write_acquisition(spec, r)
    moved = 0
    for folder, _, files in os.walk(b):
        for name in files:
            if name.endswith('.tiff'):
                img = tiffio.read_image(os.path.join(folder, name))
                if img.ndim == 3 and img.shape[2] == 3:
                    new = affine_ref.affine_file_image(img, [(77, -200), (-256, 300), (0, 0)],
                                                       [(20000, -30000, 30000, 20000), ZERO, (0, 40000, -40000, 0)])
                    assert all((new[:, :, c] != img[:, :, c]).any() for c in range(3))
                    tiffio.write_tiff(os.path.join(folder, name), new)
                    moved += 1
    assert moved == 4
    got, want = _api(a, channel_shifts=shifts, channel_affines=affines), _api(b)
    _same_trees(got.output_folder, want.output_folder)


def _prepared_names(tmp_path, spec):
    root = str(tmp_path / 'names' / 'acq')
    synth.write_acquisition(spec, root)
    return _prepared(root).monochrome_channels


# ---------------------------------------------------------------------------------------------------- the launch order
RECORDED = ('warp_tiles', 'shift_tiles', 'affine_tiles', 'bin_tiles', 'dpc_tiles', 'fuse_planes')


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
    st = _prepared(root, batch_bytes_limit=1, distortion_correction=D, tile_binning=2, dpc=True, channel_shifts={FLUO: (77, -200)},
                   channel_affines={FLUO: AFFINES[C488]})
    calls = _record(monkeypatch)
    canvas, ids = st.stitch_planes(0, 'R0')
    fluo = st.monochrome_channels.index(FLUO)
    assert ids == list(range(8)) and st._dpc_index == 2 and fluo == 3
    # the head of every chunk: corrected, mapped only where the chunk holds a plane with an affine (never shift_tiles there),
    # binned; the right halves of the derived planes are corrected and binned, never mapped
    want = [['warp_tiles'] + (['affine_tiles'] if p // st.num_z == fluo else []) + ['bin_tiles'] +
            (['warp_tiles', 'bin_tiles', 'dpc_tiles'] if p // st.num_z == st._dpc_index else []) + ['fuse_planes'] for p in ids]
    assert _chunks(calls) == want
    assert calls.count('affine_tiles') == st.num_z and 'shift_tiles' not in calls
    keys = [k for k in st._buffer_cache if k[0] == 'shift']
    assert keys == [('shift', 1, 4, 64, 64, '<u2')]      # ONE buffer of the files' shape for both ingest slots and both options
    assert canvas.cpu().numpy().any()


def test_launch_order_alone_and_off(tmp_path, monkeypatch):
    root = str(tmp_path / 'acq')
    synth.write_acquisition(synth.GridSpec(**SPEC), root)
    # one channel with a shift alone, one with an affine alone, one with neither; an all-zero entry is dropped
    st = _prepared(root, batch_bytes_limit=1, channel_shifts={C488: (0, 256)}, channel_affines={C561: AFFINES[C561], C405: ZERO})
    assert st.channel_affines == {C561: AFFINES[C561]}
    calls = _record(monkeypatch)
    _, ids = st.stitch_planes(0, 'R0')
    head = {st.monochrome_channels.index(C488): ['shift_tiles'], st.monochrome_channels.index(C561): ['affine_tiles']}
    assert _chunks(calls) == [head.get(p // st.num_z, []) + ['fuse_planes'] for p in ids]      # shift_tiles as today
    assert [k for k in st._buffer_cache if k[0] == 'shift'] == [('shift', 1, 4, 64, 64, '<u2')]
    # an affine alone allocates the buffer too
    only = _prepared(root, batch_bytes_limit=1, channel_affines={C561: AFFINES[C561]})
    del calls[:]
    only.stitch_planes(0, 'R0')
    assert calls.count('affine_tiles') == only.num_z and 'shift_tiles' not in calls
    assert [k[0] for k in only._buffer_cache] == ['ingest', 'shift']
    # off -- no option, an empty mapping, all-zero coefficients: never called, no buffer, no note
    off_root = str(tmp_path / 'off' / 'acq')
    synth.write_acquisition(synth.GridSpec(**SPEC), off_root)
    for kw in ({}, dict(channel_affines={}), dict(channel_affines={C488: ZERO}), dict(channel_affines=None)):
        off = _prepared(off_root, batch_bytes_limit=1, **kw)
        del calls[:]
        off.stitch_planes(0, 'R0')
        assert calls == ['fuse_planes'] * 6
        assert [k[0] for k in off._buffer_cache] == ['ingest']
        assert not _notes(off.output_folder) and not _notes(off.output_folder, SHIFT_NOTE)


def test_a_whole_chunk_is_one_launch(tmp_path, monkeypatch):
    """All six planes in one chunk, two of them shifted only and two mapped: ONE affine launch over the chunk, which shifts the
    first two and copies the other two, and no shift launch."""
    shifts, affines = {C488: (77, -200)}, {C561: AFFINES[C561]}
    a, b = _two_roots(tmp_path, shifts=shifts, affines=affines)
    st, plain = _prepared(a, channel_shifts=shifts, channel_affines=affines), _prepared(b)
    calls = _record(monkeypatch)
    canvas, ids = st.stitch_planes(0, 'R0')
    assert calls == ['affine_tiles', 'fuse_planes'] and len(ids) == 6
    want, _ = plain.stitch_planes(0, 'R0')
    assert bool((canvas == want).all())


# ---------------------------------------------------------------------------------------------------- refused with the metadata
def test_refusals_once_the_metadata_is_parsed(tmp_path):
    root = str(tmp_path / 'acq')
    synth.write_acquisition(synth.GridSpec(**SPEC), root)
    one = (1000, 0, 0, 0)
    with pytest.raises(ValueError, match="'no such channel'.*not a channel"):
        _prepared(root, channel_affines={'no such channel': one})
    # with -r: the resolved registration channel -- named, defaulted, or an unknown name that falls back to the first
    for params in (dict(registration_channel=C488), dict(), dict(registration_channel='nothing')):
        reg = params.get('registration_channel', C405) if params.get('registration_channel') != 'nothing' else C405
        with pytest.raises(ValueError, match=f"'{reg}'.*registration channel"):
            _prepared(root, params=dict(use_registration=True, **params), channel_affines={reg: one})
        _prepared(root, params=dict(use_registration=True, **params), channel_affines={reg: ZERO, C561: one})
    _prepared(root, channel_affines={C405: one})      # without -r no channel is the frame
    dpc_root = str(tmp_path / 'dpc' / 'acq')
    synth.write_acquisition(synth.GridSpec(**dict(SPEC, channels=(LEFT, RIGHT, FLUO))), dpc_root)
    for name in ('DPC', LEFT, RIGHT):
        with pytest.raises(ValueError, match=f"'{name}'.*--dpc"):
            _prepared(dpc_root, dpc=True, channel_affines={name: one})
    _prepared(dpc_root, dpc=True, channel_affines={FLUO: one})
    _prepared(dpc_root, channel_affines={LEFT: one})      # without --dpc the halves are channels like any other
    for bad in ({C488: (1.0, 2, 3, 4)}, {C488: (True, 2, 3, 4)}, {C488: (50001, 0, 0, 0)}, {C488: '1234'}, {C488: (1, 2)}):
        with pytest.raises(ValueError):
            Stitcher(StitchingParameters(input_folder=root), channel_affines=bad)
    with pytest.raises(SystemExit):
        stitcher_cli.main(['-i', root, '--channel-affine', C488, '1', '1', '1', '1', '--channel-affine', C488, '2', '2', '2', '2'])
    with pytest.raises(SystemExit):
        stitcher_cli.main(['-i', root, '--channel-affine', C488, '1.5', '1', '1', '1'])


# ---------------------------------------------------------------------------------------------------- finding the arguments
SCAN_S, SCAN_A = (300, -450), (4962, 8770, -8770, 4962)      # rotation by 0.5 degree with +0.5 %: 1.005 (cos - 1, sin) 10^6


def test_scan_tool_measures_a_rotated_magnified_channel_and_its_result_undoes_it(tmp_path, capsys):
    """The second channel is the first one under the definition at (SCAN_S; SCAN_A): C2(c + q) = C1(c + (1 + A0) q + S0).  So the
    window of C2 at q is displaced by d(q) = A0 q + S0 against C1's, and the map that puts C2 right is the inverse one:
    t(p) = (1 + A0)^-1 (p - S0) - p.

    Bounds (STEP = 0.1 px, the registration's resolution at upsample 10).  Premise, asserted window by window: every window
    shift is measured within one STEP of d at the window centre.  Under it the least-squares offset is out by at most STEP and
    each of the two slopes per axis by at most STEP / L, L the spacing of the window centres; the corner lies 1.5 L from the
    centre along each axis, so the tool's displacement at a corner is within STEP + 2 * 1.5 * STEP = 4 STEP = 0.4 px per axis of
    t's.  The last comparison is an order, not a figure."""
    mod_spec = importlib.util.spec_from_file_location('channel_affine_scan', os.path.join(ROOT, 'tools', 'channel_affine_scan.py'))
    tool = importlib.util.module_from_spec(mod_spec)
    mod_spec.loader.exec_module(tool)
    h, w = 256, 320
    spec = synth.GridSpec(rows=2, cols=2, tile_h=h, tile_w=w, ov_y=36, ov_x=44, channels=(C405, C488), seed=43)
    root = str(tmp_path / 'acq')
    synth.write_acquisition(spec, root)
    n = 0
    for folder, _, names in os.walk(root):
        for name in names:
            if name.endswith('.tiff') and _channel_of(name) == C488:
                first = tiffio.read_image(os.path.join(folder, name.replace(C488.replace(' ', '_'), C405.replace(' ', '_'))))
                tiffio.write_tiff(os.path.join(folder, name), affine_ref.affine_image(first, SCAN_S, SCAN_A))
                n += 1
    assert n == 4
    capsys.readouterr()
    rows = tool.main(['-i', root, '--reference', C405, '--fovs', '3'])
    printed = capsys.readouterr().out
    assert len(rows) == 1
    row = rows[0]
    assert row['name'] == C488 and row['fields'] == 3
    s0 = np.array(SCAN_S) / 256
    m0 = np.array(SCAN_A, dtype=np.float64).reshape(2, 2) * 1e-6
    # the premise: every window of every field within one step of the generating map at its centre
    worst = 0.0
    for field in row['windows']:
        assert field.shape == (9, 4)
        d_true = field[:, :2] @ m0.T + s0
        worst = max(worst, float(np.abs(-field[:, 2:4] - d_true).max()))
    print(f'window shifts: worst deviation from the true map {worst:.3f} px')
    # the tool's map at the four corners against the inverse map's
    inv = np.linalg.inv(np.eye(2) + m0)
    corners = np.array([(py, px) for py in (-(h - 1) / 2, (h - 1) / 2) for px in (-(w - 1) / 2, (w - 1) / 2)])
    t_true = (corners - s0) @ inv.T - corners
    t_tool = np.array(row['shift_px']) + corners @ (np.array(row['affine_ppm'], dtype=np.float64).reshape(2, 2) * 1e-6).T
    corner_error = float(np.abs(t_tool - t_true).max())
    print(f'corner displacement: worst deviation {corner_error:.3f} px; printed: {tool.argument_line(row)}')
    assert worst <= tool.STEP + 1e-9, worst
    assert corner_error <= 4 * tool.STEP + 1e-9, corner_error
    assert tool.argument_line(row) in printed and 'beads, brightfield' in printed and row['agree'] == 3
    # away from a border of every tile the two channels' fused planes agree better with the printed arguments than with the
    # best --channel-shift alone, and better with that than without anything
    shift = tuple(channelshift.parse_pixels(f'{v:.3f}') for v in row['shift_px'])
    runs = {'both': dict(channel_shifts={C488: shift}, channel_affines={C488: row['affine_ppm']}),
            'shift': dict(channel_shifts={C488: shift}), 'plain': {}}
    border = 8
    mad = {}
    for key, kw in runs.items():
        st = _prepared(root, **kw)
        canvas, ids = st.stitch_planes(0, 'R0')
        planes = canvas.cpu().numpy().astype(np.int64)
        assert len(ids) == 2
        bad = np.zeros(planes.shape[1:], bool)
        inner = np.zeros((h, w), bool)
        inner[border:-border, border:-border] = True
        for info in st.get_region_data(0, 'R0').values():
            sy, sx, th, tw, y, x = (int(v) for v in st._tile_rect(info))
            bad[y:y + th, x:x + tw] |= ~inner[sy:sy + th, sx:sx + tw]
        assert (~bad).mean() > 0.6
        mad[key] = float(np.abs(planes[0][~bad] - planes[1][~bad]).mean())
    print(f'mean absolute difference of the two channels: {mad}')
    assert mad['both'] < mad['shift'] < mad['plain'], mad
