"""--dark-frame on the device: sq_dark_tiles against the numpy definition (tests/dark_ref.py), and whole runs with the option
against runs without it on a folder whose every tile file was subtracted beforehand.  Every comparison is equality."""
import ctypes
import hashlib
import json
import os
import random

import numpy as np
import pytest

import dark_cases
import dark_ref
import dpc_ref
import stream_cases as SC
from image_stitcher_amd import native, stitcher_cli, synth, tiffio
from image_stitcher_amd.stitcher import Stitcher
from image_stitcher_amd.stitcher_parameters import StitchingParameters

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
IPT = dark_cases.IPT


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the cached planes are read-only)


def _full(shape, value, dtype):
    return _dev(np.full(shape, value, dtype=np.dtype(dtype)))


# ---------------------------------------------------------------------------------------------------- the kernel
# (the shapes and the kernel's own sizes they are chosen from: tests/dark_cases.py)
@pytest.mark.parametrize('dtype', dark_cases.DTYPES)
@pytest.mark.parametrize('path', ['frame', 'constant'])
def test_kernel_equals_the_definition(path, dtype):
    import torch
    for h, w in dark_cases.shapes(dtype):
        planes = dark_cases.planes(dtype, h, w)
        frames = _dev(dark_cases.frames(dtype, h, w))
        sources = [('frame', i) for i in range(len(dark_cases.FRAME_NAMES))] if path == 'frame' else \
            [('constant', c) for c in dark_cases.constants(dtype)]
        for source in sources:
            for p in dark_cases.pedestals(dtype):
                tiles = _dev(planes)
                pair = (source[1], 0) if path == 'frame' else (-1, source[1])
                got = native.dark_tiles(tiles, pair, frames=frames if path == 'frame' else None, pedestal=p)
                assert got is tiles                                            # in place
                want = dark_cases.reference(dtype, h, w, source, p)
                host = got.cpu().numpy()
                for i, name in enumerate(dark_cases.PLANE_NAMES):
                    np.testing.assert_array_equal(host[i], want[i], err_msg=f'{(h, w)} {source} P={p} {name}')
        assert torch.equal(frames.cpu(), torch.from_numpy(np.array(dark_cases.frames(dtype, h, w))))      # the frames are read only


@pytest.mark.parametrize('dtype', dark_cases.DTYPES)
def test_grid_edges(dtype):
    """Two planes at the three edges of the strip / segment grid: narrower than one vector; one vector more than a workgroup is
    wide (two strips); and, at that width, one row more than a workgroup's rows (two segments)."""
    wide = dark_cases.STRIP[dtype] + dark_cases.VEC[dtype]
    for h, w in ((3, 5), (3, wide), (dark_cases.RPT + 1, wide)):
        planes, frames = dark_cases.planes(dtype, h, w, 2), dark_cases.frames(dtype, h, w)
        got = native.dark_tiles(_dev(planes), [(2, 0), (-1, 4)], frames=_dev(frames), pedestal=9).cpu().numpy()
        np.testing.assert_array_equal(got[0], dark_ref.dark_image(planes[0], frames[2], 9), err_msg=f'{(h, w)} frame')
        np.testing.assert_array_equal(got[1], dark_ref.dark_image(planes[1], 4, 9), err_msg=f'{(h, w)} constant')


@pytest.mark.parametrize('dtype', dark_cases.DTYPES)
def test_a_table_with_several_runs_and_identity_runs_in_the_middle(dtype):
    """Planes a stride of two planes apart and rows a pitch of 32 apart in a buffer of guard bytes (the stride is a whole number of
    vectors: a thread walks IPT images): the planes of the identity runs, every gap between two planes and the columns behind w
    come back bit for bit."""
    h, w, p = dark_cases.RPT + 3, 21, 9
    same = (-1, p)
    table = [(0, 0), (0, 0), same, same, (2, 0), same, (-1, 4), (-1, 4), same, (3, 0)]
    n = len(table)
    planes, frames = dark_cases.planes(dtype, h, w, n), dark_cases.frames(dtype, h, w)
    guard = 0xA5 if dtype == 'uint8' else 0xA5A5
    buf = _full((2 * n + 1, h, 32), guard, dtype)
    tiles = buf[1::2, :, :w]
    tiles.copy_(_dev(planes))
    native.dark_tiles(tiles, table, frames=_dev(frames), pedestal=p)
    host = buf.cpu().numpy()
    assert (host[0::2] == guard).all() and (host[:, :, w:] == guard).all()
    for i, (k, c) in enumerate(table):
        want = planes[i] if (k, c) == same else dark_ref.dark_image(planes[i], frames[k] if k >= 0 else c, p)
        np.testing.assert_array_equal(host[1 + 2 * i, :, :w], want, err_msg=f'plane {i} {(k, c)}')
    assert any((host[1 + 2 * i, :, :w] != planes[i]).any() for i in range(n))
    # a stack with two leading dimensions: one pair per index of the first, for all planes under it; numpy integers are taken
    stack = _dev(planes[:6].reshape(2, 3, h, w))
    got = native.dark_tiles(stack, [same, (np.int64(2), np.int32(0))], frames=_dev(frames), pedestal=p).cpu().numpy()
    np.testing.assert_array_equal(got[0], planes[:3])
    np.testing.assert_array_equal(got[1], dark_ref.dark_image(planes[3:6], frames[2], p))
    for bad in ([(0, 0)], [(0, 0)] * 3, [(0, 0), (0,)], [(0, 0), (0.0, 0)], 5, None, [(0, 0), (True, 0)], [(0, 0), (4, 0)],
                [(0, 0), (0, 1)], [(0, 0), (-2, 0)], [(0, 0), (-1, dark_cases.top(dtype) + 1)]):
        with pytest.raises(ValueError):
            native.dark_tiles(stack, bad, frames=_dev(frames), pedestal=p)
    np.testing.assert_array_equal(stack.cpu().numpy(), got)      # nothing was launched


@pytest.mark.parametrize('dtype', dark_cases.DTYPES)
def test_run_lengths_around_the_images_a_thread_walks(dtype):
    h, w, p = 11, 37, 3
    frames = dark_cases.frames(dtype, h, w)
    lengths = [IPT - 1, IPT, IPT + 1, 1, 2 * IPT + 1]
    sources = [(2, 0), (3, 0), (-1, 77), (2, 0), (-1, 1)]
    table = [pair for pair, m in zip(sources, lengths) for _ in range(m)]
    planes = dark_cases.planes(dtype, h, w, len(table))
    # rows a pitch of 48 apart: the plane stride is a whole number of vectors, so a thread walks IPT images of a run
    buf = _full((len(table), h, 48), 1, dtype)
    buf[:, :, :w].copy_(_dev(planes))
    got = native.dark_tiles(buf[:, :, :w], table, frames=_dev(frames), pedestal=p).cpu().numpy()
    assert (buf.cpu().numpy()[:, :, w:] == 1).all()
    # ... and a contiguous stack of the same planes, whose stride is not: image by image
    np.testing.assert_array_equal(native.dark_tiles(_dev(planes), table, frames=_dev(frames), pedestal=p).cpu().numpy(), got)
    for i, (k, c) in enumerate(table):
        np.testing.assert_array_equal(got[i], dark_ref.dark_image(planes[i], frames[k] if k >= 0 else c, p), err_msg=f'plane {i}')


def test_more_images_than_one_grid_takes():
    """A grid takes 65535 groups of IPT images: a few images more, of 1 x 1 pixels, through the C entry.  Planes 16 elements apart
    (a whole vector: groups of IPT images, two grids) as one run on either path and as a table of eleven runs; planes one
    element apart (always image by image) as one run."""
    import torch
    n = (dark_cases.GRID_Y * IPT // 11 + 1) * 11      # the first multiple of eleven above what one grid takes
    src = torch.arange(n, dtype=torch.int32, device=DEV).remainder(251).to(torch.uint8)
    buf = torch.full((n + 1, 16), 200, dtype=torch.uint8, device=DEV)
    frame = torch.tensor([40], dtype=torch.uint8, device=DEV)
    L = native.lib()

    def call(table, per, frames=None, n_frames=0):
        buf[:n, 0].copy_(src)
        status = L.sq_dark_tiles(buf.data_ptr(), n, 1, 1, 16, 1, native.SQ_U8, frames, n_frames, 1, 1, table, per, 7, None)
        torch.cuda.synchronize()
        assert bool((buf[:, 1:] == 200).all()) and bool((buf[n] == 200).all())
        return status

    wide = src.to(torch.int32)
    assert call((ctypes.c_int32 * 2)(-1, 40), n) == 0
    assert torch.equal(buf[:n, 0], (wide - 33).clamp(0, 255).to(torch.uint8))
    assert call((ctypes.c_int32 * 2)(0, 0), n, frame.data_ptr(), 1) == 0
    assert torch.equal(buf[:n, 0], (wide - 33).clamp(0, 255).to(torch.uint8))
    assert n % 11 == 0      # eleven pairs of n / 11 images: the identity, two equal pairs (one run), a frame, ...
    table = [(-1, 7), (-1, 40), (-1, 40), (0, 0), (-1, 0), (-1, 7), (-1, 255), (0, 0), (0, 0), (-1, 7), (-1, 3)]
    assert call((ctypes.c_int32 * 22)(*[v for pair in table for v in pair]), n // 11, frame.data_ptr(), 1) == 0
    shift = torch.tensor([7 - (40 if k == 0 else c) for k, c in table], dtype=torch.int32, device=DEV).repeat_interleave(n // 11)
    assert torch.equal(buf[:n, 0], (wide + shift).clamp(0, 255).to(torch.uint8))
    dense = torch.full((2 * n,), 200, dtype=torch.uint8, device=DEV)
    dense[:n].copy_(src)
    assert L.sq_dark_tiles(dense.data_ptr(), n, 1, 1, 1, 1, native.SQ_U8, None, 0, 0, 0, (ctypes.c_int32 * 2)(-1, 40), n, 7, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(dense[:n], (wide - 33).clamp(0, 255).to(torch.uint8)) and bool((dense[n:] == 200).all())


@pytest.mark.parametrize('dtype', dark_cases.DTYPES)
@pytest.mark.parametrize('path', ['frame', 'constant'])
def test_views_pitches_offsets_guard_and_repeatability(path, dtype):
    import torch
    h, w, p = 9, 37, 5
    planes, frames = dark_cases.planes(dtype, h, w), dark_cases.frames(dtype, h, w)
    n_planes = len(planes)
    tdtype = native.torch_dtype_of(np.dtype(dtype))
    fill = dark_cases.top(dtype) // 3
    source, pair = (('frame', 2), (0, 0)) if path == 'frame' else (('constant', 77), (-1, 77))
    want = dark_cases.reference(dtype, h, w, source, p)
    frame_dev = _dev(frames[2:3]) if path == 'frame' else None
    # every other plane of a stack: the planes between stay as they are
    big = _full((2 * n_planes, h, w), fill, dtype)
    big[1::2].copy_(_dev(planes))
    native.dark_tiles(big[1::2], pair, frames=frame_dev, pedestal=p)
    np.testing.assert_array_equal(big.cpu().numpy()[1::2], want)
    assert (big.cpu().numpy()[0::2] == fill).all()
    # a pitch above w that is no whole number of vectors (the plane stride is none either: the images go one by one), and a
    # frame with a pitch of its own: the columns between w and the pitch stay as they are
    wide = _full((n_planes, h, w + 3), fill, dtype)
    wide[:, :, :w].copy_(_dev(planes))
    wide_frame = None
    if path == 'frame':
        wide_frame = _full((1, h, w + 5), 1, dtype)
        wide_frame[:, :, :w].copy_(frame_dev)
        wide_frame = wide_frame[:, :, :w]
    native.dark_tiles(wide[:, :, :w], pair, frames=wide_frame, pedestal=p)
    np.testing.assert_array_equal(wide.cpu().numpy()[:, :, :w], want)
    assert (wide.cpu().numpy()[:, :, w:] == fill).all()
    # tiles and a frame that each start at an element offset, through every phase of 16 bytes -- 8 uint16 / 16 uint8 -- plus
    # one beyond it: the tiles' phase decides between the 16-byte accesses and the element ones, and the frame's phase between
    # its 16-byte load and its element loads.  Both are views of wider buffers whose row pitch is a multiple of 16 bytes, so
    # the images of a group share their rows' phase.
    vec = 16 // planes.itemsize
    pitch = (w + vec - 1) // vec * vec + vec
    n_el = n_planes * h * pitch
    padded = np.full((n_planes, h, pitch), fill, planes.dtype)
    padded[:, :, :w] = planes
    padded_dev = _dev(padded).reshape(-1)
    frame_padded = np.full((1, h, pitch), 1, planes.dtype)
    frame_padded[:, :, :w] = frames[2]
    for f_off in ([0, 1, vec - 1, vec + 3] if path == 'frame' else [0]):
        fbuf = _full((h * pitch + 2 * vec + 8,), 1, dtype)
        fbuf[f_off:h * pitch + f_off] = _dev(frame_padded).reshape(-1)
        frame_off = fbuf[f_off:h * pitch + f_off].view(1, h, pitch)[:, :, :w] if path == 'frame' else None
        for t_off in list(range(vec)) + [vec + 1]:
            buf = _full((n_el + 2 * vec + 8,), fill, dtype)
            buf[t_off:n_el + t_off] = padded_dev
            view = buf[t_off:n_el + t_off].view(n_planes, h, pitch)
            assert (view.data_ptr() // planes.itemsize) % vec == t_off % vec
            got = native.dark_tiles(view[:, :, :w], pair, frames=frame_off, pedestal=p)
            np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f'frame offset {f_off}, tile offset {t_off}')
            host = buf.cpu().numpy()
            assert (host[:t_off] == fill).all() and (host[n_el + t_off:] == fill).all()
            assert (host[t_off:n_el + t_off].reshape(n_planes, h, pitch)[:, :, w:] == fill).all()      # between w and the pitch
    # a guard band of 0xA5 in front of and behind the tiles stays intact
    nbytes = want.size * planes.itemsize
    raw = torch.full((4096 + nbytes + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    tiles = raw[4096:4096 + nbytes].view(tdtype).view(n_planes, h, w)
    tiles.copy_(_dev(planes))
    native.dark_tiles(tiles, pair, frames=frame_dev, pedestal=p)
    np.testing.assert_array_equal(tiles.cpu().numpy(), want)
    assert bool((raw[:4096] == 0xA5).all()) and bool((raw[4096 + nbytes:] == 0xA5).all())
    # the same call on a fresh copy: the same bytes
    runs = [native.dark_tiles(_dev(planes), pair, frames=frame_dev, pedestal=p).cpu().numpy().tobytes() for _ in range(2)]
    assert runs[0] == runs[1] == want.tobytes()


def test_refusals():
    import torch
    t_np = (np.arange(3 * 8 * 12, dtype=np.uint16).reshape(3, 8, 12) * 200).astype(np.uint16)
    f_np = np.full((2, 8, 12), 1000, np.uint16)
    t, f = _dev(t_np), _dev(f_np)
    for bad in ((2, 0), (-2, 0), (0, 1), (-1, 65536), (-1, -1), (1.0, 0), (True, 0), (None, 0), ('0', 0)):
        with pytest.raises(ValueError):
            native.dark_tiles(t, bad, frames=f)
    for bad in (-1, 65536, 1.0, True, None):
        with pytest.raises(ValueError):
            native.dark_tiles(t, (0, 0), frames=f, pedestal=bad)
    with pytest.raises(ValueError):
        native.dark_tiles(t, (0, 0))                                                   # a frame is named, none is given
    with pytest.raises(ValueError):
        native.dark_tiles(t.to(torch.float32), (-1, 1))                                # a wrong dtype
    with pytest.raises(ValueError):
        native.dark_tiles(t.permute(0, 2, 1), (-1, 1))                                 # rows that are not contiguous
    with pytest.raises(ValueError):
        native.dark_tiles(t, (0, 0), frames=f[:, :, :11])                              # another shape
    with pytest.raises(ValueError):
        native.dark_tiles(t, (0, 0), frames=_full((2, 8, 12), 7, 'uint8'))             # another dtype
    with pytest.raises(ValueError):
        native.dark_tiles(t, (0, 0), frames=torch.zeros((2, 8, 12), dtype=torch.uint16))            # another device
    with pytest.raises(ValueError, match='shares memory'):
        native.dark_tiles(t[:2], (0, 0), frames=t[1:])
    with pytest.raises(ValueError, match='pedestal'):
        native.dark_tiles(_full((2, 4, 4), 7, 'uint8'), (-1, 1), pedestal=256)
    np.testing.assert_array_equal(t.cpu().numpy(), t_np)      # nothing was launched
    # the library itself refuses what the wrapper would let through, with its own message
    L = native.lib()
    pairs = (ctypes.c_int32 * 6)(1, 0, 1, 0, -1, 500)

    def call(tiles=t.data_ptr(), n=3, h=8, w=12, ps=96, pitch=12, dtype=native.SQ_U16, frames=f.data_ptr(), nf=2, fs=96, fp=12,
             table=pairs, per=1, pedestal=10):
        return L.sq_dark_tiles(tiles, n, h, w, ps, pitch, dtype, frames, nf, fs, fp, table, per, pedestal, None)

    assert call(n=0) == 0 and call(n=0, tiles=None, frames=None, table=None) == 0      # no image: SQ_OK, nothing launched
    for bad in (dict(dtype=native.SQ_F32), dict(dtype=0), dict(pedestal=-1), dict(pedestal=65536),
                dict(table=(ctypes.c_int32 * 6)(1, 0, 1, 0, -1, 65536)), dict(table=(ctypes.c_int32 * 6)(1, 0, 1, 0, -1, -1)),
                dict(table=(ctypes.c_int32 * 6)(2, 0, 1, 0, -1, 5)), dict(table=(ctypes.c_int32 * 6)(-2, 0, 1, 0, -1, 5)),
                dict(table=(ctypes.c_int32 * 6)(1, 1, 1, 0, -1, 5)), dict(nf=1), dict(nf=-1), dict(table=None),
                dict(pitch=11), dict(fp=11), dict(ps=95), dict(fs=95), dict(tiles=None), dict(frames=None),
                dict(tiles=t.data_ptr() + 1), dict(frames=f.data_ptr() + 1), dict(n=-1), dict(per=2), dict(per=0), dict(per=-1),
                dict(h=0), dict(w=0), dict(h=-1), dict(frames=t.data_ptr()), dict(frames=t.data_ptr() + 2 * 96 * 2, nf=1),
                dict(tiles=f.data_ptr(), n=1, table=(ctypes.c_int32 * 2)(1, 0)),
                dict(dtype=native.SQ_U8, pedestal=256), dict(dtype=native.SQ_U8, table=(ctypes.c_int32 * 6)(1, 0, 1, 0, -1, 256))):
        assert call(**bad) == -1, bad      # SQ_ERR_INVALID
    assert call(frames=t.data_ptr()) == -1 and 'overlap' in L.sq_last_error().decode()
    assert call(pedestal=65536) == -1 and '65535' in L.sq_last_error().decode()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(t.cpu().numpy(), t_np)      # nothing was written by a refused call
    np.testing.assert_array_equal(f.cpu().numpy(), f_np)
    # NULL frames are fine when no pair names one; and the call as it stands is accepted
    const = (ctypes.c_int32 * 2)(-1, 500)
    assert call(frames=None, nf=0, table=const, per=3) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(t.cpu().numpy(), dark_ref.dark_image(t_np, 500, 10))
    t.copy_(_dev(t_np))
    assert call() == 0
    torch.cuda.synchronize()
    want = np.stack([dark_ref.dark_image(t_np[0], f_np[1], 10), dark_ref.dark_image(t_np[1], f_np[1], 10),
                     dark_ref.dark_image(t_np[2], 500, 10)])
    np.testing.assert_array_equal(t.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------- off the default stream
def _stream_case(dtype, table, pedestal):
    top = dark_cases.top(dtype)
    shape = (4, 50, 70)

    def inputs(seed):
        rng = np.random.default_rng(seed)
        return {'tiles': rng.integers(0, top + 1, shape).astype(dtype), 'frames': rng.integers(0, top // 2, (2, 50, 70)).astype(dtype)}

    def call(ctx, inp, out, stream):      # in place
        return {'tiles': native.dark_tiles(inp['tiles'], table, frames=inp['frames'], pedestal=pedestal, stream=stream)}

    def reference(a, strict):
        return {'tiles': np.stack([dark_ref.dark_image(pl, a['frames'][k] if k >= 0 else c, pedestal)
                                   for pl, (k, c) in zip(a['tiles'], table)])}
    return SC.Case(f'dark-tiles-{np.dtype(dtype).name}', inputs(510), inputs(511), {}, call, reference)


STREAM_CASES = {c.name: c for c in (_stream_case(np.uint16, [(0, 0), (0, 0), (-1, 300), (1, 0)], 100),
                                    _stream_case(np.uint8, [(1, 0)] * 4, 3))}


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
NOTE = '_stitched_dark_frame.json'
LEFT, RIGHT, FLUO = 'BF LED matrix left half', 'BF LED matrix right half', 'Fluorescence 488 nm Ex'
C405, C488, C561 = synth.DEFAULT_CHANNELS[:3]
# a synthetic 2 x 2 grid of 64 x 64 tiles with two z levels and three channels; the first channel is the registration channel
SPEC = dict(rows=2, cols=2, tile_h=64, tile_w=64, ov_y=24, ov_x=24, nz=2, channels=(C405, C488, C561), seed=37)
PEDESTAL = 40
CONSTANT = 9000      # the synthetic uint16 tiles lie in 800..41200 around 21000: a dark level of 8000..16000 clips a few per cent


def _frame(seed, dtype='uint16', shape=(64, 64)):
    """A camera-like frame scaled to the synthetic tiles: a level with noise, column offsets and a few warm pixels."""
    rng = np.random.default_rng(seed)
    lo, hi, warm = (8000, 16000, 60000) if np.dtype(dtype) == np.uint16 else (30, 60, 250)
    frame = rng.integers(lo, hi, shape) + rng.integers(0, (hi - lo) // 8, (1, shape[1]))
    frame.reshape(-1)[rng.integers(0, frame.size, 12)] = warm
    return frame.astype(dtype)


def _channel_of(name):
    return os.path.splitext(name.split('_', 3)[3])[0].replace('_', ' ').replace('full ', 'full_')


def premake_folder(root, frames, pedestal):
    """F -> F' in place: every tile file replaced by dark_ref.dark_image of it under its channel's frame (``frames``: {file
    channel: frame, int, or a list of one per colour plane}, '*' for the channels without an entry).  Asserts on the host that
    the comparison is neither vacuous nor all zero: more than half of the pixels change, between 0.1 % and 50 % clip at 0."""
    total = changed = clipped = 0
    for folder, _, names in os.walk(root):
        for name in names:
            if name.lower().endswith(('.tif', '.tiff')):
                path = os.path.join(folder, name)
                channel = _channel_of(name)
                frame = frames.get(channel, frames.get('*'))
                if frame is None:
                    continue
                img = tiffio.read_image(path)
                new = dark_ref.dark_file_image(img, frame, pedestal)
                assert new.shape == img.shape and new.dtype == img.dtype
                planes = [c for c, f in enumerate(frame) if f is not None] if isinstance(frame, list) else None
                a, b = (img, new) if planes is None else (img[:, :, planes], new[:, :, planes])
                total, changed, clipped = total + a.size, changed + int((a != b).sum()), clipped + int(((b == 0) & (a != 0)).sum())
                tiffio.write_tiff(path, new)
    assert total and changed > total // 2, (changed, total)
    assert 0.001 * total < clipped < 0.5 * total, (clipped, total)
    return changed


def _two_roots(tmp_path, frames, pedestal=PEDESTAL, spec=None):
    spec = spec or synth.GridSpec(**SPEC)
    a, b = str(tmp_path / 'with_flag' / 'acq'), str(tmp_path / 'premade' / 'acq')
    for r in (a, b):
        synth.write_acquisition(spec, r)
    premake_folder(b, frames, pedestal)
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


def _files(tmp_path):
    """Two frames as files (.npy and .tiff) and the sources of the standard run: a frame, another frame, a constant."""
    f1, f2 = _frame(1), _frame(2)
    p1, p2 = str(tmp_path / 'dark_405.npy'), str(tmp_path / 'dark_488.tiff')
    np.save(p1, f1)
    tiffio.write_tiff(p2, f2)
    frames = {C405: f1, C488: f2, C561: CONSTANT}
    flags = ['--dark-frame', C405, p1, '--dark-frame', C488, p2, '--dark-frame', C561, str(CONSTANT), '--dark-pedestal', str(PEDESTAL)]
    return frames, flags, (p1, p2)


@pytest.mark.parametrize('fmt', ['.ome.zarr', '.ome.tiff'])
def test_flag_on_f_equals_no_flag_on_f_prime(tmp_path, capsys, fmt):
    frames, flags, (p1, p2) = _files(tmp_path)
    a, b = _two_roots(tmp_path, frames)
    capsys.readouterr()
    got = _cli(a, '-f', fmt, *flags)
    assert capsys.readouterr().out.count('[dark-frame]') == 1
    want = _cli(b, '-f', fmt)
    assert '[dark-frame]' not in capsys.readouterr().out
    _same_trees(got, want)
    assert _notes(got) == [os.path.join('0_stitched', 'R0' + NOTE)]
    with open(os.path.join(got, '0_stitched', 'R0' + NOTE)) as fh:
        note = json.load(fh)
    f1 = frames[C405]
    assert note['channels'][C561] == {'constant': CONSTANT}
    assert note['channels'][C405] == {'path': p1, 'sha256': hashlib.sha256(f1.tobytes()).hexdigest(), 'min': int(f1.min()),
                                      'max': int(f1.max()), 'mean': int(f1.astype(np.int64).sum()) // f1.size}
    assert note['channels'][C488]['path'] == p2 and sorted(note['channels']) == sorted([C405, C488, C561])
    assert note['pedestal'] == PEDESTAL and note['tile_shape'] == [64, 64] and note['order'].startswith('first')
    assert note['device_frames'] == 2 and note['device_frame_bytes'] == 2 * 64 * 64 * 2
    # ... and the run on F without the flag is another tree
    third = str(tmp_path / 'plain' / 'acq')
    synth.write_acquisition(synth.GridSpec(**SPEC), third)
    plain = _tree(_cli(third, '-f', fmt))
    assert sorted(plain) == sorted(_tree(got)) and plain != _tree(got)


@pytest.mark.parametrize('mode', ['overwrite', 'feather'])
def test_registration_and_device_basic_flatfield(tmp_path, mode):
    """-r -ff: the registration channel takes its frame in the centre-pair readers; the flatfield estimate's samples and
    get_tile subtract on the host with the same arithmetic."""
    frames, dark_flags, _ = _files(tmp_path)
    a, b = _two_roots(tmp_path, frames)
    flags = ('-r', '-ff', '--flatfield-estimator', 'basic', '--fusion-mode', mode)
    tree = _same_trees(_cli(a, *flags, *dark_flags), _cli(b, *flags))
    assert 'shift_table.json' in tree and 'flatfield_info.json' in tree
    st_a, st_b = _prepared(a, dark_frames=frames, dark_pedestal=PEDESTAL), _prepared(b)
    for channel in (C405, C488, C561):
        info = next(v for v in st_a.get_region_data(0, 'R0').values() if v['channel'] == channel and v['z_level'] == 1)
        np.testing.assert_array_equal(st_a.get_tile(0, 'R0', info['x'], info['y'], channel, 1),
                                      st_b.get_tile(0, 'R0', info['x'], info['y'], channel, 1))


def test_all_pairs_registration_takes_the_registration_channels_frame(tmp_path, monkeypatch):
    frames, dark_flags, _ = _files(tmp_path)
    a, b = _two_roots(tmp_path, frames)
    calls = _record(monkeypatch)
    flags = ('-r', '--all-pairs-registration', '--registration-channel', C488)
    got = _cli(a, *flags, *dark_flags)
    assert calls[0] == 'dark_tiles'      # registration's stack, before the first chunk
    tree = _same_trees(got, _cli(b, *flags))
    assert 'shift_table.json' in tree


def test_with_every_other_head_option(tmp_path):
    """Dark frame, correct, shift / affine, bin, all in sensor pixels: the other options are on in both runs."""
    frames, dark_flags, _ = _files(tmp_path)
    a, b = _two_roots(tmp_path, frames)
    flags = ('--distortion-correction', '20000', '--channel-shift', C488, '0.3', '-0.78125', '--channel-affine', C561, '300',
             '-4000', '4000', '300', '--tile-binning', '2')
    tree = _same_trees(_cli(a, *flags, *dark_flags), _cli(b, *flags))      # (the other options' notes are in both trees)
    for note in ('_stitched_distortion.json', '_stitched_binning.json', '_stitched_channel_shift.json',
                 '_stitched_channel_affine.json'):
        assert any(k.endswith(note) for k in tree), note


def test_with_dpc_a_different_frame_on_each_half(tmp_path):
    spec = synth.GridSpec(**dict(SPEC, channels=(LEFT, RIGHT, FLUO)))
    frames = {LEFT: _frame(3), RIGHT: _frame(4), FLUO: CONSTANT}
    a, b = _two_roots(tmp_path, frames, spec=spec)
    got, want = _api(a, dpc=True, dark_frames=frames, dark_pedestal=PEDESTAL), _api(b, dpc=True)
    _same_trees(got.output_folder, want.output_folder)
    # DPC is dpc_ref of the two F' files: wherever one tile alone covers the canvas
    st = _prepared(a, dpc=True, dark_frames=frames, dark_pedestal=PEDESTAL)
    canvas, ids = st.stitch_planes(0, 'R0', only_planes=[st._dpc_index * st.num_z])
    plane = canvas[0].cpu().numpy()
    cover = np.zeros(plane.shape, np.int32)
    expect = np.zeros(plane.shape, plane.dtype)
    n = 0
    for info in st.get_region_data(0, 'R0').values():
        if info['channel'] == native.DPC_CHANNEL and info['z_level'] == 0:
            name = os.path.basename(info['filepath'])
            left = tiffio.read_image(os.path.join(b, '0', name))
            right = tiffio.read_image(os.path.join(b, '0', os.path.basename(info['filepath_right'])))
            tile = dpc_ref.dpc_image(left, right, 1)
            sy, sx, h, w, y, x = (int(v) for v in st._tile_rect(info))
            cover[y:y + h, x:x + w] += 1
            expect[y:y + h, x:x + w] = tile[sy:sy + h, sx:sx + w]
            n += 1
    assert n == 4 and (cover == 1).mean() > 0.3
    np.testing.assert_array_equal(plane[cover == 1], expect[cover == 1])


def test_with_tile_qc_seam_qc_despeckle_tophat_and_projection(tmp_path):
    frames, _, _ = _files(tmp_path)
    a, b = _two_roots(tmp_path, frames)
    kw = dict(tile_qc=True, seam_qc=True, seam_qc_min_pixels=16, despeckle='hot', despeckle_threshold=2000,
              background_subtract='tophat', background_radius=5, z_projection='max')
    got, want = _api(a, dark_frames=frames, dark_pedestal=PEDESTAL, **kw), _api(b, **kw)
    skip = (NOTE,)
    tree = _same_trees(got.output_folder, want.output_folder, skip)
    for part in ('_tile_qc.csv', '_tile_qc.json', '_seam_qc.csv', '_seam_qc.json', '_mip'):
        assert any(part in k for k in tree), part
    assert got.tile_qc_table and got.tile_qc_table == want.tile_qc_table      # the report describes F''s files
    assert got.seam_qc_table and got.seam_qc_table == want.seam_qc_table
    assert got.despeckle_replaced == want.despeckle_replaced


def test_uint8_rgb_files_with_a_frame_on_one_colour_plane(tmp_path):
    rgb = 'BF LED matrix full_RGB'
    spec = synth.GridSpec(rows=2, cols=2, tile_h=64, tile_w=64, ov_y=24, ov_x=24, channels=(rgb, C488), rgb_channels=(rgb,),
                          dtype='uint8', seed=41)
    names_root = str(tmp_path / 'names' / 'acq')
    synth.write_acquisition(spec, names_root)
    names = _prepared(names_root).monochrome_channels
    base = [n for n in names if n.endswith('_G')][0][:-2]
    frame = _frame(5, 'uint8')
    a, b = _two_roots(tmp_path, {rgb: [None, frame, None]}, pedestal=2, spec=spec)
    got, want = _api(a, dark_frames={f'{base}_G': frame}, dark_pedestal=2), _api(b)
    _same_trees(got.output_folder, want.output_folder)
    assert got._dark_params == {got.monochrome_channels.index(f'{base}_G'): (0, 0)}


def test_wildcard_plus_one_override(tmp_path):
    f1, f2 = _frame(6), _frame(7)
    a, b = _two_roots(tmp_path, {'*': f1, C488: f2})
    got, want = _api(a, dark_frames={'*': f1, C488: f2}, dark_pedestal=PEDESTAL), _api(b)
    _same_trees(got.output_folder, want.output_folder)
    idx = got.monochrome_channels.index
    assert got._dark_params == {idx(C405): (0, 0), idx(C488): (1, 0), idx(C561): (0, 0)}


def test_small_batches_ring_turns_and_row_bands_subtract_every_plane_once(tmp_path):
    """One plane per chunk: six chunks over two ring slots, three turns each, and the same region again in two row bands and in
    a second call on the same cached buffers -- a plane subtracted twice, or not at all, is another canvas."""
    frames, _, _ = _files(tmp_path)
    a, b = _two_roots(tmp_path, frames)
    st = _prepared(a, batch_bytes_limit=1, dark_frames=frames, dark_pedestal=PEDESTAL)
    plain = _prepared(b, batch_bytes_limit=1)
    want, ids = plain.stitch_planes(0, 'R0')
    want = want.cpu().numpy()
    assert len(ids) == 6 and want.any()
    for _ in range(2):      # the second call finds the ring's slots and the frames in the cache
        canvas, _ = st.stitch_planes(0, 'R0')
        np.testing.assert_array_equal(canvas.cpu().numpy(), want)
    assert [k for k in st._buffer_cache if k[0] == 'ingest'][0][1] == 1      # chunks of one plane
    height = want.shape[1]
    mid = height // 2 + 3
    top, _ = st.stitch_planes(0, 'R0', row_band=(0, mid))
    bottom, _ = st.stitch_planes(0, 'R0', row_band=(mid, height))
    np.testing.assert_array_equal(np.concatenate([top.cpu().numpy(), bottom.cpu().numpy()], axis=1), want)
    # a batch of some planes (chunks of four and two), and all six in one chunk
    per_plane = 4 * 64 * 64 * 2
    for limit in (4 * per_plane, None):
        other = _prepared(a, batch_bytes_limit=limit, dark_frames=frames, dark_pedestal=PEDESTAL)
        canvas, _ = other.stitch_planes(0, 'R0')
        np.testing.assert_array_equal(canvas.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------- the launches
RECORDED = ('dark_tiles', 'warp_tiles', 'shift_tiles', 'affine_tiles', 'bin_tiles', 'dpc_tiles', 'fuse_planes')


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
    st = _prepared(root, batch_bytes_limit=1, distortion_correction=20000, tile_binning=2, dpc=True,
                   channel_shifts={FLUO: (77, -200)}, dark_frames={'*': _frame(8), RIGHT: _frame(9)}, dark_pedestal=PEDESTAL)
    calls = _record(monkeypatch)
    canvas, ids = st.stitch_planes(0, 'R0')
    fluo = st.monochrome_channels.index(FLUO)
    assert ids == list(range(8)) and st._dpc_index == 2 and fluo == 3
    # the head of every chunk: dark first, corrected, shifted only where the chunk holds a shifted plane, binned; the right
    # halves of the derived planes pass the same head under the right half's frame
    want = [['dark_tiles', 'warp_tiles'] + (['shift_tiles'] if p // st.num_z == fluo else []) + ['bin_tiles'] +
            (['dark_tiles', 'warp_tiles', 'bin_tiles', 'dpc_tiles'] if p // st.num_z == st._dpc_index else []) + ['fuse_planes']
            for p in ids]
    assert _chunks(calls) == want
    assert [k for k in st._buffer_cache if k[0] == 'dark-frames'] == [('dark-frames', 2, 64, 64, '<u2')]
    assert not [k for k in st._buffer_cache if k[0] not in ('ingest', 'dpc', 'distortion', 'distortion-dpc', 'shift', 'binning',
                                                             'binning-dpc', 'dark-frames')]
    assert canvas.cpu().numpy().any()


def test_launch_order_alone_off_and_identity(tmp_path, monkeypatch):
    root = str(tmp_path / 'acq')
    synth.write_acquisition(synth.GridSpec(**SPEC), root)
    # C405 has a frame, C488 the identity (a constant equal to the pedestal), C561 no entry
    st = _prepared(root, batch_bytes_limit=1, dark_frames={C405: _frame(10), C488: PEDESTAL}, dark_pedestal=PEDESTAL)
    calls = _record(monkeypatch)
    _, ids = st.stitch_planes(0, 'R0')
    first = st.monochrome_channels.index(C405)
    # a chunk whose channels are all the identity launches nothing
    assert _chunks(calls) == [(['dark_tiles'] if p // st.num_z == first else []) + ['fuse_planes'] for p in ids]
    assert _notes(st.output_folder)
    # every channel the identity: no launch at all, no frame on the device
    same = _prepared(root, dark_frames={'*': PEDESTAL}, dark_pedestal=PEDESTAL)
    del calls[:]
    canvas, _ = same.stitch_planes(0, 'R0')
    assert calls == ['fuse_planes'] and [k[0] for k in same._buffer_cache] == ['ingest']
    # off -- no option, None, an empty mapping: never called, no buffer, no note, the canvas of the identity run
    off_root = str(tmp_path / 'off' / 'acq')
    synth.write_acquisition(synth.GridSpec(**SPEC), off_root)
    for kw in ({}, dict(dark_frames=None), dict(dark_frames={})):
        off = _prepared(off_root, batch_bytes_limit=1, **kw)
        del calls[:]
        plain, _ = off.stitch_planes(0, 'R0')
        assert calls == ['fuse_planes'] * 6
        assert [k[0] for k in off._buffer_cache] == ['ingest']
        assert not _notes(off.output_folder)
        assert bool((plain == canvas).all())


def test_off_the_output_tree_is_todays(tmp_path, capsys):
    """Without the flag: the tree of a run whose Stitcher was never told of the option (the defaults), and no line printed."""
    a, b = str(tmp_path / 'a' / 'acq'), str(tmp_path / 'b' / 'acq')
    for r in (a, b):
        synth.write_acquisition(synth.GridSpec(**SPEC), r)
    capsys.readouterr()
    got = _cli(a)
    assert '[dark-frame]' not in capsys.readouterr().out
    want = _api(b).output_folder
    x, y = _tree(got, ()), _tree(want, ())
    assert x and sorted(x) == sorted(y) and [k for k in x if x[k] != y[k]] == []
    assert not _notes(got)
