"""--distortion-correction on the device: sq_warp_tiles against the numpy definition (tests/warp_ref.py), and whole runs with the
option against runs without it on a folder of files corrected beforehand.  Every comparison is equality."""
import hashlib
import json
import os
import random
import re

import numpy as np
import pytest

import bin_ref
import stream_cases as SC
import warp_cases
import warp_ref
from helpers import load_case, spec_of
from image_stitcher_amd import native, stitcher_cli, synth, tiffio
from image_stitcher_amd.stitcher import Stitcher
from image_stitcher_amd.stitcher_parameters import StitchingParameters

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
D = 20000      # the whole runs' coefficient: it changes 98 % of the pixels of a 128 x 160 synthetic tile


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the cached planes are read-only)


def _full(shape, value, dtype):
    return _dev(np.full(shape, value, dtype=np.dtype(dtype)))


# ---------------------------------------------------------------------------------------------------- the kernel
# (the shapes and the kernel's own sizes they are chosen from: tests/warp_cases.py)
@pytest.mark.parametrize('dtype', warp_cases.DTYPES)
@pytest.mark.parametrize('ppm', warp_cases.PPMS)
def test_kernel_equals_the_definition(ppm, dtype):
    clamped = 0
    for h, w in warp_cases.SHAPES:
        planes = warp_cases.planes(dtype, h, w)
        src = _dev(planes)
        want = warp_cases.reference(dtype, h, w, ppm)
        got = native.warp_tiles(src, ppm)
        assert got.dtype == src.dtype and tuple(got.shape) == planes.shape
        host = got.cpu().numpy()
        for i, name in enumerate(warp_cases.PLANE_NAMES):
            np.testing.assert_array_equal(host[i], want[i], err_msg=f'{(h, w)} D={ppm} {name}')
        np.testing.assert_array_equal(src.cpu().numpy(), planes)      # the source is left as it was
        if ppm in (0, 1, -1) and max(h, w) <= 300:
            np.testing.assert_array_equal(host, planes)                # the identity
        # the clamp, from the definition's own map: on every border at +50000, nowhere at -50000
        if abs(ppm) == 50000 and min(h, w) >= 3:
            active = warp_ref.clamp_active(h, w, ppm)
            assert all(active.values()) if ppm > 0 else not any(active.values()), (h, w, active)
            clamped += 1
    assert clamped >= 8 or abs(ppm) != 50000


@pytest.mark.parametrize('dtype', warp_cases.DTYPES)
def test_more_planes_than_a_thread_walks_over(dtype):
    h, w, n = warp_cases.MANY
    assert warp_cases.WALK < n < 2 * warp_cases.WALK
    planes = warp_cases.planes(dtype, h, w, n)
    for ppm in (0, -50000, 50000, 1500):
        got = native.warp_tiles(_dev(planes), ppm)
        np.testing.assert_array_equal(got.cpu().numpy(), warp_cases.reference(dtype, h, w, ppm, n))
    # a stack with two leading dimensions is the same run of planes
    got = native.warp_tiles(_dev(planes[:22].reshape(2, 11, h, w)), -1500)
    np.testing.assert_array_equal(got.cpu().numpy().reshape(22, h, w), warp_cases.reference(dtype, h, w, -1500, n)[:22])


def test_more_planes_than_one_launch_takes():
    """65535 runs of 16 planes go into one launch: one plane more, of 1 x 1 and of 1 x 2 pixels, through the C entry (the
    wrapper's layout of such a stack is the same call)."""
    import torch
    n = 65535 * native.SQ_WARP_PLANES_PER_THREAD + 1
    src = torch.arange(2 * n, dtype=torch.int32, device=DEV).remainder(251).to(torch.uint8)
    out = torch.full((2 * n,), 255, dtype=torch.uint8, device=DEV)
    L = native.lib()
    assert L.sq_warp_tiles(src.data_ptr(), out.data_ptr(), n, 1, 1, 1, 1, 1, 1, native.SQ_U8, 50000, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:n], src[:n]) and bool((out[n:] == 255).all())      # 1 x 1: the identity, plane for plane
    out.fill_(255)
    assert L.sq_warp_tiles(src.data_ptr(), out.data_ptr(), n, 1, 2, 2, 2, 2, 2, native.SQ_U8, -50000, None) == 0
    torch.cuda.synchronize()
    # 1 x 2 at -50000: U = 1, R2 = 1, rho = 2^24 at both pixels, du = +-6: out = (a*250 + b*6 + 128) >> 8 and its mirror image
    a, b = src[0::2].to(torch.int32), src[1::2].to(torch.int32)
    want = torch.stack([(a * 250 + b * 6 + 128) >> 8, (a * 6 + b * 250 + 128) >> 8], dim=1).to(torch.uint8).reshape(-1)
    assert warp_ref.loop(np.array([[10, 200]], np.uint8), -50000).tolist() == [[(10 * 250 + 200 * 6 + 128) >> 8,
                                                                               (10 * 6 + 200 * 250 + 128) >> 8]]
    assert torch.equal(out, want)


@pytest.mark.parametrize('dtype', warp_cases.DTYPES)
@pytest.mark.parametrize('ppm', [-50000, 1500])
def test_views_pitches_offsets_guard_and_repeatability(ppm, dtype):
    import torch
    h, w = 9, 37
    planes = warp_cases.planes(dtype, h, w)
    n_planes = len(planes)
    tdtype = native.torch_dtype_of(np.dtype(dtype))
    fill = int(np.iinfo(np.dtype(dtype)).max) // 3
    want = warp_cases.reference(dtype, h, w, ppm)
    # every other plane of a stack, as source and as destination; the planes between stay as they are
    big = _dev(planes)
    out_big = _full((n_planes + 1, h, w), fill, dtype)
    got = native.warp_tiles(big[::2], ppm, out=out_big[1::2])
    assert got.data_ptr() == out_big[1::2].data_ptr()
    np.testing.assert_array_equal(out_big.cpu().numpy()[1::2], want[::2])
    assert (out_big.cpu().numpy()[::2] == fill).all()
    np.testing.assert_array_equal(big.cpu().numpy(), planes)
    # a pitched source and a pitched destination: the columns beyond w of dst stay as they are
    wide_src = _dev(np.concatenate([planes, np.full((n_planes, h, 5), 7, planes.dtype)], axis=2))
    wide_dst = _full((n_planes, h, w + 3), fill, dtype)
    native.warp_tiles(wide_src[:, :, :w], ppm, out=wide_dst[:, :, :w])
    np.testing.assert_array_equal(wide_dst.cpu().numpy()[:, :, :w], want)
    assert (wide_dst.cpu().numpy()[:, :, w:] == fill).all()
    # a source and a destination that each start at an element offset, through every phase of 16 bytes -- 8 uint16 / 16 uint8
    # -- plus one pair beyond it: the destination's phase decides between the packed store of a run (4 or 2 bytes) and the
    # element stores, and the source's phase puts the pair loads on every alignment an element allows.  Both are views of wider
    # buffers whose row pitch is a multiple of 16 bytes.
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
            got = native.warp_tiles(src_off, ppm, out=out_off[:, :, :w])
            np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f'src offset {s_off}, dst offset {d_off}')
            host = obuf.cpu().numpy()
            assert (host[:d_off] == fill).all() and (host[n_el + d_off:] == fill).all()
            assert (host[d_off:n_el + d_off].reshape(n_planes, h, pitch)[:, :, w:] == fill).all()      # between w and the pitch
    np.testing.assert_array_equal(buf[s_off:n_el + s_off].cpu().numpy(), padded.reshape(-1))
    # a guard band of 0xA5 in front of and behind out stays intact
    nbytes = want.size * planes.itemsize
    raw = torch.full((4096 + nbytes + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    out = raw[4096:4096 + nbytes].view(tdtype).view(n_planes, h, w)
    native.warp_tiles(_dev(planes), ppm, out=out)
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    assert bool((raw[:4096] == 0xA5).all()) and bool((raw[4096 + nbytes:] == 0xA5).all())
    # the same call twice: the same bytes
    runs = [native.warp_tiles(_dev(planes), ppm).cpu().numpy().tobytes() for _ in range(2)]
    assert runs[0] == runs[1] == want.tobytes()


def test_refusals():
    import torch
    t_np = np.arange(3 * 8 * 12, dtype=np.uint16).reshape(3, 8, 12)
    t = _dev(t_np)
    out = _full((3, 8, 12), 7, 'uint16')
    for ppm in (50001, -50001, 2.0, True, None, '2'):
        with pytest.raises(ValueError):
            native.warp_tiles(t, ppm, out=out)
    with pytest.raises(ValueError):
        native.warp_tiles(t.to(torch.float32), 2, out=out)                      # a wrong dtype
    with pytest.raises(ValueError):
        native.warp_tiles(t.permute(0, 2, 1), 2)                                # rows that are not contiguous
    with pytest.raises(ValueError):
        native.warp_tiles(t, 2, out=_full((3, 12, 8), 7, 'uint16').permute(0, 2, 1))
    with pytest.raises(ValueError):
        native.warp_tiles(t, 2, out=out[:2])                                    # another shape
    with pytest.raises(ValueError):
        native.warp_tiles(t, 2, out=_full((3, 8, 12), 7, 'uint8'))              # another dtype
    with pytest.raises(ValueError):
        native.warp_tiles(t, 2, out=torch.zeros((3, 8, 12), dtype=torch.uint16))            # another device
    assert (out.cpu().numpy() == 7).all()      # nothing was launched
    # an out that shares memory with tiles
    before = t.cpu().numpy()
    with pytest.raises(ValueError):
        native.warp_tiles(t, 2, out=t)
    with pytest.raises(ValueError):
        native.warp_tiles(t[:2], 2, out=t[1:])
    with pytest.raises(ValueError):
        native.warp_tiles(t[::2], 2, out=t[1:3])
    np.testing.assert_array_equal(t.cpu().numpy(), before)
    # the library itself refuses what the wrapper would let through
    L = native.lib()

    def call(src=t.data_ptr(), dst=out.data_ptr(), n=3, h=8, w=12, sps=96, sp=12, dps=96, dp=12, dtype=native.SQ_U16, ppm=1500):
        return L.sq_warp_tiles(src, dst, n, h, w, sps, sp, dps, dp, dtype, ppm, None)

    assert call() == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), warp_ref.warp_image(t_np, 1500))
    assert call(ppm=0) == 0                                              # ppm = 0 is accepted: an exact copy
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), t_np)
    out.copy_(_full((3, 8, 12), 7, 'uint16'))
    torch.cuda.synchronize()
    assert call(n=0) == 0 and call(n=0, src=None, dst=None) == 0      # no image: SQ_OK, nothing launched
    for bad in (dict(ppm=50001), dict(ppm=-50001), dict(dtype=native.SQ_F32), dict(dtype=0), dict(sp=11), dict(dp=11),
                dict(sps=95), dict(dps=95), dict(src=None), dict(dst=None), dict(src=t.data_ptr() + 1),
                dict(dst=out.data_ptr() + 1), dict(n=-1), dict(dst=t.data_ptr() + 96 * 2), dict(dst=t.data_ptr()),
                dict(src=out.data_ptr(), n=1), dict(h=0), dict(w=0), dict(h=-1)):
        assert call(**bad) == -1, bad      # SQ_ERR_INVALID
    for big in (dict(h=65536, sps=65536 * 12, dps=65536 * 12), dict(w=65536, sp=65536, dp=65536, sps=8 * 65536, dps=8 * 65536)):
        assert call(**big) == native.SQ_ERR_UNSUPPORTED, big
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7).all()
    np.testing.assert_array_equal(t.cpu().numpy(), before)


# ---------------------------------------------------------------------------------------------------- off the default stream
def _stream_call(ppm):
    def call(ctx, inp, out, stream):
        native.warp_tiles(inp['tiles'], ppm, out=out['out'], stream=stream)
        return {'out': out['out']}
    return call


def _stream_case(dtype, ppm):
    top = int(np.iinfo(dtype).max)
    shape = (4, 50, 70)
    real = {'tiles': np.random.default_rng(310).integers(0, top + 1, shape).astype(dtype)}
    poison = {'tiles': np.random.default_rng(311).integers(0, top + 1, shape).astype(dtype)}
    canary = {'out': np.full(shape, 7, dtype)}
    return SC.Case(f'warp-tiles-{np.dtype(dtype).name}-{ppm}', real, poison, canary, _stream_call(ppm),
                   lambda a, strict: {'out': warp_ref.warp_image(a['tiles'], ppm)})


STREAM_CASES = {c.name: c for c in (_stream_case(np.uint16, 20000), _stream_case(np.uint8, -50000))}


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
NOTE = '_stitched_distortion.json'
BIN_NOTE = '_stitched_binning.json'
LEFT, RIGHT, FLUO = 'BF LED matrix left half', 'BF LED matrix right half', 'Fluorescence 488 nm Ex'
APPLIES_TO = 'every tile, before binning, placement, registration, the flatfield estimate and every tile filter'


def prewarp_folder(root, ppm, then_bin=1):
    """F -> F' in place: every tile file corrected by the definition (and then, for the run with --tile-binning too, binned by
    its definition, the sensor pixel multiplied), the rest as it is."""
    n = changed = 0
    for folder, _, names in os.walk(root):
        for name in names:
            if name.lower().endswith(('.tif', '.tiff')):
                path = os.path.join(folder, name)
                img = tiffio.read_image(path)
                new = warp_ref.warp_file_image(img, ppm)
                changed += int((new != img).any())
                tiffio.write_tiff(path, new if then_bin == 1 else bin_ref.bin_file_image(new, then_bin, 'mean'))
                n += 1
    assert n > 0 and changed == n      # F' is not F
    if then_bin > 1:
        path = os.path.join(root, 'acquisition parameters.json')
        with open(path) as fh:
            ap = json.load(fh)
        ap['sensor_pixel_size_um'] = ap['sensor_pixel_size_um'] * then_bin
        with open(path, 'w') as fh:
            json.dump(ap, fh, indent=2)
    return n


def _two_roots(tmp_path, spec, ppm=D, then_bin=1):
    a, b = str(tmp_path / 'with_flag' / 'acq'), str(tmp_path / 'prewarped' / 'acq')
    for r in (a, b):
        synth.write_acquisition(spec, r)
    prewarp_folder(b, ppm, then_bin)
    return a, b


def _cli(root, *extra):
    """One run through the command line -> its output folder."""
    random.seed(1234)
    stitcher_cli.main(['-i', root, '--normalization', 'none', *extra])
    base = os.path.dirname(root)
    outs = [d for d in os.listdir(base) if d.startswith(os.path.basename(root) + '_stitched_')]
    assert len(outs) == 1
    return os.path.join(base, outs[0])


def _api(root, params=None, batch_bytes_limit=None, **kw):
    """One run of a Stitcher made by hand -> the Stitcher."""
    random.seed(1234)
    st = Stitcher(StitchingParameters(input_folder=root, **(params or {})), normalization=None, **kw)
    if batch_bytes_limit is not None:
        st.batch_bytes_limit = batch_bytes_limit
    st.run()
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


def _shifts(out):
    with open(os.path.join(out, 'shift_table.json')) as fh:
        return json.load(fh)['shifts'][0]


def test_coordinate_placement_and_the_note(tmp_path, capsys):
    spec = spec_of(load_case('coord_3x4_small')[0])
    a, b = _two_roots(tmp_path, spec)
    capsys.readouterr()
    got = _cli(a, '--distortion-correction', str(D))
    assert capsys.readouterr().out.count('[distortion]') == 1
    want = _cli(b)
    assert '[distortion]' not in capsys.readouterr().out
    _same_trees(got, want)
    assert _notes(got) == [os.path.join('0_stitched', 'R0' + NOTE)]
    with open(os.path.join(got, '0_stitched', 'R0' + NOTE)) as fh:
        note = json.load(fh)
    du, dv, _, _ = warp_ref.maps(spec.tile_h, spec.tile_w, D)
    assert note == {'ppm': D, 'tile_shape': [spec.tile_h, spec.tile_w], 'max_abs_du_256': int(np.abs(du).max()),
                    'max_abs_dv_256': int(np.abs(dv).max()), 'edges': 'replicated', 'interpolation': 'bilinear, 8 fractional bits',
                    'applies_to': APPLIES_TO}
    assert note['max_abs_du_256'] > 256      # more than a pixel at the corners
    # ... and the run on F without the flag is another tree
    third = str(tmp_path / 'plain' / 'acq')
    synth.write_acquisition(spec, third)
    plain = _tree(_cli(third))
    assert sorted(plain) == sorted(_tree(got)) and plain != _tree(got)


@pytest.mark.parametrize('case,on_f,on_f_prime', [('reg_3x4_small', [3, -44], [3, -45]), ('reg_spattern', [-2, -48], [-2, -49])])
def test_registration_and_device_basic_flatfield(tmp_path, case, on_f, on_f_prime):
    info, _ = load_case(case)
    a, b = _two_roots(tmp_path, spec_of(info))
    flags = ('-r', '-ff', '--flatfield-estimator', 'basic', '-s', info['spec']['scan_pattern'])
    got, want = _cli(a, *flags, '--distortion-correction', str(D)), _cli(b, *flags)
    tree = _same_trees(got, want)
    assert 'shift_table.json' in tree and 'flatfield_info.json' in tree
    shifts = _shifts(got)
    assert shifts['h_shift'] != [0, 0] and shifts['v_shift'] != [0, 0]
    assert ('h_shift_rev' in shifts) == (case == 'reg_spattern')
    # the registration read corrected tiles: the shifts are those of F', not those of a run on F without the flag (the numpy
    # oracle's values for both folders)
    third = str(tmp_path / 'plain' / 'acq')
    synth.write_acquisition(spec_of(info), third)
    plain = _shifts(_cli(third, *flags))
    # (reg_spattern: the values of its right-to-left rows, whichever of the two keys the centre row makes them)
    assert on_f_prime in (shifts['h_shift'], shifts.get('h_shift_rev')) and on_f in (plain['h_shift'], plain.get('h_shift_rev'))
    assert shifts['h_shift'] != plain['h_shift'] and shifts['h_shift'] != [0, 0] != plain['h_shift']


def test_uint8_rgb_files(tmp_path):
    a, b = _two_roots(tmp_path, spec_of(load_case('coord_rgb')[0]))
    tree = _same_trees(_cli(a, '--distortion-correction', str(D)), _cli(b))
    assert len(tree) > 4


@pytest.mark.parametrize('flag', ['all_pairs_registration', 'global_registration'])
def test_all_pairs_and_global_registration(tmp_path, flag):
    info, _ = load_case('reg_3x4_small')
    a, b = _two_roots(tmp_path, spec_of(info))
    params = dict(use_registration=True, registration_channel=info['params']['registration_channel'],
                  registration_z_level=info['params']['registration_z_level'])
    got, want = _api(a, params, distortion_correction=D, **{flag: True}), _api(b, params, **{flag: True})
    tree = _same_trees(got.output_folder, want.output_folder)
    assert got.pair_table.shape == want.pair_table.shape and got.pair_table.tobytes() == want.pair_table.tobytes()
    assert len(got.pair_table) == 17 and (got.h_shift, got.v_shift) == (want.h_shift, want.v_shift) != ((0, 0), (0, 0))
    assert (os.path.join('0_stitched', 'R0_tile_positions.csv') in tree) == (flag == 'global_registration')
    third = str(tmp_path / 'plain' / 'acq')
    synth.write_acquisition(spec_of(info), third)
    plain = _api(third, params, **{flag: True})
    assert plain.pair_table.tobytes() != got.pair_table.tobytes()      # the stack was corrected before it was registered
    assert (plain.h_shift, plain.v_shift) != (got.h_shift, got.v_shift)


def test_every_option_together(tmp_path):
    """... including --tile-binning 2: corrected first, in sensor pixels, binned second -- a run on bin_2(F')."""
    spec = synth.GridSpec(rows=2, cols=3, tile_h=96, tile_w=128, ov_y=24, ov_x=40, nz=2, channels=(LEFT, RIGHT, FLUO), seed=23)
    a, b = _two_roots(tmp_path, spec, then_bin=2)
    kw = dict(dpc=True, despeckle='hot', despeckle_threshold=40, background_subtract='tophat', background_radius=5, tile_qc=True,
              seam_qc=True, z_projection='focus', focus_depth_map=True, contrast_limits='percentile', composite=True,
              pyramid_method='mean')
    got, want = _api(a, distortion_correction=D, tile_binning=2, **kw), _api(b, **kw)
    tree = _same_trees(got.output_folder, want.output_folder, skip=(NOTE, BIN_NOTE))
    assert _notes(got.output_folder, BIN_NOTE) and not _notes(want.output_folder, BIN_NOTE)
    for part in ('_edf.ome.zarr', '_depth.ome.zarr', '_tile_qc.csv', '_tile_qc.json', '_seam_qc.csv', '_seam_qc.json',
                 '_histogram.npy', '_stats.json', '.png', '_despeckle.json', '_background.json', '_dpc.json'):
        assert any(part in k for k in tree), part
    assert got.tile_qc_table and got.tile_qc_table == want.tile_qc_table
    assert got.seam_qc_table and got.seam_qc_table == want.seam_qc_table
    assert len(got.seam_qc_table[(0, 'R0')]) > 0 and got.tile_qc_table[(0, 'R0')][0]['pixels'] == 48 * 64
    assert got.despeckle_replaced == want.despeckle_replaced and got.despeckle_staged == want.despeckle_staged
    # the same options without the binning: a run on F'
    c, d = _two_roots(tmp_path / 'unbinned', spec)
    got, want = _api(c, distortion_correction=D, **kw), _api(d, **kw)
    _same_trees(got.output_folder, want.output_folder)
    assert got.tile_qc_table[(0, 'R0')][0]['pixels'] == 96 * 128 and got.seam_qc_table == want.seam_qc_table


def test_feather_fusion(tmp_path):
    a, b = _two_roots(tmp_path, spec_of(load_case('coord_3x4_small')[0]))
    _same_trees(_cli(a, '--fusion-mode', 'feather', '--distortion-correction', str(D)), _cli(b, '--fusion-mode', 'feather'))


def test_ome_tiff_output(tmp_path):
    a, b = _two_roots(tmp_path, spec_of(load_case('coord_3x4_small')[0]), ppm=-D)
    tree = _same_trees(_cli(a, '-f', '.ome.tiff', '--distortion-correction', str(-D)), _cli(b, '-f', '.ome.tiff'))
    assert any(k.endswith('.ome.tiff') for k in tree)


@pytest.mark.parametrize('dpc', [False, True])
def test_small_batches_use_both_ingest_slots(tmp_path, dpc):
    """One plane per chunk: the one corrected buffer is written by every chunk while the two raw slots alternate (with --dpc the
    right halves' buffers turn over too)."""
    spec = synth.GridSpec(rows=2, cols=3, tile_h=96, tile_w=128, ov_y=24, ov_x=40, nz=2,
                          channels=(LEFT, RIGHT, FLUO) if dpc else tuple(synth.DEFAULT_CHANNELS[:2]), seed=29)
    a, b = _two_roots(tmp_path, spec)
    got, want = _api(a, batch_bytes_limit=1, distortion_correction=D, dpc=dpc), _api(b, batch_bytes_limit=1, dpc=dpc)
    _same_trees(got.output_folder, want.output_folder)
    ingest = [k for k in got._buffer_cache if k[0] == 'ingest']
    assert len(ingest) == 1 and ingest[0][1] == 1 and ingest[0][5] == 2      # a batch of one plane, two slots
    assert got.num_c * got.num_z >= 4                                       # one rectangle list, at least three chunks
    warped = [k for k in got._buffer_cache if k[0] == 'distortion']
    assert len(warped) == 1 and warped[0][1:5] == (1, 6, 96, 128)           # ONE buffer of the files' shape for both slots
    assert not [k for k in want._buffer_cache if str(k[0]).startswith('distortion')]
    assert bool([k for k in got._buffer_cache if k[0] == 'distortion-dpc']) == dpc
    # ... and the same stores as the run in one batch
    third = str(tmp_path / 'one_batch' / 'acq')
    synth.write_acquisition(spec, third)
    whole = _api(third, distortion_correction=D, dpc=dpc)
    assert _tree(whole.output_folder) == _tree(got.output_folder)


def test_z_levels_timepoints_and_unequal_regions(tmp_path):
    info, _ = load_case('coord_unequal_wells')
    spec = spec_of(dict(info, spec=dict(info['spec'], nz=2)))
    assert spec.nt == 2 and len(spec.regions) == 2 and spec.region_dims
    a, b = _two_roots(tmp_path, spec)
    got, want = _cli(a, '--distortion-correction', str(D)), _cli(b)
    tree = _same_trees(got, want)
    assert _notes(got) == sorted(os.path.join(f'{t}_stitched', r + NOTE) for t in range(2) for r in spec.regions)
    assert len({k.split(os.sep)[0] for k in tree}) == 2


def test_default_is_untouched(tmp_path, capsys):
    info, _ = load_case('coord_3x4_small')
    roots = [str(tmp_path / k / 'acq') for k in ('zero', 'none', 'api')]
    for r in roots:
        synth.write_acquisition(spec_of(info), r)
    capsys.readouterr()
    zero = _cli(roots[0], '--distortion-correction', '0')
    printed_zero = capsys.readouterr().out
    none = _cli(roots[1])
    printed_none = capsys.readouterr().out
    assert _tree(zero, skip=()) and _tree(zero, skip=()) == _tree(none, skip=())
    assert not [n for _, _, names in os.walk(str(tmp_path)) for n in names if n.endswith(NOTE)]      # no note
    # the printed lines: the same but for the folders' own names
    # the printed lines: the same but for the folders' own names and the numbers (times, the output folder's date)
    plain = lambda text, root: sorted(re.sub(r'\d+(\.\d+)?', '#', line.replace(os.path.dirname(root), '<root>'))
                                      for line in text.splitlines())
    assert plain(printed_zero, roots[0]) == plain(printed_none, roots[1]) and len(plain(printed_zero, roots[0])) > 3
    assert 'distortion' not in printed_zero.replace('--distortion-correction', '')
    st = Stitcher(StitchingParameters(input_folder=roots[2]), normalization=None, distortion_correction=0)
    st.get_timepoints()
    st.extract_acquisition_parameters()
    st.get_pixel_size()
    st.parse_acquisition_metadata()
    st.stitch_region(0, 'R0')
    assert st._buffer_cache and not [k for k in st._buffer_cache if str(k[0]).startswith('distortion')]


# ---------------------------------------------------------------------------------------------------- finding D
def test_scan_tool_finds_the_coefficient_of_a_distorted_folder(tmp_path, capsys):
    """tools/distortion_scan.py on the tiles of reg_3x4_small distorted beforehand at -D (the lens): of 0, D and 2 D the median
    best-offset ncc of the seams is highest at D, where no seam is shifted any more; the scan leaves nothing behind."""
    import importlib.util
    root_dir = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mod_spec = importlib.util.spec_from_file_location('distortion_scan', os.path.join(root_dir, 'tools', 'distortion_scan.py'))
    tool = importlib.util.module_from_spec(mod_spec)
    mod_spec.loader.exec_module(tool)
    info, _ = load_case('reg_3x4_small')
    root = str(tmp_path / 'lens' / 'acq')
    synth.write_acquisition(spec_of(info), root)
    prewarp_folder(root, -D)
    before = sorted(os.listdir(os.path.dirname(root)))
    found = tool.main(['-i', root, '-r', '--', '0', str(D), str(2 * D)])
    assert [f[0] for f in found] == [0, D, 2 * D] and all(f[3] > 0 for f in found)
    assert found[1][1] > found[0][1] and found[1][1] > found[2][1]
    # (the shifted seams: none at D, most of them at 0; at 2 D the registration of this run absorbs what is left of them)
    assert found[1][2] == 0 < found[0][2] and found[1][2] <= found[2][2]
    assert f'highest median: D = {D}' in capsys.readouterr().out
    assert sorted(os.listdir(os.path.dirname(root))) == before
