"""--tile-binning on the device: sq_bin_tiles against the numpy definition (tests/bin_ref.py), and whole runs with the option
against runs without it on a folder of files binned beforehand.  Every comparison is equality."""
import hashlib
import json
import math
import os
import random

import numpy as np
import pytest

import bin_cases
import bin_ref
import stream_cases as SC
from helpers import load_case, spec_of
from image_stitcher_amd import native, stitcher_cli, synth, tiffio
from image_stitcher_amd.stitcher import Stitcher
from image_stitcher_amd.stitcher_parameters import StitchingParameters

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the cached planes are read-only)


def _full(shape, value, dtype):
    return _dev(np.full(shape, value, dtype=np.dtype(dtype)))


# ---------------------------------------------------------------------------------------------------- the kernel
# (the shapes and the kernel's own sizes they are chosen from: tests/bin_cases.py)
@pytest.mark.parametrize('dtype', bin_cases.DTYPES)
@pytest.mark.parametrize('k', bin_cases.FACTORS)
def test_kernel_equals_the_definition(k, dtype):
    top = int(np.iinfo(np.dtype(dtype)).max)
    shares, vector = [], 0
    for h, w in bin_cases.shapes(k):
        planes = bin_cases.planes(dtype, k, h, w)
        src = _dev(planes)
        vector += bin_cases.takes_vector_loads(dtype, k, h, w, first_element=(src.data_ptr() // src.element_size()) % (16 // src.element_size()))
        for method in ('mean', 'sum'):
            want = bin_cases.reference(dtype, k, h, w, method)
            got = native.bin_tiles(src, k, method)
            assert got.dtype == src.dtype and tuple(got.shape) == (len(planes), h // k, w // k)
            host = got.cpu().numpy()
            for i, name in enumerate(bin_cases.PLANE_NAMES):
                np.testing.assert_array_equal(host[i], want[i], err_msg=f'{(h, w)} K={k} {method} {name}')
        np.testing.assert_array_equal(src.cpu().numpy(), planes)      # the source is left as it was
        if (h // k) * (w // k) >= 1000:
            # 'sum' on the noise of range [0, 2 M / K^2], in what the kernel wrote (`host` is the 'sum' result): neither
            # branch of the clamp goes unexercised
            share = bin_ref.saturated_share(host[bin_cases.LOW_NOISE])
            assert 0.1 < share < 0.9, (h, w, share)
            assert share == bin_ref.saturated_share(bin_cases.reference(dtype, k, h, w, 'sum')[bin_cases.LOW_NOISE])
            assert (host[bin_cases.LOW_NOISE] < top).any()
            shares.append(share)
    assert vector >= 3      # (the device's allocations start on 16-byte boundaries: the shapes made for the vector loads take them)
    assert len(shares) >= 3


@pytest.mark.parametrize('dtype', bin_cases.DTYPES)
@pytest.mark.parametrize('k', [2, 3, 6, 7, 8])
def test_views_pitches_offsets_guard_and_repeatability(k, dtype):
    import torch
    h, w = 9 * k + 1, 37 * k + k - 1
    hb, wb = 9, 37
    planes = bin_cases.planes(dtype, k, h, w)
    n_planes = len(planes)
    tdtype = native.torch_dtype_of(np.dtype(dtype))
    fill = int(np.iinfo(np.dtype(dtype)).max) // 3
    want = bin_cases.reference(dtype, k, h, w, 'mean')
    want_sum = bin_cases.reference(dtype, k, h, w, 'sum')
    # every other plane of a stack, as source and as destination; the planes between stay as they are
    big = _dev(planes)
    out_big = _full((n_planes, hb, wb), fill, dtype)
    got = native.bin_tiles(big[::2], k, 'mean', out=out_big[1::2])
    assert got.data_ptr() == out_big[1::2].data_ptr()
    np.testing.assert_array_equal(out_big.cpu().numpy()[1::2], want[::2])
    assert (out_big.cpu().numpy()[::2] == fill).all()
    np.testing.assert_array_equal(big.cpu().numpy(), planes)
    # a pitched source and a pitched destination: the columns beyond wb of dst stay as they are
    wide_src = _dev(np.concatenate([planes, np.full((n_planes, h, 5), 7, planes.dtype)], axis=2))
    wide_dst = _full((n_planes, hb, wb + 3), fill, dtype)
    native.bin_tiles(wide_src[:, :, :w], k, 'sum', out=wide_dst[:, :, :wb])
    np.testing.assert_array_equal(wide_dst.cpu().numpy()[:, :, :wb], want_sum)
    assert (wide_dst.cpu().numpy()[:, :, wb:] == fill).all()
    # a source and a destination that each start at an element offset, in every combination of phases a vector has -- 16
    # bytes hold 8 uint16 / 16 uint8 -- plus one pair beyond it.  Both are views of wider buffers whose row pitch is a multiple
    # of 16 bytes, so the K rows of a block share one phase: wherever K can reach the source's phase the runs are shifted onto
    # it (a run that starts in front of the row, runs read with 16-byte loads, a partial run at the row's end), and the
    # destination's phase decides between the packed store and the element stores.  Elsewhere: element by element.
    vec = 16 // planes.itemsize
    outs = bin_cases.run_columns(dtype, k)
    sp, dp = (w + vec - 1) // vec * vec + vec, (wb + vec - 1) // vec * vec + vec      # the pitches
    n_src, n_dst = n_planes * h * sp, n_planes * hb * dp
    padded = np.full((n_planes, h, sp), 7, planes.dtype)
    padded[:, :, :w] = planes
    padded_dev = _dev(padded).reshape(-1)
    vector_pairs = packed = unpacked = 0
    for s_off in list(range(vec)) + [vec + 3]:
        buf = _full((n_src + 2 * vec + 8,), 0, dtype)
        buf[s_off:n_src + s_off] = padded_dev
        src_off = buf[s_off:n_src + s_off].view(n_planes, h, sp)[:, :, :w]
        s_phase = (src_off.data_ptr() // planes.itemsize) % vec
        assert s_phase == s_off % vec
        for d_off in list(range(vec)) + [vec + 1]:
            obuf = _full((n_dst + 2 * vec + 8,), fill, dtype)
            out_off = obuf[d_off:n_dst + d_off].view(n_planes, hb, dp)
            got = native.bin_tiles(src_off, k, 'mean', out=out_off[:, :, :wb])
            np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f'src offset {s_off}, dst offset {d_off}')
            host = obuf.cpu().numpy()
            assert (host[:d_off] == fill).all() and (host[n_dst + d_off:] == fill).all()
            assert (host[d_off:n_dst + d_off].reshape(n_planes, hb, dp)[:, :, wb:] == fill).all()      # between wb and the pitch
            if bin_cases.takes_vector_loads(dtype, k, h, w, pitch=sp, first_element=s_phase):
                # the shifts that align the source, and whether one of them aligns the store too (csrc/bin.hip)
                shifts = [t for t in range(outs) if (k * t - s_phase) % vec == 0]
                vector_pairs += 1
                packed += (d_off % outs) in shifts
                unpacked += (d_off % outs) not in shifts
    np.testing.assert_array_equal(buf[s_off:n_src + s_off].cpu().numpy(), padded.reshape(-1))
    # K odd reaches every source phase, K = 2 and 6 every other one, K = 8 only its own; the store is packed in some pairs
    # and not in others unless a run is one element
    assert vector_pairs >= vec * (vec + 1) // math.gcd(k, vec) and packed > 0
    assert unpacked > 0 or outs == 1
    # a guard band of 0xA5 in front of and behind out stays intact
    nbytes = want.size * planes.itemsize
    raw = torch.full((4096 + nbytes + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    out = raw[4096:4096 + nbytes].view(tdtype).view(n_planes, hb, wb)
    native.bin_tiles(_dev(planes), k, 'mean', out=out)
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    assert bool((raw[:4096] == 0xA5).all()) and bool((raw[4096 + nbytes:] == 0xA5).all())
    # the same call twice: the same bytes
    runs = [native.bin_tiles(_dev(planes), k, 'sum').cpu().numpy().tobytes() for _ in range(2)]
    assert runs[0] == runs[1] == want_sum.tobytes()


def test_refusals():
    import torch
    t_np = np.arange(3 * 8 * 12, dtype=np.uint16).reshape(3, 8, 12)
    t = _dev(t_np)
    out = _full((3, 4, 6), 7, 'uint16')
    for factor in (1, 9, 0, -2, 2.0, True, None, '2'):
        with pytest.raises(ValueError):
            native.bin_tiles(t, factor, out=out)
    for method in ('median', None, 1, 'MEAN'):
        with pytest.raises(ValueError):
            native.bin_tiles(t, 2, method, out=out)
    with pytest.raises(ValueError):
        native.bin_tiles(t.to(torch.float32), 2, out=out)                      # a wrong dtype
    with pytest.raises(ValueError):
        native.bin_tiles(t.permute(0, 2, 1), 2, out=out)                       # rows that are not contiguous
    with pytest.raises(ValueError):
        native.bin_tiles(t, 2, out=_full((3, 6, 4), 7, 'uint16').permute(0, 2, 1))
    with pytest.raises(ValueError):
        native.bin_tiles(t, 2, out=out[:2])                                    # another shape
    with pytest.raises(ValueError):
        native.bin_tiles(t, 2, out=_full((3, 8, 12), 7, 'uint16'))             # the unbinned shape
    with pytest.raises(ValueError):
        native.bin_tiles(t, 2, out=_full((3, 4, 6), 7, 'uint8'))               # another dtype
    with pytest.raises(ValueError):
        native.bin_tiles(t, 2, out=torch.zeros((3, 4, 6), dtype=torch.uint16))             # another device
    with pytest.raises(ValueError):
        native.bin_tiles(t[:, :, :7], 8)                                       # wb < 1
    with pytest.raises(ValueError):
        native.bin_tiles(t[:, :7], 8)                                          # hb < 1
    assert (out.cpu().numpy() == 7).all()      # nothing was launched
    # an out that shares memory with tiles
    before = t.cpu().numpy()
    with pytest.raises(ValueError):
        native.bin_tiles(t, 2, out=t.view(-1)[:72].view(3, 4, 6))
    with pytest.raises(ValueError):
        native.bin_tiles(t[:2], 2, out=t[1].reshape(-1)[:48].view(2, 4, 6))
    np.testing.assert_array_equal(t.cpu().numpy(), before)
    # the library itself refuses what the wrapper would let through
    L = native.lib()

    def call(src=t.data_ptr(), dst=out.data_ptr(), n=3, h=8, w=12, sps=96, sp=12, dps=24, dp=6, dtype=native.SQ_U16, factor=2,
             method=native.SQ_BIN_MEAN):
        return L.sq_bin_tiles(src, dst, n, h, w, sps, sp, dps, dp, dtype, factor, method, None)

    assert call() == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), bin_ref.bin_image(t_np, 2, 'mean'))
    out.copy_(_full((3, 4, 6), 7, 'uint16'))
    torch.cuda.synchronize()
    assert call(n=0) == 0 and call(n=0, src=None, dst=None) == 0      # no image: SQ_OK, nothing launched
    for bad in (dict(method=0), dict(method=3), dict(dtype=native.SQ_F32), dict(dtype=0), dict(factor=1), dict(factor=9),
                dict(factor=0), dict(h=1), dict(w=1), dict(factor=8, w=7, sp=12), dict(sp=11), dict(dp=5), dict(sps=95), dict(dps=23),
                dict(src=None), dict(dst=None), dict(src=t.data_ptr() + 1), dict(dst=out.data_ptr() + 1), dict(n=-1),
                dict(dst=t.data_ptr() + 96 * 2), dict(dst=t.data_ptr()), dict(src=out.data_ptr(), n=1), dict(h=0), dict(w=0)):
        assert call(**bad) == -1, bad      # SQ_ERR_INVALID
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7).all()
    np.testing.assert_array_equal(t.cpu().numpy(), before)


# ---------------------------------------------------------------------------------------------------- off the default stream
def _stream_call(k, method):
    def call(ctx, inp, out, stream):
        native.bin_tiles(inp['tiles'], k, method, out=out['out'], stream=stream)
        return {'out': out['out']}
    return call


def _stream_case(dtype, k, method):
    top = int(np.iinfo(dtype).max)
    if method == 'sum':      # full-range noise saturates every sum: the range of which about half do
        top = round(2 * top / (k * k))
    shape = (4, 50, 70)
    real = {'tiles': np.random.default_rng(290).integers(0, top + 1, shape).astype(dtype)}
    poison = {'tiles': np.random.default_rng(291).integers(0, top + 1, shape).astype(dtype)}
    canary = {'out': np.full((4, 50 // k, 70 // k), 7, dtype)}
    return SC.Case(f'bin-tiles-{np.dtype(dtype).name}-{k}-{method}', real, poison, canary, _stream_call(k, method),
                   lambda a, strict: {'out': bin_ref.bin_image(a['tiles'], k, method)})


STREAM_CASES = {c.name: c for c in (_stream_case(np.uint16, 2, 'mean'), _stream_case(np.uint8, 3, 'sum'))}


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
NOTE = '_stitched_binning.json'
LEFT, RIGHT, FLUO = 'BF LED matrix left half', 'BF LED matrix right half', 'Fluorescence 488 nm Ex'


def prebin_folder(root, k, method):
    """F -> F/K in place: every tile file binned by the definition, sensor_pixel_size_um multiplied by K, the rest as it is."""
    n = 0
    for folder, _, names in os.walk(root):
        for name in names:
            if name.lower().endswith(('.tif', '.tiff')):
                path = os.path.join(folder, name)
                tiffio.write_tiff(path, bin_ref.bin_file_image(tiffio.read_image(path), k, method))
                n += 1
    assert n > 0
    path = os.path.join(root, 'acquisition parameters.json')
    with open(path) as fh:
        ap = json.load(fh)
    ap['sensor_pixel_size_um'] = ap['sensor_pixel_size_um'] * k
    with open(path, 'w') as fh:
        json.dump(ap, fh, indent=2)
    return n


def _two_roots(tmp_path, spec, k, method='mean'):
    a, b = str(tmp_path / 'with_flag' / 'acq'), str(tmp_path / 'prebinned' / 'acq')
    for r in (a, b):
        synth.write_acquisition(spec, r)
    prebin_folder(b, k, method)
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


def _tree(out):
    """{relative path: digest} of every file of an output tree but the option's own note."""
    found = {}
    for folder, _, names in os.walk(out):
        for name in names:
            if not name.endswith(NOTE):
                with open(os.path.join(folder, name), 'rb') as fh:
                    found[os.path.relpath(os.path.join(folder, name), out)] = hashlib.sha256(fh.read()).hexdigest()
    return found


def _notes(out):
    return sorted(os.path.relpath(os.path.join(folder, n), out) for folder, _, names in os.walk(out) for n in names if n.endswith(NOTE))


def _same_trees(got, want):
    a, b = _tree(got), _tree(want)
    assert a and sorted(a) == sorted(b)
    differ = [k for k in a if a[k] != b[k]]
    assert not differ, differ[:10]
    assert any('.ome.zarr' in k and not os.path.basename(k).startswith('.') for k in a) or any(k.endswith('.ome.tiff') for k in a)
    assert _notes(got) and not _notes(want)
    return a


SPEC_K3 = dict(rows=3, cols=4, tile_h=120, tile_w=136, ov_y=24, ov_x=40, nz=2, channels=tuple(synth.DEFAULT_CHANNELS[:2]), seed=41)


@pytest.mark.parametrize('method', ['mean', 'sum'])
def test_coordinate_placement_k3_with_a_dropped_column(tmp_path, method):
    spec = synth.GridSpec(**SPEC_K3)
    a, b = _two_roots(tmp_path, spec, 3, method)
    flags = ('--tile-binning', '3', '--tile-binning-method', method)
    got, want = _cli(a, *flags), _cli(b)
    _same_trees(got, want)
    assert _notes(got) == [os.path.join('0_stitched', 'R0' + NOTE)]
    with open(os.path.join(got, '0_stitched', 'R0' + NOTE)) as fh:
        note = json.load(fh)
    px = spec.pixel_size_um
    assert note == {'factor': 3, 'method': method, 'file_tile_shape': [120, 136], 'binned_tile_shape': [40, 45],
                    'rows_dropped': 0, 'columns_dropped': 1, 'file_pixel_size_um': px,
                    'pixel_size_um': (spec.sensor_pixel_size_um * 3) / spec.magnification,
                    'applies_to': 'every tile, before placement, registration, the flatfield estimate and every tile filter'}
    if method == 'sum':      # the sum saturates on these tiles: the two methods are told apart
        tile = spec.tile(0, 0)
        assert (bin_ref.bin_image(tile, 3, 'sum') != bin_ref.bin_image(tile, 3, 'mean')).any()


@pytest.mark.parametrize('case', ['reg_3x4_small', 'reg_spattern'])
def test_registration_and_device_basic_flatfield(tmp_path, case):
    info, _ = load_case(case)
    a, b = _two_roots(tmp_path, spec_of(info), 2)
    flags = ('-r', '-ff', '--flatfield-estimator', 'basic', '-s', info['spec']['scan_pattern'])
    got, want = _cli(a, *flags, '--tile-binning', '2'), _cli(b, *flags)
    tree = _same_trees(got, want)
    assert 'shift_table.json' in tree and 'flatfield_info.json' in tree
    with open(os.path.join(got, 'shift_table.json')) as fh:
        shifts = json.load(fh)['shifts'][0]
    assert shifts['h_shift'] != [0, 0] and shifts['v_shift'] != [0, 0]
    assert ('h_shift_rev' in shifts) == (case == 'reg_spattern')


def test_uint8_rgb_files(tmp_path):
    a, b = _two_roots(tmp_path, spec_of(load_case('coord_rgb')[0]), 2)
    tree = _same_trees(_cli(a, '--tile-binning', '2'), _cli(b))
    assert len(tree) > 4


@pytest.mark.parametrize('flag', ['all_pairs_registration', 'global_registration'])
def test_all_pairs_and_global_registration(tmp_path, flag):
    info, _ = load_case('reg_3x4_small')
    a, b = _two_roots(tmp_path, spec_of(info), 2)
    params = dict(use_registration=True, registration_channel=info['params']['registration_channel'],
                  registration_z_level=info['params']['registration_z_level'])
    got, want = _api(a, params, tile_binning=2, **{flag: True}), _api(b, params, **{flag: True})
    tree = _same_trees(got.output_folder, want.output_folder)
    assert got.pair_table.shape == want.pair_table.shape and got.pair_table.tobytes() == want.pair_table.tobytes()
    assert len(got.pair_table) == 17 and (got.h_shift, got.v_shift) == (want.h_shift, want.v_shift) != ((0, 0), (0, 0))
    assert (os.path.join('0_stitched', 'R0_tile_positions.csv') in tree) == (flag == 'global_registration')


def test_every_option_together(tmp_path):
    spec = synth.GridSpec(rows=2, cols=3, tile_h=96, tile_w=128, ov_y=24, ov_x=40, nz=2, channels=(LEFT, RIGHT, FLUO), seed=23)
    a, b = _two_roots(tmp_path, spec, 2)
    kw = dict(dpc=True, despeckle='hot', despeckle_threshold=40, background_subtract='tophat', background_radius=5, tile_qc=True,
              seam_qc=True, z_projection='focus', focus_depth_map=True, contrast_limits='percentile', composite=True,
              pyramid_method='mean')
    got, want = _api(a, tile_binning=2, **kw), _api(b, **kw)
    tree = _same_trees(got.output_folder, want.output_folder)
    for part in ('_edf.ome.zarr', '_depth.ome.zarr', '_tile_qc.csv', '_tile_qc.json', '_seam_qc.csv', '_seam_qc.json',
                 '_histogram.npy', '_stats.json', '.png', '_despeckle.json', '_background.json', '_dpc.json'):
        assert any(part in k for k in tree), part
    assert got.tile_qc_table and got.tile_qc_table == want.tile_qc_table
    assert got.seam_qc_table and got.seam_qc_table == want.seam_qc_table
    assert len(got.seam_qc_table[(0, 'R0')]) > 0 and got.tile_qc_table[(0, 'R0')][0]['pixels'] == 48 * 64
    assert got.despeckle_replaced == want.despeckle_replaced and got.despeckle_staged == want.despeckle_staged


def test_feather_fusion(tmp_path):
    a, b = _two_roots(tmp_path, spec_of(load_case('coord_3x4_small')[0]), 2)
    _same_trees(_cli(a, '--fusion-mode', 'feather', '--tile-binning', '2'), _cli(b, '--fusion-mode', 'feather'))


def test_ome_tiff_output(tmp_path):
    a, b = _two_roots(tmp_path, spec_of(load_case('coord_3x4_small')[0]), 2)
    tree = _same_trees(_cli(a, '-f', '.ome.tiff', '--tile-binning', '2'), _cli(b, '-f', '.ome.tiff'))
    assert any(k.endswith('.ome.tiff') for k in tree)


@pytest.mark.parametrize('dpc', [False, True])
def test_small_batches_use_both_ingest_slots(tmp_path, dpc):
    """One plane per chunk: the one binned buffer is written by every chunk while the two raw slots alternate (with --dpc the
    right halves' buffers turn over too)."""
    spec = synth.GridSpec(rows=2, cols=3, tile_h=96, tile_w=128, ov_y=24, ov_x=40, nz=2,
                          channels=(LEFT, RIGHT, FLUO) if dpc else tuple(synth.DEFAULT_CHANNELS[:2]), seed=29)
    a, b = _two_roots(tmp_path, spec, 2)
    got, want = _api(a, batch_bytes_limit=1, tile_binning=2, dpc=dpc), _api(b, batch_bytes_limit=1, dpc=dpc)
    _same_trees(got.output_folder, want.output_folder)
    ingest = [k for k in got._buffer_cache if k[0] == 'ingest']
    assert len(ingest) == 1 and ingest[0][1] == 1 and ingest[0][5] == 2      # a batch of one plane, two slots
    assert got.num_c * got.num_z >= 4                                       # one rectangle list, at least three chunks
    assert [k for k in got._buffer_cache if k[0] == 'binning'] and not [k for k in want._buffer_cache if k[0].startswith('binning')]
    assert bool([k for k in got._buffer_cache if k[0] == 'binning-dpc']) == dpc
    # ... and the same stores as the run in one batch
    third = str(tmp_path / 'one_batch' / 'acq')
    synth.write_acquisition(spec, third)
    whole = _api(third, tile_binning=2, dpc=dpc)
    assert _tree(whole.output_folder) == _tree(got.output_folder)


def test_z_levels_timepoints_and_unequal_regions(tmp_path):
    info, _ = load_case('coord_unequal_wells')
    spec = spec_of(dict(info, spec=dict(info['spec'], nz=2)))
    assert spec.nt == 2 and len(spec.regions) == 2 and spec.region_dims
    a, b = _two_roots(tmp_path, spec, 2)
    got, want = _cli(a, '--tile-binning', '2'), _cli(b)
    tree = _same_trees(got, want)
    assert _notes(got) == sorted(os.path.join(f'{t}_stitched', r + NOTE) for t in range(2) for r in spec.regions)
    assert len({k.split(os.sep)[0] for k in tree}) == 2


def test_supplied_flatfield_must_have_the_binned_shape(tmp_path):
    root = str(tmp_path / 'acq')
    synth.write_acquisition(spec_of(load_case('coord_3x4_small')[0]), root)
    st = Stitcher(StitchingParameters(input_folder=root, apply_flatfield=True), normalization=None, tile_binning=2)
    st.get_timepoints()
    st.extract_acquisition_parameters()
    st.get_pixel_size()
    st.parse_acquisition_metadata()
    st.flatfields = {0: synth.synthetic_flatfield(96, 128, np.float32)}
    with pytest.raises(ValueError, match=r'\(96, 128\).*\(48, 64\)|\(48, 64\).*\(96, 128\)'):
        st.stitch_region(0, 'R0')
    st.flatfields = {0: synth.synthetic_flatfield(48, 64, np.float32)}
    assert st.stitch_region(0, 'R0').any()


def test_default_is_untouched(tmp_path):
    info, _ = load_case('coord_3x4_small')
    roots = [str(tmp_path / k / 'acq') for k in ('one', 'none', 'api')]
    for r in roots:
        synth.write_acquisition(spec_of(info), r)
    one, none = _cli(roots[0], '--tile-binning', '1', '--tile-binning-method', 'sum'), _cli(roots[1])
    assert _tree(one) and _tree(one) == _tree(none)
    assert not [n for _, _, names in os.walk(str(tmp_path)) for n in names if n.endswith(NOTE)]      # no note
    st = Stitcher(StitchingParameters(input_folder=roots[2]), normalization=None, tile_binning=1)
    st.get_timepoints()
    st.extract_acquisition_parameters()
    st.get_pixel_size()
    st.parse_acquisition_metadata()
    st.stitch_region(0, 'R0')
    assert st._buffer_cache and not [k for k in st._buffer_cache if str(k[0]).startswith('binning')]
    assert (st.input_height, st.input_width) == (st.file_height, st.file_width) == (96, 128)
    assert st.pixel_size_um == st.file_pixel_size_um
