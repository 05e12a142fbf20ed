"""Maximum-intensity projection over z (sq_fuse_project_max, Stitcher.project_region, --z-projection) on the GPU, bit for bit
against max over z of the fused stack (native.fuse_planes, the oracle, the reference's golden canvases)."""
import os

import numpy as np
import pytest

from helpers import flatfields_for, load_case, spec_of
from image_stitcher_amd import native, omezarr, placement, synth
from image_stitcher_amd.ometiff import read_ome_tiff
from image_stitcher_amd.stitcher import Stitcher
from image_stitcher_amd.stitcher_parameters import StitchingParameters
from image_stitcher_amd import stitcher_cli

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _rects(rng, n, th, tw, ch, cw):
    """Random cropped rectangles, some reaching past the canvas' far edges (the planner clips them)."""
    out = []
    for _ in range(n):
        sy, sx = int(rng.integers(0, th // 3)), int(rng.integers(0, tw // 3))
        h, w = int(rng.integers(1, th - sy + 1)), int(rng.integers(1, tw - sx + 1))
        out.append((sy, sx, h, w, int(rng.integers(0, ch)), int(rng.integers(0, cw))))
    return np.array(out, dtype=np.int64).reshape(-1, 6)


def _gains(rng, th, tw, dt):
    """Mostly ordinary gains, with subnormal, huge, zero, negative and tiny ones mixed in."""
    g = rng.uniform(0.25, 4.0, (th, tw)).astype(dt)
    odd = rng.random((th, tw))
    tiny = np.finfo(dt).tiny
    g[odd < 0.02] = dt(tiny / 8)                  # subnormal
    g[(odd >= 0.02) & (odd < 0.04)] = dt(2.0 ** 110)
    g[(odd >= 0.04) & (odd < 0.06)] = 0
    g[(odd >= 0.06) & (odd < 0.09)] = -rng.uniform(0.5, 2.0, int(((odd >= 0.06) & (odd < 0.09)).sum()))
    g[(odd >= 0.09) & (odd < 0.10)] = dt(2.0 ** -105)
    return g


def amax_z(stack):
    """Unsigned maximum over the first axis (torch has no uint16 max reduction on the device: flip the sign bit, reduce as int16)."""
    import torch
    if stack.dtype != torch.uint16:
        return stack.amax(0)
    flip = stack.view(torch.int16) ^ -32768
    return (flip.amax(0) ^ -32768).view(torch.uint16)


def _stack_max(plan, tiles, flats, ch, cw):
    import torch
    stack = torch.empty((tiles.shape[0], ch, cw), dtype=tiles.dtype, device=DEV)
    native.fuse_planes(plan, tiles, stack, flats)
    return stack, amax_z(stack)


@pytest.mark.parametrize('nz', [1, 2, 5, 8, 13])
@pytest.mark.parametrize('dtype', ['uint8', 'uint16'])
@pytest.mark.parametrize('gain', [None, 'float32', 'float64'])
def test_projection_equals_max_of_the_fused_stack(nz, dtype, gain):
    import torch
    rng = np.random.default_rng(1000 * nz + len(dtype) + (0 if gain is None else len(gain)))
    th, tw, ch, cw = 67, 150, 173, 301
    tdt = native.torch_dtype_of(np.dtype(dtype))
    top = 255 if dtype == 'uint8' else 65535
    for n_rects in (0, 9):
        rects = _rects(rng, n_rects, th, tw, ch, cw)
        plan = native.FusePlan(rects, th, tw, ch, cw)
        tiles = torch.from_numpy(rng.integers(0, top + 1, (nz, n_rects, th, tw), dtype=np.int64).astype(dtype)).to(DEV)
        if gain is None:
            cases = [('none', None)]
        else:
            dt = np.dtype(gain).type
            shared = torch.from_numpy(_gains(rng, th, tw, dt)).to(DEV)
            own = [torch.from_numpy(_gains(rng, th, tw, dt)).to(DEV) for _ in range(nz)]
            cases = [('shared', [shared] * nz), ('per-plane', own), ('with-none', [None if z % 2 else own[z] for z in range(nz)])]
        for label, flats in cases:
            stack, want = _stack_max(plan, tiles, flats, ch, cw)
            if n_rects and label != 'none':      # the oracle, plane by plane, on the host
                tl = tiles.cpu().numpy()
                ref = np.zeros((ch, cw), dtype=dtype)
                for z in range(nz):
                    ff = None if flats[z] is None else flats[z].cpu().numpy()
                    ref = np.maximum(ref, _oracle_plane(list(tl[z]), rects, ch, cw, ff))
                np.testing.assert_array_equal(want.cpu().numpy(), ref)
            for flags in (0, native.SQ_FUSE_FORCE_QUEUES, native.SQ_FUSE_FORCE_STATIC):
                out = torch.full((ch, cw), top, dtype=tdt, device=DEV)     # poisoned: every voxel must be written
                native.fuse_project_max(plan, tiles, out, flats, flags=flags)
                assert torch.equal(out, want), (label, flags, n_rects)
            # padded row pitch, tiles through a pointer table
            wide = torch.full((ch, cw + 45), 7, dtype=tdt, device=DEV)
            out = wide[:, 3:3 + cw]
            ptrs = native.pointer_table([tiles[z, i] for z in range(nz) for i in range(n_rects)], DEV) if n_rects else None
            if ptrs is not None:
                native.fuse_project_max(plan, None, out, flats, tile_ptrs=ptrs)
            else:
                native.fuse_project_max(plan, tiles, out, flats)
            assert torch.equal(out, want), (label, 'padded')
            assert (wide[:, :3] == 7).all() and (wide[:, 3 + cw:] == 7).all()


def _oracle_plane(tiles, rects, ch, cw, ff):
    from oracle import stitch_oracle as O
    return O.fuse_plane_overwrite(tiles, rects, ch, cw, ff)


@pytest.mark.parametrize('dtype', ['uint8', 'uint16'])
def test_accumulate_over_two_plans(dtype):
    """A channel whose z planes come under two different plans: write with the first, accumulate with the second -> the max
    of both fused stacks.  Accumulating leaves the voxels the plan does not cover untouched."""
    import torch
    rng = np.random.default_rng(7)
    th, tw, ch, cw = 90, 120, 211, 257
    tdt = native.torch_dtype_of(np.dtype(dtype))
    top = 255 if dtype == 'uint8' else 65535
    gains = torch.from_numpy(_gains(rng, th, tw, np.float32)).to(DEV)
    plans, stacks, tiles_of = [], [], []
    for n, nz in ((6, 3), (4, 2)):
        rects = _rects(rng, n, th, tw, ch, cw)
        plans.append(native.FusePlan(rects, th, tw, ch, cw))
        tiles_of.append(torch.from_numpy(rng.integers(0, top + 1, (nz, n, th, tw)).astype(dtype)).to(DEV))
        stacks.append(_stack_max(plans[-1], tiles_of[-1], [gains] * nz, ch, cw)[1])
    out = torch.ones((ch, cw), dtype=tdt, device=DEV)
    native.fuse_project_max(plans[0], tiles_of[0], out, [gains] * 3)
    native.fuse_project_max(plans[1], tiles_of[1], out, [gains] * 2, accumulate=True)
    assert torch.equal(out, amax_z(torch.stack(stacks)))
    # on prior contents: covered voxels max(prior, projection), the others unchanged
    ones = torch.ones((1, len(plans[1].rects), th, tw), dtype=tdt, device=DEV)
    covered = torch.empty((1, ch, cw), dtype=tdt, device=DEV)
    native.fuse_planes(plans[1], ones, covered)
    covered = covered[0] == 1
    assert 0 < int(covered.sum()) < ch * cw
    prior = torch.from_numpy(rng.integers(0, top + 1, (ch, cw)).astype(dtype)).to(DEV)
    for flags in (native.SQ_FUSE_FORCE_QUEUES, native.SQ_FUSE_FORCE_STATIC):
        out = prior.clone()
        native.fuse_project_max(plans[1], tiles_of[1], out, [gains] * 2, accumulate=True, flags=flags)
        # (torch cannot index uint16 tensors on the device: compare the bits through a signed view of the same width)
        bits = (lambda t: t.view(torch.int16)) if dtype == 'uint16' else (lambda t: t)
        assert torch.equal(bits(out)[~covered], bits(prior)[~covered])
        assert torch.equal(bits(out)[covered], bits(amax_z(torch.stack([prior, stacks[1]])))[covered])


def test_rejects_feather_plans_and_bad_outputs():
    import torch
    rects = np.array([[0, 0, 32, 32, 0, 0]])
    tiles = torch.zeros((2, 1, 32, 32), dtype=torch.uint16, device=DEV)
    feather = native.FusePlan(rects, 32, 32, 40, 40, native.SQ_FUSE_FEATHER)
    with pytest.raises(ValueError, match='overwrite'):
        native.fuse_project_max(feather, tiles, torch.empty((40, 40), dtype=torch.uint16, device=DEV))
    plan = native.FusePlan(rects, 32, 32, 40, 40)
    with pytest.raises(ValueError):
        native.fuse_project_max(plan, tiles, torch.empty((2, 40, 40), dtype=torch.uint16, device=DEV))
    with pytest.raises(native.NativeError, match='dtype'):
        native.fuse_project_max(plan, tiles, torch.empty((40, 40), dtype=torch.uint8, device=DEV))


def _prepared(info, root, **kw):
    p = info['params']
    params = StitchingParameters(input_folder=root, use_registration=p['use_registration'],
                                 apply_flatfield=p['apply_flatfield'],
                                 registration_channel=p['registration_channel'],
                                 registration_z_level=p['registration_z_level'],
                                 scan_pattern=info['spec']['scan_pattern'])
    st = Stitcher(params, normalization=None, **kw)
    st.get_timepoints()
    st.extract_acquisition_parameters()
    st.get_pixel_size()
    st.parse_acquisition_metadata()
    flats = flatfields_for(info, st.num_c)
    if flats:
        st.flatfields = flats
    if p['use_registration']:
        st.calculate_shifts(st.timepoints[0], st.regions[0])
    return st


@pytest.mark.parametrize('name', ['coord_1x3', 'coord_3x4_small', 'coord_jitter', 'reg_3x4_small', 'reg_ragged'])
def test_project_region_matches_the_golden_stack(name, tmp_path):
    info, arrays = load_case(name)
    assert info['num_z'] == 2
    root = str(tmp_path / 'acq')
    synth.write_acquisition(spec_of(info), root)
    st = _prepared(info, root)
    for key in info['canvases']:
        t, region = key[1:].split('_', 1)
        mip = st.project_region(int(t), region)
        stack = arrays[f'{key}_canvas'] if f'{key}_canvas' in arrays else st.stitch_region(int(t), region)
        assert mip.shape == stack.shape[:2] + (1,) + stack.shape[3:]
        np.testing.assert_array_equal(mip, stack.max(axis=2, keepdims=True))


def test_project_region_matches_the_oracle_with_flatfields(tmp_path):
    """nz = 5, two channels, -ff (float32 gains per channel): the oracle's stack, max over z."""
    from oracle import stitch_oracle as O
    from image_stitcher_amd.tiffio import read_image
    spec = synth.GridSpec(rows=2, cols=3, tile_h=96, tile_w=128, ov_y=17, ov_x=23, nz=5,
                          channels=tuple(synth.DEFAULT_CHANNELS[:2]), seed=11)
    root = str(tmp_path / 'acq')
    synth.write_acquisition(spec, root)
    info = {'params': {'use_registration': False, 'apply_flatfield': True, 'registration_channel': None,
                       'registration_z_level': 0, 'flat_dtype': 'float32'},
            'spec': {'scan_pattern': 'Unidirectional', 'tile_h': spec.tile_h, 'tile_w': spec.tile_w}}
    st = _prepared(info, root)
    assert st.num_z == 5 and st.num_c == 2
    mip = st.project_region(0, 'R0')
    acq = O.parse_acquisition(root, read_image)
    ref = O.stitch_region(acq, 0, 'R0', read_image, False, None, st.flatfields, apply_flat=True)
    np.testing.assert_array_equal(mip, ref.max(axis=2, keepdims=True))
    np.testing.assert_array_equal(st.project_region(0, 'R0', device_output=True).cpu().numpy(), mip)


def _run(root, *extra):
    stitcher_cli.main(['-i', root, '-r', '--normalization', 'none', *extra])
    base = os.path.dirname(root)
    outs = [d for d in os.listdir(base) if d.startswith(os.path.basename(root) + '_stitched_')]
    assert len(outs) == 1
    return os.path.join(base, outs[0], '0_stitched')


def _files(path):
    out = {}
    for d, _, fs in os.walk(path):
        for f in fs:
            with open(os.path.join(d, f), 'rb') as fh:
                out[os.path.relpath(os.path.join(d, f), path)] = fh.read()
    return out


def test_run_writes_the_projection_store(tmp_path):
    from oracle import stitch_oracle as O
    info, arrays = load_case('reg_3x4_small')
    spec = spec_of(info)
    ch = ['--registration-channel', info['params']['registration_channel'], '--registration-z-level', '1']
    roots = {k: str(tmp_path / k / 'acq') for k in ('plain', 'max', 'only', 'tiff')}
    for r in roots.values():
        synth.write_acquisition(spec, r)
    plain = _run(roots['plain'], *ch)
    with_mip = _run(roots['max'], *ch, '--z-projection', 'max')
    assert _files(os.path.join(plain, 'R0_stitched.ome.zarr')) == _files(os.path.join(with_mip, 'R0_stitched.ome.zarr'))
    want = arrays['t0_R0_canvas'].max(axis=2, keepdims=True)
    mip_store = os.path.join(with_mip, 'R0_stitched_mip.ome.zarr')
    level0 = omezarr.read_array(os.path.join(mip_store, '0'))
    np.testing.assert_array_equal(level0, want)
    levels = O.pyramid_nearest(level0, info['canvases']['t0_R0'].get('num_pyramid_levels', 1))
    for lv in range(1, len(levels)):
        np.testing.assert_array_equal(omezarr.read_array(os.path.join(mip_store, str(lv))), levels[lv])
    only = _run(roots['only'], *ch, '--z-projection', 'max-only')
    assert not os.path.exists(os.path.join(only, 'R0_stitched.ome.zarr'))
    np.testing.assert_array_equal(omezarr.read_array(os.path.join(only, 'R0_stitched_mip.ome.zarr', '0')), want)
    tiff = _run(roots['tiff'], *ch, '--z-projection', 'max', '-f', '.ome.tiff')
    planes, xml = read_ome_tiff(os.path.join(tiff, 'R0_stitched_mip.ome.tiff'))
    assert len(planes) == want.shape[1] and 'SizeZ="1"' in xml
    np.testing.assert_array_equal(np.stack(planes).reshape(want.shape), want)
    assert os.path.exists(os.path.join(tiff, 'R0_stitched.ome.tiff'))


def test_run_projection_pyramid_on_a_tall_canvas(tmp_path):
    """3 pyramid levels: level 0 equals max over z of the reference's canvas, the other levels the oracle's pyramid of it."""
    from oracle import stitch_oracle as O
    info, arrays = load_case('reg_2x2_2048')
    root = str(tmp_path / 'acq')
    synth.write_acquisition(spec_of(info), root)
    out = _run(root, '--zarr-compression', 'none', '--z-projection', 'max-only')
    store = os.path.join(out, 'R0_stitched_mip.ome.zarr')
    level0 = omezarr.read_array(os.path.join(store, '0'))
    cinfo = info['canvases']['t0_R0']
    assert list(level0.shape) == cinfo['shape'][:2] + [1] + cinfo['shape'][3:]
    if 't0_R0_canvas' in arrays:
        np.testing.assert_array_equal(level0, arrays['t0_R0_canvas'].max(axis=2, keepdims=True))
    levels = O.pyramid_nearest(level0, cinfo['num_pyramid_levels'])
    assert len(levels) == 3
    for lv in range(1, 3):
        np.testing.assert_array_equal(omezarr.read_array(os.path.join(store, str(lv))), levels[lv])


def test_config3_channel_full_size():
    """One config-3-shaped channel on the device: 16 x 16 tiles of 2048^2, 10 z, float32 gains -> 0 voxels differ from amax of
    sq_fuse_planes' 10 planes."""
    import torch
    g, T, Z = 16, 2048, 10
    shifts = placement.Shifts((3, -244), (-244, -2))
    rects = placement.grid_rects(g, g, T, T, shifts, crop=True)
    wc, hc = placement.canvas_size(g, g, T, T, use_registration=True, shifts=shifts)
    plan = native.FusePlan(rects, T, T, hc, wc, expand_on_device=True)
    spec = synth.GridSpec(rows=g, cols=g, tile_h=T, tile_w=T, ov_y=244, ov_x=244, seed=1)
    tiles = torch.empty((Z, g * g, T, T), dtype=torch.uint16, device=DEV)
    for z in range(Z):
        desc = np.zeros(g * g, dtype=native.SYNTH_DTYPE)
        for r in range(g):
            for c in range(g):
                oy, ox = spec.origin(r, c)
                desc[r * g + c] = (spec.scene_seed(0, 0, z, 0) % 2**64, spec.noise_seed(0, 0, z, 0, r * g + c) % 2**64, oy, ox)
        native.synth_tiles(desc, T, T, spec.noise, 'uint16', DEV, out=tiles[z])
    gain = torch.from_numpy(synth.synthetic_flatfield(T, T, np.float32)).to(DEV)
    flats = [gain] * Z
    stack = native.empty_canvas(Z, hc, wc, torch.uint16, DEV)
    native.fuse_planes(plan, tiles, stack, flats)
    want = amax_z(stack)
    del stack
    out = torch.empty((hc, wc), dtype=torch.uint16, device=DEV)
    native.fuse_project_max(plan, tiles, out, flats)
    assert int((out != want).sum()) == 0
