"""Guide channel and depth map of the best-focus projection on the GPU (sq_focus_depth_plane, sq_fuse_select_depth,
Stitcher(focus_guide_channel=..., focus_depth_map=...)).  The oracle is never the code under test: a follower channel is
compared with np.take_along_axis of the fused stack (sq_fuse_planes / stitch_region, pinned by the fusion tests) along z by the
guide's depth (sq_fuse_project_focus / focus_region without a guide, pinned by test_focus_gpu.py).  Equality is exact."""
import os

import numpy as np
import pytest

from focus_guide_ref import select_by_depth
from helpers import flatfields_for
from image_stitcher_amd import native, omezarr, synth, stitcher_cli
from image_stitcher_amd.ometiff import read_ome_tiff
from image_stitcher_amd.stitcher import Stitcher
from image_stitcher_amd.stitcher_parameters import StitchingParameters

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _rects(rng, n, th, tw, ch, cw):
    out = []
    for _ in range(n):
        sy, sx = int(rng.integers(0, max(1, th // 3))), int(rng.integers(0, max(1, tw // 3)))
        h, w = int(rng.integers(1, th - sy + 1)), int(rng.integers(1, tw - sx + 1))
        out.append((sy, sx, h, w, int(rng.integers(0, ch)), int(rng.integers(0, cw))))
    return np.array(out, dtype=np.int64).reshape(-1, 6)


def _gains(rng, th, tw, dt):
    """Mostly ordinary gains, with subnormal, huge, zero, negative and tiny ones mixed in (as test_focus_gpu.py)."""
    g = rng.uniform(0.25, 4.0, (th, tw)).astype(dt)
    odd = rng.random((th, tw))
    g[odd < 0.02] = dt(np.finfo(dt).tiny / 8)
    g[(odd >= 0.02) & (odd < 0.04)] = dt(2.0 ** 110)
    g[(odd >= 0.04) & (odd < 0.06)] = 0
    g[(odd >= 0.06) & (odd < 0.09)] = -rng.uniform(0.5, 2.0, int(((odd >= 0.06) & (odd < 0.09)).sum()))
    g[(odd >= 0.09) & (odd < 0.10)] = dt(2.0 ** -105)
    return g


def _stack(plan, tiles, flats, ch, cw):
    """The fused stack of the planes ``tiles`` [Z, N, H, W] through sq_fuse_planes -> numpy [Z, Hc, Wc]."""
    import torch
    canvas = torch.full((tiles.shape[0], ch, cw), 9, dtype=tiles.dtype, device=DEV)
    native.fuse_planes(plan, tiles, canvas, flats)
    return canvas.cpu().numpy()


def _guide_depth(plan, tiles, zl, flats, ch, cw, radius=2):
    """The guide through sq_fuse_project_focus -> (signed depth as numpy, key tensor)."""
    import torch
    out = torch.empty((ch, cw), dtype=tiles.dtype, device=DEV)
    key = torch.empty((ch, cw), dtype=torch.int64, device=DEV)
    native.fuse_project_focus(plan, tiles, out, key, zl, radius, flats)
    return native.depth_of_keys(key).cpu().numpy(), key


@pytest.mark.parametrize('dtype', ['uint8', 'uint16'])
@pytest.mark.parametrize('gain', [None, 'float32', 'float64'])
def test_select_equals_the_stack_at_the_guides_depth(dtype, gain):
    import torch
    rng = np.random.default_rng(7 + len(dtype) + (0 if gain is None else len(gain)))
    th, tw, ch, cw = 67, 150, 173, 301
    nz, nc, n = 5, 3, 9
    top = 255 if dtype == 'uint8' else 65535
    tdt = native.torch_dtype_of(np.dtype(dtype))
    rects = _rects(rng, n, th, tw, ch, cw)
    plan = native.FusePlan(rects, th, tw, ch, cw)
    # the guide's rectangle list differs from the followers' (other tiles): voxels the guide does not cover, and voxels only it covers
    grects = _rects(rng, 7, th, tw, ch, cw)
    gplan = native.FusePlan(grects, th, tw, ch, cw)
    zl = list(range(nz))
    chan = [torch.from_numpy(rng.integers(0, top + 1, (nz, n, th, tw)).astype(dtype)).to(DEV) for _ in range(nc)]
    flats = [None] * nc
    if gain is not None:
        dt = np.dtype(gain).type
        # per channel: one shared gain image, one per plane, and a mix with None
        own = [[torch.from_numpy(_gains(rng, th, tw, dt)).to(DEV) for _ in range(nz)] for _ in range(nc)]
        flats = [[own[0][0]] * nz, own[1], [None if z % 2 else own[2][z] for z in range(nz)]]
    stacks = [_stack(plan, chan[c], flats[c], ch, cw) for c in range(nc)]
    for g in (0, 1, 2):      # the guide first, in the middle and last in the channel order
        gt = torch.from_numpy(rng.integers(0, top + 1, (nz, 7, th, tw)).astype(dtype)).to(DEV)
        depth, key = _guide_depth(gplan, gt, zl, None, ch, cw)
        assert (depth == -1).any() and len(np.unique(depth)) == nz + 1
        for ddt in (torch.uint8, torch.uint16):
            dplane = native.focus_depth_plane(key, dtype=native.np_dtype_of_torch(ddt))
            assert dplane.dtype == ddt
            np.testing.assert_array_equal(dplane.cpu().numpy(), depth + 1)
        dplane = native.focus_depth_plane(key)
        for c in range(nc):
            if c == g:
                continue
            want = select_by_depth(stacks[c], depth)
            assert want.any()
            for flags in (native.SQ_FUSE_FORCE_QUEUES, native.SQ_FUSE_FORCE_STATIC):
                for splits in ([(0, nz)], [(0, 2), (2, nz)], [(z, z + 1) for z in range(nz)],
                               [(z, z + 1) for z in reversed(range(nz))], [(3, nz), (0, 3)]):
                    out = torch.full((ch, cw), 3, dtype=tdt, device=DEV)      # poisoned: the first call writes every voxel
                    for i, (a, b) in enumerate(splits):
                        native.fuse_select_depth(plan, chan[c][a:b], out, dplane, zl[a:b],
                                                 None if flats[c] is None else flats[c][a:b], accumulate=i > 0, flags=flags)
                        if i == 0:
                            got = out.cpu().numpy()
                            inside = np.isin(depth, zl[a:b])
                            np.testing.assert_array_equal(got[inside], want[inside])
                            assert (got[~inside] == 0).all()
                    np.testing.assert_array_equal(out.cpu().numpy(), want)
        # padded row pitches of output and depth plane, a uint16 depth plane, tiles through a pointer table, z levels on the device
        c = (g + 1) % nc
        wide = torch.full((ch, cw + 45), 7, dtype=tdt, device=DEV)
        dwide = torch.full((ch, cw + 13), 99, dtype=torch.uint16, device=DEV)
        out, dpl = wide[:, 3:3 + cw], dwide[:, 5:5 + cw]
        native.focus_depth_plane(key, out=dpl)
        assert (dwide[:, :5] == 99).all() and (dwide[:, 5 + cw:] == 99).all()
        ptrs = native.pointer_table([chan[c][z, i] for z in range(nz) for i in range(n)], DEV)
        native.fuse_select_depth(plan, None, out, dpl, torch.tensor(zl, dtype=torch.int64, device=DEV), flats[c], tile_ptrs=ptrs)
        np.testing.assert_array_equal(out.cpu().numpy(), select_by_depth(stacks[c], depth))
        assert (wide[:, :3] == 7).all() and (wide[:, 3 + cw:] == 7).all()


def test_select_ragged_plans_sparse_levels_and_prior_contents():
    """A follower whose planes come under two rectangle lists (a tile missing in some planes), z levels far apart (the search
    behind the direct table) in a uint16 depth plane, and accumulate leaving the voxels of other depths untouched."""
    import torch
    rng = np.random.default_rng(41)
    th, tw, ch, cw = 90, 120, 211, 257
    zl = [0, 5, 900, 1023, 1024, 40000]
    nz = len(zl)
    rects = _rects(rng, 6, th, tw, ch, cw)
    plan_a, plan_b = native.FusePlan(rects, th, tw, ch, cw), native.FusePlan(rects[:4], th, tw, ch, cw)
    gains = torch.from_numpy(rng.uniform(0.5, 2.0, (th, tw)).astype(np.float32)).to(DEV)
    guide = torch.from_numpy(rng.integers(0, 65536, (nz, 6, th, tw)).astype(np.uint16)).to(DEV)
    depth, key = _guide_depth(plan_a, guide, zl, None, ch, cw)
    assert set(np.unique(depth)) == {-1, *zl}
    dplane = native.focus_depth_plane(key, dtype='uint16')
    np.testing.assert_array_equal(dplane.cpu().numpy(), depth + 1)
    assert (native.focus_depth_plane(key, dtype='uint8').cpu().numpy() == np.minimum(depth + 1, 255)).all()      # saturates
    ta = torch.from_numpy(rng.integers(0, 65536, (3, 6, th, tw)).astype(np.uint16)).to(DEV)       # levels 0, 900, 1024: all tiles
    tb = torch.from_numpy(rng.integers(0, 65536, (2, 4, th, tw)).astype(np.uint16)).to(DEV)       # levels 5, 40000: two tiles missing
    za, zb = [0, 900, 1024], [5, 40000]                                                           # (no plane at level 1023)
    sa, sb = _stack(plan_a, ta, [gains] * 3, ch, cw), _stack(plan_b, tb, [gains] * 2, ch, cw)
    want = np.zeros((ch, cw), dtype=np.uint16)
    for z, plane in list(zip(za, sa)) + list(zip(zb, sb)):
        want[depth == z] = plane[depth == z]
    assert (want[depth == 1023] == 0).all() and (depth == 1023).any()
    for flags in (native.SQ_FUSE_FORCE_QUEUES, native.SQ_FUSE_FORCE_STATIC):
        for order in ((0, 1), (1, 0)):
            out = torch.full((ch, cw), 3, dtype=torch.uint16, device=DEV)
            for i, which in enumerate(order):
                if which == 0:
                    native.fuse_select_depth(plan_a, ta, out, dplane, za, [gains] * 3, accumulate=i > 0, flags=flags)
                else:
                    native.fuse_select_depth(plan_b, tb, out, dplane, zb, [gains] * 2, accumulate=i > 0, flags=flags)
            np.testing.assert_array_equal(out.cpu().numpy(), want)
        # accumulate onto prior contents: only the voxels whose depth is one of the call's levels change
        prior = torch.from_numpy(rng.integers(1, 200, (ch, cw)).astype(np.uint16)).to(DEV)
        out = prior.clone()
        native.fuse_select_depth(plan_b, tb, out, dplane, zb, [gains] * 2, accumulate=True, flags=flags)
        mine = np.isin(depth, zb)
        got = out.cpu().numpy()
        np.testing.assert_array_equal(got[~mine], prior.cpu().numpy()[~mine])
        np.testing.assert_array_equal(got[mine], want[mine])


def test_rejections():
    import torch
    rects = np.array([[0, 0, 32, 32, 0, 0]])
    tiles = torch.zeros((2, 1, 32, 32), dtype=torch.uint16, device=DEV)
    out = torch.empty((40, 40), dtype=torch.uint16, device=DEV)
    depth = torch.zeros((40, 40), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match='overwrite'):
        native.fuse_select_depth(native.FusePlan(rects, 32, 32, 40, 40, native.SQ_FUSE_FEATHER), tiles, out, depth, [0, 1])
    plan = native.FusePlan(rects, 32, 32, 40, 40)
    with pytest.raises(ValueError, match='z levels'):
        native.fuse_select_depth(plan, tiles, out, depth, [0])
    with pytest.raises(ValueError, match='distinct'):
        native.fuse_select_depth(plan, tiles, out, depth, [1, 1])
    with pytest.raises(ValueError, match='uint8 or uint16'):
        native.fuse_select_depth(plan, tiles, out, depth.to(torch.int32), [0, 1])
    with pytest.raises(ValueError, match='planes'):
        native.fuse_select_depth(plan, torch.zeros((257, 1, 32, 32), dtype=torch.uint16, device=DEV), out, depth, list(range(257)))
    with pytest.raises(native.NativeError, match='dtype'):
        native.fuse_select_depth(plan, tiles, torch.empty((40, 40), dtype=torch.uint8, device=DEV), depth, [0, 1])
    with pytest.raises(ValueError, match='int64'):
        native.focus_depth_plane(depth)


# ---------------------------------------------------------------------------------------------- through Stitcher
def _prepared(root, spec, flat_dtype='float32', register=False, **kw):
    params = StitchingParameters(input_folder=root, use_registration=register, apply_flatfield=flat_dtype is not None,
                                 registration_channel=None, registration_z_level=0, scan_pattern=spec.scan_pattern)
    st = Stitcher(params, normalization=None, **kw)
    st.get_timepoints()
    st.extract_acquisition_parameters()
    st.get_pixel_size()
    st.parse_acquisition_metadata()
    if flat_dtype is not None:
        info = {'params': {'apply_flatfield': True, 'flat_dtype': flat_dtype},
                'spec': {'tile_h': spec.tile_h, 'tile_w': spec.tile_w}}
        st.flatfields = flatfields_for(info, st.num_c)
    if register:
        st.calculate_shifts(st.timepoints[0], st.regions[0])
    return st


def _want(root, spec, guide_name, flat_dtype='float32', register=False, radius=3):
    """(expected (1, C, 1, Hc, Wc), the guide's signed depth [Hc, Wc]) from a Stitcher WITHOUT a guide: its focus projection
    for the guide channel, its fused stack indexed by the guide's depth for the others."""
    plain = _prepared(root, spec, flat_dtype, register, z_projection='focus-only', focus_radius=radius)
    g = plain.monochrome_channels.index(guide_name)
    img, depth = plain.focus_region(0, 'R0', return_depth=True)
    stack = plain.stitch_region(0, 'R0')
    want = np.stack([img[0, c, 0] if c == g else select_by_depth(stack[0, c], depth[g]) for c in range(plain.num_c)])
    return want[None, :, None], depth[g], img


SPEC = dict(rows=2, cols=3, tile_h=96, tile_w=128, ov_y=17, ov_x=23, nz=4, channels=tuple(synth.DEFAULT_CHANNELS[:3]), seed=11)


@pytest.mark.parametrize('gi', [0, 1, 2])
def test_focus_region_with_a_guide_registered_and_flatfielded(tmp_path, gi):
    spec = synth.GridSpec(**dict(SPEC, rows=3, ov_y=36, ov_x=44))      # (a centre tile with a right and a lower neighbour)
    root = str(tmp_path / 'acq')
    synth.write_acquisition(spec, root)
    name = synth.DEFAULT_CHANNELS[gi]
    want, depth, plain = _want(root, spec, name, register=True)
    assert (want != plain).any()      # the followers do change
    st = _prepared(root, spec, register=True, z_projection='focus-only', focus_guide_channel=name)
    img, d = st.focus_region(0, 'R0', return_depth=True)
    np.testing.assert_array_equal(img, want)
    assert d.shape == (3,) + depth.shape and d.dtype == np.int32
    for c in range(3):
        np.testing.assert_array_equal(d[c], depth)
    # the guide's planes span several ingest chunks and share none with a follower; followers' chunks are a few planes each
    st.batch_bytes_limit = 3 * spec.n_tiles * spec.tile_h * spec.tile_w * 2
    np.testing.assert_array_equal(st.focus_region(0, 'R0'), want)
    st.batch_bytes_limit = 1
    np.testing.assert_array_equal(st.focus_region(0, 'R0', device_output=True).cpu().numpy(), want)


def test_row_band_equals_the_rows_of_the_whole_region(tmp_path):
    import torch
    spec = synth.GridSpec(**SPEC)
    root = str(tmp_path / 'acq')
    synth.write_acquisition(spec, root)
    st = _prepared(root, spec, z_projection='focus-only', focus_guide_channel=synth.DEFAULT_CHANNELS[1])
    whole = st.focus_region(0, 'R0')
    height = whole.shape[3]
    for y0, y1 in ((0, 64), (64, 150), (150, height)):
        out, key, depth, target = st._focus_target(0, 'R0', (y0, y1))
        st.stitch_planes(0, 'R0', None, row_band=(y0, y1), stack=False, project_to=target)
        np.testing.assert_array_equal(out.cpu().numpy(), whole[0, :, 0, y0:y1])
        # a follower alone, handed the band's depth plane
        out2, _, _, target2 = st._focus_target(0, 'R0', (y0, y1), [2], depth)
        st.stitch_planes(0, 'R0', [2 * st.num_z + z for z in range(st.num_z)], row_band=(y0, y1), stack=False, project_to=target2)
        np.testing.assert_array_equal(out2.cpu().numpy()[0], whole[0, 2, 0, y0:y1])


def test_ragged_acquisition(tmp_path):
    """Files missing in a follower (every level but one of a tile: some voxels' guide depth has no file there) and in the guide."""
    miss = tuple((1, z, 1, 0) for z in (0, 1, 3)) + ((4, 2, 0, 0), (2, 0, 1, 0))
    spec = synth.GridSpec(**dict(SPEC, channels=tuple(synth.DEFAULT_CHANNELS[:2]), missing=miss))
    root = str(tmp_path / 'acq')
    synth.write_acquisition(spec, root)
    want, depth, _ = _want(root, spec, synth.DEFAULT_CHANNELS[0])
    plain = _prepared(root, spec, z_projection='focus-only')
    stack = plain.stitch_region(0, 'R0')
    hole = (stack[0, 1, 0] == 0) & (stack[0, 1, 2] != 0)      # the follower's tile 1 region: no file at level 0
    assert (hole & (depth == 0)).any() and (want[0, 1, 0][hole & (depth == 0)] == 0).all()
    st = _prepared(root, spec, z_projection='focus-only', focus_guide_channel=synth.DEFAULT_CHANNELS[0])
    np.testing.assert_array_equal(st.focus_region(0, 'R0'), want)


def test_rgb_acquisition_with_the_green_component_as_guide(tmp_path):
    spec = synth.GridSpec(rows=2, cols=2, tile_h=80, tile_w=112, ov_y=15, ov_x=21, nz=3, dtype='uint8',
                          channels=(synth.DEFAULT_CHANNELS[1], 'BF LED matrix full'), rgb_channels=('BF LED matrix full',),
                          missing=((1, 2, 0, 0),), seed=5)
    root = str(tmp_path / 'acq')
    synth.write_acquisition(spec, root)
    plain = _prepared(root, spec, flat_dtype=None, z_projection='focus-only')
    name = [n for n in plain.monochrome_channels if n.endswith('_G')][0]
    want, depth, _ = _want(root, spec, name, flat_dtype=None)
    st = _prepared(root, spec, flat_dtype=None, z_projection='focus-only', focus_guide_channel=name)
    assert st.num_c == 4
    img, d = st.focus_region(0, 'R0', return_depth=True)
    np.testing.assert_array_equal(img, want)
    np.testing.assert_array_equal(d[0], depth)


# ---------------------------------------------------------------------------------------------- run() end to end
def _run(root, *extra):
    import random
    random.seed(1234)      # -ff samples the files it fits the flatfields to at random: the same sample in every run
    stitcher_cli.main(['-i', root, '--normalization', 'none', *extra])
    base = os.path.dirname(root)
    outs = [d for d in os.listdir(base) if d.startswith(os.path.basename(root) + '_stitched_')]
    assert len(outs) == 1
    return os.path.join(base, outs[0], '0_stitched')


def _tree(path):
    out = {}
    for d, _, files in os.walk(path):
        for f in files:
            with open(os.path.join(d, f), 'rb') as fh:
                out[os.path.relpath(os.path.join(d, f), path)] = fh.read()
    return out


def _levels(store):
    return [omezarr.read_array(os.path.join(store, str(lv))) for lv in sorted(int(d) for d in os.listdir(store) if d.isdigit())]


def test_run_writes_guided_edf_and_depth_stores(tmp_path):
    from oracle import stitch_oracle as O
    spec = synth.GridSpec(**dict(SPEC, rows=3, cols=3, tile_h=160, tile_w=192))
    name = synth.DEFAULT_CHANNELS[1]
    roots = {k: str(tmp_path / k / 'acq') for k in ('plain', 'guide', 'only', 'nog', 'gstack', 'tiff')}
    for r in roots.values():
        synth.write_acquisition(spec, r)
    common = ['-r', '-ff', '--focus-radius', '2']
    plain = _run(roots['plain'], *common, '--z-projection', 'focus')
    assert not any('depth' in f for f in os.listdir(plain))      # no flags: no new store
    stack = omezarr.read_array(os.path.join(plain, 'R0_stitched.ome.zarr', '0'))
    edf = omezarr.read_array(os.path.join(plain, 'R0_stitched_edf.ome.zarr', '0'))
    # 'focus' with a guide and the depth map, under the mean pyramid and percentile windows
    out = _run(roots['guide'], *common, '--z-projection', 'focus', '--focus-guide-channel', name, '--focus-depth-map',
               '--pyramid-method', 'mean', '--contrast-limits', 'percentile')
    dstore = os.path.join(out, 'R0_stitched_depth.ome.zarr')
    dlev = _levels(dstore)
    assert dlev[0].shape == (1, 1, 1) + stack.shape[3:] and dlev[0].dtype == np.uint8
    depth = dlev[0][0, 0, 0].astype(np.int64) - 1
    want = np.stack([edf[0, c, 0] if c == 1 else select_by_depth(stack[0, c], depth) for c in range(3)])[None, :, None]
    got = omezarr.read_array(os.path.join(out, 'R0_stitched_edf.ome.zarr', '0'))
    np.testing.assert_array_equal(got[0, 1], edf[0, 1])      # the guide: today's projection (which also pins the depth map:
    np.testing.assert_array_equal(got, want)                 # the guide's output is the stack at that depth)
    np.testing.assert_array_equal(select_by_depth(stack[0, 1], depth), edf[0, 1, 0])
    np.testing.assert_array_equal(omezarr.read_array(os.path.join(out, 'R0_stitched.ome.zarr', '0')), stack)
    import json
    with open(os.path.join(dstore, '.zattrs')) as fh:
        attrs = json.load(fh)
    assert [c['label'] for c in attrs['omero']['channels']] == [f'depth({name})']
    assert attrs['omero']['channels'][0]['window']['end'] == 4 and 'type' not in attrs['multiscales'][0]
    n_levels = len(_levels(os.path.join(out, 'R0_stitched_edf.ome.zarr')))
    assert len(dlev) == n_levels
    for a, b in zip(dlev, O.pyramid_nearest(dlev[0], n_levels)):
        np.testing.assert_array_equal(a, b)
    assert not any('depth_histogram' in f or 'depth_stats' in f for f in os.listdir(out))
    only = _run(roots['only'], *common, '--z-projection', 'focus-only', '--focus-guide-channel', name, '--focus-depth-map')
    assert not os.path.exists(os.path.join(only, 'R0_stitched.ome.zarr'))
    np.testing.assert_array_equal(omezarr.read_array(os.path.join(only, 'R0_stitched_edf.ome.zarr', '0')), want)
    np.testing.assert_array_equal(omezarr.read_array(os.path.join(only, 'R0_stitched_depth.ome.zarr', '0')), dlev[0])
    # the depth map without a guide: one plane per channel, each the depth of that channel's own projection
    nog = _run(roots['nog'], *common, '--z-projection', 'focus', '--focus-depth-map')
    d3 = omezarr.read_array(os.path.join(nog, 'R0_stitched_depth.ome.zarr', '0'))
    assert d3.shape == (1, 3, 1) + stack.shape[3:]
    np.testing.assert_array_equal(d3[0, 1], dlev[0][0, 0])
    for c in range(3):
        np.testing.assert_array_equal(select_by_depth(stack[0, c], d3[0, c, 0].astype(np.int64) - 1), edf[0, c, 0])
    # the stack and _edf stores of a run with the depth map / with a guide (nearest pyramid, as the plain run): the plain run's bytes
    assert _tree(os.path.join(nog, 'R0_stitched.ome.zarr')) == _tree(os.path.join(plain, 'R0_stitched.ome.zarr'))
    assert _tree(os.path.join(nog, 'R0_stitched_edf.ome.zarr')) == _tree(os.path.join(plain, 'R0_stitched_edf.ome.zarr'))
    gstack = _run(roots['gstack'], *common, '--z-projection', 'focus', '--focus-guide-channel', name)
    assert _tree(os.path.join(gstack, 'R0_stitched.ome.zarr')) == _tree(os.path.join(plain, 'R0_stitched.ome.zarr'))
    assert not any('depth' in f for f in os.listdir(gstack))
    # OME-TIFF
    tiff = _run(roots['tiff'], *common, '--z-projection', 'focus', '--focus-guide-channel', name, '--focus-depth-map',
                '-f', '.ome.tiff')
    planes, xml = read_ome_tiff(os.path.join(tiff, 'R0_stitched_edf.ome.tiff'))
    np.testing.assert_array_equal(np.stack(planes).reshape(want.shape), want)
    planes, xml = read_ome_tiff(os.path.join(tiff, 'R0_stitched_depth.ome.tiff'))
    assert len(planes) == 1 and f'depth({name})' in xml
    np.testing.assert_array_equal(planes[0], dlev[0][0, 0, 0])
