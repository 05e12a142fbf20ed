"""Best-focus (extended depth of field) projection over z (sq_fuse_project_focus, Stitcher.focus_region, --z-projection focus)
on the GPU: output and key plane bit for bit against the numpy definition (focus_ref.py), a synthetic defocus stack with a
known best plane, and the stores of a whole run."""
import os

import numpy as np
import pytest

from focus_ref import depth_of, focus_reference, focus_reference_region
from helpers import flatfields_for
from image_stitcher_amd import native, omezarr, synth
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
        sy, sx = int(rng.integers(0, max(1, th // 3))), int(rng.integers(0, max(1, tw // 3)))
        h, w = int(rng.integers(1, th - sy + 1)), int(rng.integers(1, tw - sx + 1))
        out.append((sy, sx, h, w, int(rng.integers(0, ch)), int(rng.integers(0, cw))))
    return np.array(out, dtype=np.int64).reshape(-1, 6)


def _gains(rng, th, tw, dt):
    """Mostly ordinary gains, with subnormal, huge, zero, negative and tiny ones mixed in (as test_projection_gpu.py)."""
    g = rng.uniform(0.25, 4.0, (th, tw)).astype(dt)
    odd = rng.random((th, tw))
    tiny = np.finfo(dt).tiny
    g[odd < 0.02] = dt(tiny / 8)
    g[(odd >= 0.02) & (odd < 0.04)] = dt(2.0 ** 110)
    g[(odd >= 0.04) & (odd < 0.06)] = 0
    g[(odd >= 0.06) & (odd < 0.09)] = -rng.uniform(0.5, 2.0, int(((odd >= 0.06) & (odd < 0.09)).sum()))
    g[(odd >= 0.09) & (odd < 0.10)] = dt(2.0 ** -105)
    return g


def _tiles(rng, nz, n, th, tw, dtype):
    """Random planes, plane 1 a copy of plane 0 (every score ties: the lower z level must win) and the last plane flat."""
    top = 255 if dtype == 'uint8' else 65535
    t = rng.integers(0, top + 1, (nz, n, th, tw)).astype(dtype)
    if nz >= 2:
        t[1] = t[0]
    if nz >= 3:
        t[-1] = top // 3
    return t


def _host(t):
    return None if t is None else t.cpu().numpy()


def _check(out, key, want):
    import torch
    ref_out, ref_key = want
    np.testing.assert_array_equal(out.cpu().numpy(), ref_out)
    np.testing.assert_array_equal(key.cpu().numpy().view(np.uint64), ref_key)
    assert key.dtype == torch.int64


CASES = [(1, 0), (1, 3), (2, 1), (2, 3), (5, 0), (5, 3), (5, 15), (13, 1), (13, 3), (13, 15)]


@pytest.mark.parametrize('nz,radius', CASES)
@pytest.mark.parametrize('dtype', ['uint8', 'uint16'])
@pytest.mark.parametrize('gain', [None, 'float32', 'float64'])
def test_focus_equals_the_definition(nz, radius, dtype, gain):
    import torch
    rng = np.random.default_rng(100 * nz + radius + len(dtype) + (0 if gain is None else len(gain)))
    th, tw, ch, cw = 67, 150, 173, 301       # neither a multiple of the 64 x 32 block
    tdt = native.torch_dtype_of(np.dtype(dtype))
    zl = [int(z) for z in rng.choice(1000, nz, replace=False)]
    for n_rects in (0, 9):
        rects = _rects(rng, n_rects, th, tw, ch, cw)
        plan = native.FusePlan(rects, th, tw, ch, cw)
        tl = _tiles(rng, nz, n_rects, th, tw, dtype)
        tiles = torch.from_numpy(tl).to(DEV)
        if gain is None:
            cases = [('none', None)]
        else:
            dt = np.dtype(gain).type
            shared = torch.from_numpy(_gains(rng, th, tw, dt)).to(DEV)
            own = [torch.from_numpy(_gains(rng, th, tw, dt)).to(DEV) for _ in range(nz)]
            cases = [('shared', [shared] * nz), ('per-plane', own), ('with-none', [None if z % 2 else own[z] for z in range(nz)])]
        for label, flats in cases:
            want = focus_reference([(tl, rects, None if flats is None else [_host(f) for f in flats], zl)], ch, cw, radius)
            if n_rects:
                assert (want[1] > 0).any()
            for flags in (0, native.SQ_FUSE_FORCE_QUEUES, native.SQ_FUSE_FORCE_STATIC):
                out = torch.full((ch, cw), 3, dtype=tdt, device=DEV)     # poisoned: every voxel must be written
                key = torch.full((ch, cw), -7, dtype=torch.int64, device=DEV)
                native.fuse_project_focus(plan, tiles, out, key, zl, radius, flats, flags=flags)
                _check(out, key, want)
            # padded row pitch of both outputs, tiles through a pointer table, z levels already on the device
            wide = torch.full((ch, cw + 45), 7, dtype=tdt, device=DEV)
            kwide = torch.full((ch, cw + 13), 9, dtype=torch.int64, device=DEV)
            out, key = wide[:, 3:3 + cw], kwide[:, 5:5 + cw]
            zdev = torch.tensor(zl, dtype=torch.int64, device=DEV)
            if n_rects:
                ptrs = native.pointer_table([tiles[z, i] for z in range(nz) for i in range(n_rects)], DEV)
                native.fuse_project_focus(plan, None, out, key, zdev, radius, flats, tile_ptrs=ptrs)
            else:
                native.fuse_project_focus(plan, tiles, out, key, zdev, radius, flats)
            _check(out, key, want)
            assert (wide[:, :3] == 7).all() and (wide[:, 3 + cw:] == 7).all()
            assert (kwide[:, :5] == 9).all() and (kwide[:, 5 + cw:] == 9).all()


@pytest.mark.parametrize('th,tw', [(1, 1), (1, 5), (3, 2), (5, 1), (31, 65), (33, 64), (64, 33)])
@pytest.mark.parametrize('radius', [0, 3, 15])
def test_small_and_odd_tiles(th, tw, radius):
    """Tiles narrower than the window (2R + 1 up to 31) and block edges off by one."""
    import torch
    rng = np.random.default_rng(th * 1000 + tw * 10 + radius)
    nz, n = 4, 6
    ch, cw = 3 * th + 2, 3 * tw + 2
    rects = _rects(rng, n, th, tw, ch, cw)
    plan = native.FusePlan(rects, th, tw, ch, cw)
    tl = _tiles(rng, nz, n, th, tw, 'uint16')
    zl = [3, 0, 2, 1]
    want = focus_reference([(tl, rects, None, zl)], ch, cw, radius)
    for flags in (native.SQ_FUSE_FORCE_QUEUES, native.SQ_FUSE_FORCE_STATIC):
        out = torch.full((ch, cw), 5, dtype=torch.uint16, device=DEV)
        key = torch.full((ch, cw), -1, dtype=torch.int64, device=DEV)
        native.fuse_project_focus(plan, torch.from_numpy(tl).to(DEV), out, key, zl, radius, flags=flags)
        _check(out, key, want)


@pytest.mark.parametrize('dtype', ['uint8', 'uint16'])
def test_accumulate_over_calls_orders_and_plans(dtype):
    """A channel's planes split over several calls -- ascending z, descending z, and under two plans (ragged input) -- give
    what one call gives; accumulating onto prior contents leaves the voxels the plan does not cover untouched."""
    import torch
    rng = np.random.default_rng(17)
    th, tw, ch, cw = 90, 120, 211, 257
    tdt = native.torch_dtype_of(np.dtype(dtype))
    gains = rng.uniform(0.5, 2.0, (th, tw)).astype(np.float32)
    gdev = torch.from_numpy(gains).to(DEV)
    nz = 7
    rects = _rects(rng, 6, th, tw, ch, cw)
    plan = native.FusePlan(rects, th, tw, ch, cw)
    tl = _tiles(rng, nz, 6, th, tw, dtype)
    tiles = torch.from_numpy(tl).to(DEV)
    zl = list(range(nz))
    one_out = torch.empty((ch, cw), dtype=tdt, device=DEV)
    one_key = torch.empty((ch, cw), dtype=torch.int64, device=DEV)
    native.fuse_project_focus(plan, tiles, one_out, one_key, zl, 3, [gdev] * nz)
    _check(one_out, one_key, focus_reference([(tl, rects, [gains] * nz, zl)], ch, cw, 3))
    scratch = torch.empty(native.focus_scratch_bytes(6, th, tw), dtype=torch.uint8, device=DEV)
    for splits in ([(0, 3), (3, 5), (5, 7)], [(5, 7), (3, 5), (0, 3)], [(6, 7), (0, 1), (2, 6), (1, 2)]):
        out = torch.empty((ch, cw), dtype=tdt, device=DEV)
        key = torch.empty((ch, cw), dtype=torch.int64, device=DEV)
        for i, (a, b) in enumerate(splits):
            native.fuse_project_focus(plan, tiles[a:b], out, key, zl[a:b], 3, [gdev] * (b - a), scratch=scratch,
                                      accumulate=i > 0)
        assert torch.equal(out, one_out) and torch.equal(key, one_key), splits
    # two plans: planes 0..3 under the first, 4..6 under a second rectangle list of other tiles
    rects2 = _rects(rng, 4, th, tw, ch, cw)
    plan2 = native.FusePlan(rects2, th, tw, ch, cw)
    tl2 = _tiles(rng, 3, 4, th, tw, dtype)
    want = focus_reference([(tl[:4], rects, [gains] * 4, zl[:4]), (tl2, rects2, [gains] * 3, [4, 5, 6])], ch, cw, 3)
    for order in ((0, 1), (1, 0)):
        out = torch.empty((ch, cw), dtype=tdt, device=DEV)
        key = torch.empty((ch, cw), dtype=torch.int64, device=DEV)
        for i, which in enumerate(order):
            if which == 0:
                native.fuse_project_focus(plan, tiles[:4], out, key, zl[:4], 3, [gdev] * 4, accumulate=i > 0)
            else:
                native.fuse_project_focus(plan2, torch.from_numpy(tl2).to(DEV), out, key, [4, 5, 6], 3, [gdev] * 3,
                                          accumulate=i > 0)
        _check(out, key, want)
    # prior contents: key 0 everywhere -> covered voxels take the projection, the others keep their value
    prior = torch.from_numpy(rng.integers(0, 200, (ch, cw)).astype(dtype)).to(DEV)
    for flags in (native.SQ_FUSE_FORCE_QUEUES, native.SQ_FUSE_FORCE_STATIC):
        out, key = prior.clone(), torch.zeros((ch, cw), dtype=torch.int64, device=DEV)
        native.fuse_project_focus(plan, tiles, out, key, zl, 3, [gdev] * nz, accumulate=True, flags=flags)
        covered = (one_key != 0).cpu().numpy()
        assert 0 < covered.sum() < ch * cw
        np.testing.assert_array_equal(out.cpu().numpy()[~covered], prior.cpu().numpy()[~covered])
        np.testing.assert_array_equal(out.cpu().numpy()[covered], one_out.cpu().numpy()[covered])


def test_rejections():
    import torch
    rects = np.array([[0, 0, 32, 32, 0, 0]])
    tiles = torch.zeros((2, 1, 32, 32), dtype=torch.uint16, device=DEV)
    out = torch.empty((40, 40), dtype=torch.uint16, device=DEV)
    key = torch.empty((40, 40), dtype=torch.int64, device=DEV)
    feather = native.FusePlan(rects, 32, 32, 40, 40, native.SQ_FUSE_FEATHER)
    with pytest.raises(ValueError, match='overwrite'):
        native.fuse_project_focus(feather, tiles, out, key, [0, 1])
    plan = native.FusePlan(rects, 32, 32, 40, 40)
    for r in (-1, 16):
        with pytest.raises(ValueError, match='radius'):
            native.fuse_project_focus(plan, tiles, out, key, [0, 1], r)
    with pytest.raises(ValueError, match='z levels'):
        native.fuse_project_focus(plan, tiles, out, key, [0])
    with pytest.raises(ValueError, match='scratch'):
        native.fuse_project_focus(plan, tiles, out, key, [0, 1], scratch=torch.empty(100, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match='int64'):
        native.fuse_project_focus(plan, tiles, out, key.to(torch.float64), [0, 1])
    with pytest.raises(ValueError, match='planes'):
        native.fuse_project_focus(plan, torch.zeros((257, 1, 32, 32), dtype=torch.uint16, device=DEV), out, key,
                                  list(range(257)))
    with pytest.raises(native.NativeError, match='dtype'):
        native.fuse_project_focus(plan, tiles, torch.empty((40, 40), dtype=torch.uint8, device=DEV), key, [0, 1])


def _box_blur(img, k):
    """Mean over a (2k+1)^2 window, edges clamped, rounded down (integer)."""
    if k == 0:
        return img.copy()
    p = np.pad(img.astype(np.int64), k, mode='edge')
    c = np.zeros((p.shape[0] + 1, p.shape[1] + 1), dtype=np.int64)
    c[1:, 1:] = p.cumsum(0).cumsum(1)
    n = 2 * k + 1
    s = c[n:, n:] - c[:-n, n:] - c[n:, :-n] + c[:-n, :-n]
    return (s // (n * n)).astype(img.dtype)


@pytest.mark.parametrize('radius', [1, 3])
def test_defocus_stack_ground_truth(radius):
    """A sharp texture in focus at a known z* per 48 x 48 patch, box-blurred more the farther z is from z*: the depth equals
    z* on >= 99 % of the voxels farther than R + 2 px from a patch boundary (and the output is the in-focus texture there)."""
    import torch
    rng = np.random.default_rng(23 + radius)
    P, gy, gx, nz = 48, 4, 5, 6
    th, tw = P * gy, P * gx
    zstar = rng.integers(0, nz, (gy, gx))
    tiles = np.empty((nz, 2, th, tw), dtype=np.uint16)
    truth = np.repeat(np.repeat(zstar, P, 0), P, 1)
    for k in range(2):
        tex = rng.integers(500, 4000, (th, tw)).astype(np.uint16)
        blurred = [_box_blur(tex, b) for b in range(nz)]
        for z in range(nz):
            dist = np.abs(z - truth)
            tiles[z, k] = np.choose(dist, blurred)
    # two tiles side by side with a cropped overlap
    rects = np.array([[0, 0, th, tw - 10, 0, 0], [0, 10, th, tw - 10, 0, tw - 10]])
    ch, cw = th, 2 * tw - 20
    plan = native.FusePlan(rects, th, tw, ch, cw)
    out = torch.empty((ch, cw), dtype=torch.uint16, device=DEV)
    key = torch.empty((ch, cw), dtype=torch.int64, device=DEV)
    native.fuse_project_focus(plan, torch.from_numpy(tiles).to(DEV), out, key, list(range(nz)), radius)
    depth = depth_of(key.cpu().numpy().view(np.uint64))
    np.testing.assert_array_equal(depth, native.depth_of_keys(key).cpu().numpy())
    # canvas voxel -> (tile, tile column); patch boundaries in tile coordinates
    yy, xx = np.mgrid[0:ch, 0:cw]
    tx = np.where(xx < tw - 10, xx, xx - (tw - 10) + 10)
    want = truth[yy, tx]
    m = radius + 2
    far = ((yy % P) >= m) & ((yy % P) < P - m) & ((tx % P) >= m) & ((tx % P) < P - m)
    right = (depth == want)[far].mean()
    assert right >= 0.99, right
    ok = far & (xx < tw - 10) & (depth == want)      # the first tile's voxels: the output is its in-focus plane
    got = out.cpu().numpy()
    for z in range(nz):
        sel = ok & (want == z)
        np.testing.assert_array_equal(got[sel], tiles[z, 0][yy[sel], tx[sel]])


def _prepared(root, spec, flat_dtype='float32', **kw):
    params = StitchingParameters(input_folder=root, use_registration=False, apply_flatfield=flat_dtype is not None,
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
    return st


def _oracle(root, st, radius):
    from oracle import stitch_oracle as O
    from image_stitcher_amd.tiffio import read_image
    acq = O.parse_acquisition(root, read_image)
    return focus_reference_region(acq, 0, 'R0', read_image, radius, st.flatfields if st.apply_flatfield else None,
                                  apply_flat=st.apply_flatfield)


SPEC = dict(rows=2, cols=3, tile_h=96, tile_w=128, ov_y=17, ov_x=23, nz=4, channels=tuple(synth.DEFAULT_CHANNELS[:2]), seed=11)


@pytest.mark.parametrize('radius', [0, 3])
def test_focus_region_matches_the_oracle_with_flatfields(tmp_path, radius):
    import torch
    spec = synth.GridSpec(**SPEC)
    root = str(tmp_path / 'acq')
    synth.write_acquisition(spec, root)
    st = _prepared(root, spec, focus_radius=radius)
    assert st.num_z == 4 and st.num_c == 2
    img, depth = st.focus_region(0, 'R0', return_depth=True)
    want, key = _oracle(root, st, radius)
    np.testing.assert_array_equal(img, want)
    np.testing.assert_array_equal(depth, depth_of(key))
    assert depth.dtype == np.int32 and depth.shape == want.shape[1:2] + want.shape[3:]
    dimg, ddepth = st.focus_region(0, 'R0', device_output=True, return_depth=True)
    assert isinstance(dimg, torch.Tensor) and dimg.is_cuda
    np.testing.assert_array_equal(dimg.cpu().numpy(), want)
    np.testing.assert_array_equal(ddepth.cpu().numpy(), depth)
    # several ingest batches per channel (a few planes each): the same bits
    st.batch_bytes_limit = 2 * spec.n_tiles * spec.tile_h * spec.tile_w * 2
    np.testing.assert_array_equal(st.focus_region(0, 'R0'), want)


def test_focus_region_rgb_and_ragged(tmp_path):
    """An RGB channel (each colour is its own monochrome channel, scored on its own component) and files that are missing."""
    spec = synth.GridSpec(rows=2, cols=2, tile_h=80, tile_w=112, ov_y=15, ov_x=21, nz=3, dtype='uint8',
                          channels=(synth.DEFAULT_CHANNELS[1], 'BF LED matrix full'), rgb_channels=('BF LED matrix full',),
                          missing=((1, 2, 0, 0), (2, 0, 1, 0), (3, 1, 1, 0)), seed=5)
    root = str(tmp_path / 'acq')
    synth.write_acquisition(spec, root)
    st = _prepared(root, spec, flat_dtype=None)
    assert st.num_c == 4
    want, key = _oracle(root, st, 3)
    img, depth = st.focus_region(0, 'R0', return_depth=True)
    np.testing.assert_array_equal(img, want)
    np.testing.assert_array_equal(depth, depth_of(key))


def _run(root, *extra):
    import random
    random.seed(1234)      # -ff samples the files it fits the flatfields to at random: the same sample in every run
    stitcher_cli.main(['-i', root, '--normalization', 'none', *extra])
    base = os.path.dirname(root)
    outs = [d for d in os.listdir(base) if d.startswith(os.path.basename(root) + '_stitched_')]
    assert len(outs) == 1
    return os.path.join(base, outs[0], '0_stitched')


def test_run_writes_the_edf_stores(tmp_path):
    """-ff, nz = 4: 'focus' writes the stack and <region>_stitched_edf (OME-Zarr with its pyramid, OME-TIFF) whose voxels are
    the stack's at the winning plane of the raw tiles' keys; 'focus-only' writes the same projection and no stack."""
    from oracle import stitch_oracle as O
    from image_stitcher_amd.tiffio import read_image
    spec = synth.GridSpec(**dict(SPEC, rows=3, cols=3, tile_h=160, tile_w=192))
    roots = {k: str(tmp_path / k / 'acq') for k in ('zarr', 'only', 'tiff')}
    for r in roots.values():
        synth.write_acquisition(spec, r)
    out = _run(roots['zarr'], '-ff', '--z-projection', 'focus', '--focus-radius', '2')
    stack = omezarr.read_array(os.path.join(out, 'R0_stitched.ome.zarr', '0'))
    _, key = focus_reference_region(O.parse_acquisition(roots['zarr'], read_image), 0, 'R0', read_image, 2)
    want = np.take_along_axis(stack[0], depth_of(key).clip(0)[:, None], 1)[None]
    store = os.path.join(out, 'R0_stitched_edf.ome.zarr')
    level0 = omezarr.read_array(os.path.join(store, '0'))
    np.testing.assert_array_equal(level0, want)
    n_levels = len([d for d in os.listdir(os.path.join(out, 'R0_stitched.ome.zarr')) if d.isdigit()])
    levels = O.pyramid_nearest(level0, n_levels)
    for lv in range(1, n_levels):
        np.testing.assert_array_equal(omezarr.read_array(os.path.join(store, str(lv))), levels[lv])
    only = _run(roots['only'], '-ff', '--z-projection', 'focus-only', '--focus-radius', '2')
    assert not os.path.exists(os.path.join(only, 'R0_stitched.ome.zarr'))
    np.testing.assert_array_equal(omezarr.read_array(os.path.join(only, 'R0_stitched_edf.ome.zarr', '0')), want)
    tiff = _run(roots['tiff'], '-ff', '--z-projection', 'focus', '--focus-radius', '2', '-f', '.ome.tiff')
    planes, xml = read_ome_tiff(os.path.join(tiff, 'R0_stitched_edf.ome.tiff'))
    assert len(planes) == want.shape[1] and 'SizeZ="1"' in xml
    np.testing.assert_array_equal(np.stack(planes).reshape(want.shape), want)
    assert os.path.exists(os.path.join(tiff, 'R0_stitched.ome.tiff'))
