"""Global registration on the MI355X: the overlap-moment kernel against numpy's int64 sums, and -r --global-registration
end to end against the ground truth of a jittered synthetic acquisition and against the oracle."""
import os
import socket
import sys

import numpy as np
import pytest

from image_stitcher_amd import native, omezarr, placement, synth
from image_stitcher_amd.ometiff import read_ome_tiff
from image_stitcher_amd.stitcher import Stitcher
from image_stitcher_amd.stitcher_parameters import StitchingParameters
from oracle import stitch_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _want(stack, windows):
    out = np.zeros((len(windows), 5), dtype=np.int64)
    for i, (rt, mt, ry, rx, my, mx, h, w) in enumerate(windows):
        a = stack[rt, ry:ry + h, rx:rx + w].astype(np.int64)
        b = stack[mt, my:my + h, mx:mx + w].astype(np.int64)
        out[i] = (a.sum(), b.sum(), (a * a).sum(), (b * b).sum(), (a * b).sum())
    return out


@pytest.mark.parametrize('dtype', [np.uint16, np.uint8])
def test_moments_are_numpys_int64_sums(dtype):
    import torch
    rng = np.random.default_rng(3)
    th, tw = 96, 2049
    stack = rng.integers(0, np.iinfo(dtype).max + 1, (5, th, tw)).astype(dtype)
    windows = [(0, 1, 0, 0, 0, 0, th, tw),                                   # whole tiles
               (1, 2, 0, 0, th - 7, tw - 61, 7, 61), (2, 3, th - 1, tw - 1, 0, 0, 1, 1),   # corners
               (3, 4, 5, 0, 9, tw - 3, 80, 3), (4, 0, 0, 1, 40, 2, 1, 2047),             # edges, widths 3 and 2047
               (0, 0, 3, 11, 3, 11, 50, 1), (2, 4, 10, 1000, 30, 999, 60, 61),
               (1, 3, 5, 5, 5, 5, 0, 40), (1, 3, 5, 5, 5, 5, 40, 0)]               # empty windows
    # a batch of 2000 random windows at arbitrary (unaligned) columns
    for _ in range(2000):
        h, w = int(rng.integers(0, 40)), int(rng.integers(0, 300))
        windows.append((int(rng.integers(0, 5)), int(rng.integers(0, 5)), int(rng.integers(0, th - h + 1)),
                        int(rng.integers(0, tw - w + 1)), int(rng.integers(0, th - h + 1)), int(rng.integers(0, tw - w + 1)), h, w))
    windows = np.array(windows, dtype=np.int32)
    dev = torch.from_numpy(stack).cuda()
    got = native.pair_overlap_moments(dev, windows).cpu().numpy()
    np.testing.assert_array_equal(got, _want(stack, windows))
    assert not got[7:9].any()
    # a pointer table over the same tiles gives the same sums, and a second call into the same output starts from zero
    ptrs = native.pointer_table([dev[i] for i in range(5)], dev.device)
    out = torch.full((len(windows), 5), 7, dtype=torch.int64, device='cuda')
    native.pair_overlap_moments(None, windows, out=out, tile_ptrs=ptrs, shape=(th, tw), np_dtype=dtype)
    native.pair_overlap_moments(None, windows, out=out, tile_ptrs=ptrs, shape=(th, tw), np_dtype=dtype)
    np.testing.assert_array_equal(out.cpu().numpy(), got)


def test_moments_of_the_largest_window_are_exact():
    import torch
    tiles = torch.full((2, 2048, 2048), 65535, dtype=torch.uint16, device='cuda')
    got = native.pair_overlap_moments(tiles, [(0, 1, 0, 0, 0, 0, 2048, 2048)]).cpu().numpy()[0]
    n = 2048 * 2048
    assert [int(v) for v in got] == [65535 * n, 65535 * n] + [65535 * 65535 * n] * 3     # sum ab = 1.8e16, all 64 bits


def test_more_windows_than_one_call_takes():
    """A single rank of a grid beyond ~181 x 181 tiles has more than 65535 pairs: the wrapper sends them in batches."""
    import torch
    rng = np.random.default_rng(9)
    stack = rng.integers(0, 65536, (4, 40, 50)).astype(np.uint16)
    k = native.OVERLAP_BATCH + 4465
    hw = rng.integers(0, 9, (k, 2))
    windows = np.stack([rng.integers(0, 4, k), rng.integers(0, 4, k), rng.integers(0, 40 - hw[:, 0] + 1), rng.integers(0, 50 - hw[:, 1] + 1),
                        rng.integers(0, 40 - hw[:, 0] + 1), rng.integers(0, 50 - hw[:, 1] + 1), hw[:, 0], hw[:, 1]], axis=1).astype(np.int32)
    dev = torch.from_numpy(stack).cuda()
    np.testing.assert_array_equal(native.pair_overlap_moments(dev, windows).cpu().numpy(), _want(stack, windows))
    # a window outside its tile in the SECOND batch: nothing is written, not even the first batch
    out = torch.full((k, 5), -3, dtype=torch.int64, device='cuda')
    windows[-1] = (0, 1, 39, 0, 0, 0, 2, 1)
    with pytest.raises(native.NativeError):
        native.pair_overlap_moments(dev, windows, out=out)
    torch.cuda.synchronize()
    assert (out.cpu() == -3).all()


def test_window_outside_its_tile_raises_and_leaves_the_output():
    import torch
    tiles = torch.ones((2, 64, 80), dtype=torch.uint16, device='cuda')
    out = torch.full((2, 5), -3, dtype=torch.int64, device='cuda')
    for bad in ((0, 1, 0, 0, 60, 0, 5, 80), (0, 1, 0, 1, 0, 0, 64, 80), (0, 2, 0, 0, 0, 0, 1, 1), (0, 1, -1, 0, 0, 0, 1, 1)):
        with pytest.raises(native.NativeError):
            native.pair_overlap_moments(tiles, [(0, 1, 0, 0, 0, 0, 4, 4), bad], out=out)
        torch.cuda.synchronize()
        assert (out.cpu() == -3).all()


# ---------------------------------------------------------------------------------------------------------------------
# end to end: a 6 x 7 grid of 256 x 320 uint16 tiles whose scene origins are jittered by up to 6 px per tile
# ---------------------------------------------------------------------------------------------------------------------
def _spec(**kw):
    base = dict(rows=6, cols=7, tile_h=256, tile_w=320, ov_y=64, ov_x=80, seed=21, tile_jitter_px=6, noise=0)
    base.update(kw)
    return synth.GridSpec(**base)


def _stitcher(root, fusion_mode='overwrite', global_registration=True, all_pairs=False, output_format='.ome.zarr'):
    st = Stitcher(StitchingParameters(input_folder=root, use_registration=True, output_format=output_format),
                  fusion_mode=fusion_mode, global_registration=global_registration, all_pairs_registration=all_pairs)
    st.get_timepoints(); st.extract_acquisition_parameters(); st.get_pixel_size(); st.parse_acquisition_metadata()
    return st


def _truth(spec):
    o = np.array([spec.origin(r, c) for r in range(spec.rows) for c in range(spec.cols)])
    return {(r, c): tuple(o[r * spec.cols + c] - o.min(axis=0)) for r in range(spec.rows) for c in range(spec.cols)}, o.min(axis=0)


def _placed(st, spec):
    """{cell: (y, x)} of the tiles as the stitcher's rects put them (the tile's own top-left corner)."""
    out = {}
    for info in st.get_region_data(0, 'R0').values():
        sy, sx, _, _, dy, dx = st._tile_rect(info)
        out[(st.y_positions.index(info['y']), st.x_positions.index(info['x']))] = (dy - sy, dx - sx)
    lo = np.min(list(out.values()), axis=0)
    return {c: tuple(np.subtract(p, lo)) for c, p in out.items()}


@pytest.fixture(scope='module')
def jittered(tmp_path_factory):
    spec = _spec()
    root = str(tmp_path_factory.mktemp('jit') / 'acq')
    synth.write_acquisition(spec, root)
    return spec, root


def test_global_registration_reaches_the_ground_truth(jittered):
    spec, root = jittered
    truth, lo = _truth(spec)
    st = _stitcher(root)
    st.calculate_shifts(0, 'R0')
    solved = st.placements[(0, 'R0')]
    assert solved.by_pairs.all()
    assert solved.position_of() == {c: tuple(int(v) for v in p) for c, p in truth.items()}
    width, height = st.calculate_output_dimensions(0, 'R0')
    assert (height, width) == solved.canvas_hw
    canvas = st.stitch_region(0, 'R0')[0, 0, 0]
    assert canvas.shape == solved.canvas_hw
    scene = synth.scene_patch(spec.scene_seed(0, 0, 0, 0), int(lo[0]), int(lo[1]), canvas.shape[0], canvas.shape[1])
    covered = np.zeros(canvas.shape, dtype=bool)
    for info in st.get_region_data(0, 'R0').values():
        _, _, h, w, dy, dx = st._tile_rect(info)
        covered[dy:dy + h, dx:dx + w] = True
    assert covered.mean() > 0.95
    np.testing.assert_array_equal(canvas[covered], scene[covered].astype(np.uint16))
    # the same acquisition under --all-pairs-registration alone: one lattice for all tiles, so not the truth
    lattice = _stitcher(root, global_registration=False, all_pairs=True)
    lattice.calculate_shifts(0, 'R0')
    lattice.calculate_output_dimensions(0, 'R0')
    assert _placed(lattice, spec) != truth


@pytest.mark.parametrize('fusion_mode', ['overwrite', 'feather'])
def test_solved_rects_fuse_like_the_oracle(jittered, fusion_mode):
    spec, root = jittered
    st = _stitcher(root, fusion_mode=fusion_mode)
    st.calculate_shifts(0, 'R0')
    width, height = st.calculate_output_dimensions(0, 'R0')
    canvas = st.stitch_region(0, 'R0')[0, 0, 0]
    infos = list(st.get_region_data(0, 'R0').values())         # the reference's write order
    rects = np.array([st._tile_rect(i) for i in infos])
    from image_stitcher_amd.tiffio import read_image
    tiles = [read_image(i['filepath']) for i in infos]
    if fusion_mode == 'overwrite':
        want = O.fuse_plane_overwrite(tiles, rects, height, width)
    else:
        want = O.fuse_plane_feather(tiles, rects, height, width, out_dtype=np.uint16)
    np.testing.assert_array_equal(canvas, want)


def test_noisy_acquisition_with_a_blank_tile(tmp_path):
    spec_fov = 2 * 7 + 3
    spec = _spec(noise=200, blank_fovs=(spec_fov,), seed=22)
    root = str(tmp_path / 'acq')
    synth.write_acquisition(spec, root)
    truth, _ = _truth(spec)
    st = _stitcher(root)
    st.output_folder = str(tmp_path / 'out')
    st.calculate_shifts(0, 'R0')
    solved = st.placements[(0, 'R0')]
    blank = (2, 3)
    assert spec.fov_index(*blank) == spec_fov
    assert [c for c, ok in zip(solved.cells, solved.by_pairs) if not ok] == [blank]
    # every other tile at the truth, moved as a whole onto the prior's mean; the blank tile at its prior
    lattice = placement.grid_rects(spec.rows, spec.cols, spec.tile_w, spec.tile_h, st._shifts(), order=solved.cells, crop=False)
    prior = {c: np.array(r[4:6], dtype=float) for c, r in zip(solved.cells, lattice)}
    others = [c for c in solved.cells if c != blank]
    off = np.rint(np.mean([prior[c] for c in others], axis=0) - np.mean([truth[c] for c in others], axis=0))
    want = np.array([prior[c] if c == blank else np.add(truth[c], off) for c in solved.cells])
    np.testing.assert_array_equal(solved.positions, (want - want.min(axis=0)).astype(np.int64))
    path = st.write_tile_positions(0, 'R0')
    rows = [line.split(',') for line in open(path).read().strip().splitlines()]
    assert rows[0] == ['fov', 'row', 'col', 'y_px', 'x_px', 'source']
    by_fov = {int(r[0]): r for r in rows[1:]}
    assert len(by_fov) == spec.rows * spec.cols and by_fov[spec_fov][5] == 'prior'
    assert all(r[5] == 'pairs' for f, r in by_fov.items() if f != spec_fov)
    assert [int(v) for v in by_fov[spec_fov][3:5]] == list(solved.position_of()[blank])


@pytest.mark.parametrize('output_format', ['.ome.zarr', '.ome.tiff'])
def test_run_writes_the_solved_canvas_and_the_positions_file(jittered, output_format):
    spec, root = jittered
    st = _stitcher(root, output_format=output_format)
    st.run()
    solved = st.placements[(0, 'R0')]
    out = os.path.join(st.output_folder, '0_stitched')
    if output_format == '.ome.zarr':
        shape = omezarr.read_array(os.path.join(out, 'R0_stitched.ome.zarr', '0')).shape
    else:
        planes, _ = read_ome_tiff(os.path.join(out, 'R0_stitched.ome.tiff'))
        shape = planes[0].shape
    assert tuple(shape[-2:]) == solved.canvas_hw
    with open(os.path.join(out, 'R0_tile_positions.csv')) as fh:
        lines = fh.read().strip().splitlines()
    assert len(lines) == 1 + spec.rows * spec.cols
    truth, _ = _truth(spec)
    for line in lines[1:]:
        fov, r, c, y, x, src = line.split(',')
        assert (int(y), int(x)) == truth[(int(r), int(c))] and src == 'pairs'


def _worker(rank, world, port, root):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), SQ_DIST_BACKEND='gloo')
    from image_stitcher_amd import stitcher_cli
    stitcher_cli.main(['-i', root, '-r', '--global-registration'])
    import torch.distributed as dist
    dist.destroy_process_group()


def test_two_ranks_sharing_the_region_write_what_one_rank_writes(tmp_path):
    import torch.multiprocessing as mp
    spec = _spec(nz=2, seed=23)        # one region, two planes: the ranks share it plane by plane
    root = str(tmp_path / 'acq')
    synth.write_acquisition(spec, root)
    one = _stitcher(root)
    one.run()
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(2, port, root), nprocs=2, join=True)
    outs = [d for d in os.listdir(tmp_path) if d.startswith('acq_stitched_') and os.path.join(tmp_path, d) != one.output_folder]
    assert len(outs) == 1
    for name in ('R0_stitched.ome.zarr/0', 'R0_tile_positions.csv'):
        a, b = os.path.join(one.output_folder, '0_stitched', name), os.path.join(tmp_path, outs[0], '0_stitched', name)
        if name.endswith('.csv'):
            assert open(a).read() == open(b).read()
        else:
            np.testing.assert_array_equal(omezarr.read_array(a), omezarr.read_array(b))
