"""Global registration on the host (no GPU): window geometry, the ncc from exact sums, the solve, the row width of the
gathered pair table and the CLI switch."""
import os
import socket
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from image_stitcher_amd import alignment as A
from image_stitcher_amd import registration as R
from image_stitcher_amd import sharding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 512, 640
H_CROP, V_CROP = (256, 64), (48, 320)      # (n0, n1) of the horizontal / vertical registration crops
PITCH = (H - 40, W - 50)


def _grid(rows, cols, seed, jitter=6, noise=0.3, ncc=0.9):
    """Random per-tile truth around the nominal lattice, the pair table that measures it with +-noise px, and the prior
    (the nominal lattice)."""
    rng = np.random.default_rng(seed)
    truth = {(r, c): (r * PITCH[0] + int(rng.integers(-jitter, jitter + 1)), c * PITCH[1] + int(rng.integers(-jitter, jitter + 1)))
             for r in range(rows) for c in range(cols)}
    prior = {(r, c): (r * PITCH[0], c * PITCH[1]) for r in range(rows) for c in range(cols)}
    pairs = R.grid_pair_list(rows, cols)
    table = np.zeros((len(pairs), 4))
    for i, (kind, a, b) in enumerate(pairs):
        d = np.subtract(truth[b], truth[a]) + rng.uniform(-noise, noise, 2)
        raw = d - ([0, W - H_CROP[1]] if kind == R.PAIR_H else [H - V_CROP[0], 0])     # back to skimage's raw crop shift
        table[i] = (raw[0], raw[1], 0.2, ncc)
    return truth, prior, pairs, table


def _solve(pairs, table, prior):
    return A.solve_positions(pairs, table, H, W, H_CROP, V_CROP, prior)


def _rel(pos):
    pos = np.asarray(pos)
    return pos - pos.min(axis=0)


@pytest.mark.parametrize('rows, cols', [(8, 8), (100, 100)])
def test_solver_recovers_random_truth_exactly(rows, cols):
    import time
    truth, prior, pairs, table = _grid(rows, cols, seed=rows)
    t0 = time.perf_counter()
    pl = _solve(pairs, table, prior)
    took = time.perf_counter() - t0
    np.testing.assert_array_equal(pl.positions, _rel([truth[c] for c in pl.cells]))
    assert pl.by_pairs.all() and pl.n_accepted == pl.n_kept == len(pairs)
    assert pl.canvas_hw == (int(pl.positions[:, 0].max()) + H, int(pl.positions[:, 1].max()) + W)
    assert pl.positions.dtype == np.int64 and pl.positions.min() == 0
    if rows == 100:
        assert took < 1.0, took


def _subpixel_grid(rows, cols, seed, sigma):
    """Non-integer truth, Gaussian noise of sigma px on every pair: the whole-pixel offsets disagree around most cycles."""
    rng = np.random.default_rng(seed)
    pitch = (PITCH[0] + 0.37, PITCH[1] - 0.29)
    truth = {(r, c): (r * pitch[0] + rng.uniform(-6, 6), c * pitch[1] + rng.uniform(-6, 6)) for r in range(rows) for c in range(cols)}
    prior = {(r, c): (r * PITCH[0], c * PITCH[1]) for r in range(rows) for c in range(cols)}
    pairs = R.grid_pair_list(rows, cols)
    table = np.zeros((len(pairs), 4))
    for i, (kind, a, b) in enumerate(pairs):
        d = np.subtract(truth[b], truth[a]) + rng.normal(0, sigma, 2)
        raw = d - ([0, W - H_CROP[1]] if kind == R.PAIR_H else [H - V_CROP[0], 0])
        table[i] = (raw[0], raw[1], 0.2, 0.9)
    return truth, prior, pairs, table


@pytest.mark.parametrize('sigma, outliers', [(0.3, 0), (0.1, 0), (0.3, 40)])
def test_solver_on_inconsistent_subpixel_offsets_of_a_100_by_100_grid(sigma, outliers):
    """The case that matters on real acquisitions: the true offsets are not whole pixels, so the rounded offsets do not
    close their cycles.  Every true pair must be kept, every tile within 2 px of the truth (up to one translation), the
    position RMSE per axis at most 0.5 px, and the solve well under a second."""
    import time
    truth, prior, pairs, table = _subpixel_grid(100, 100, seed=11 + outliers, sigma=sigma)
    bad = np.random.default_rng(5).choice(len(pairs), outliers, replace=False)
    table[bad, 1] += np.where(np.arange(outliers) % 2, 7.0, -25.0)          # wrong peaks that passed NCC_MIN
    table[bad, 3] = 0.5
    t0 = time.perf_counter()
    pl = _solve(pairs, table, prior)
    took = time.perf_counter() - t0
    err = pl.positions - np.array([truth[c] for c in pl.cells])
    err -= err.mean(axis=0)
    assert pl.n_kept == len(pairs) - outliers and pl.by_pairs.all()
    assert np.abs(err).max() <= 2.0, np.abs(err).max()
    assert np.sqrt((err ** 2).mean(axis=0)).max() <= 0.5, np.sqrt((err ** 2).mean(axis=0))
    if outliers == 0:
        assert took < 1.0, took


def test_iterative_solve_agrees_with_the_dense_solve():
    """A component just above DENSE_MAX with inconsistent offsets: conjugate gradients (two-level preconditioner) against
    numpy's dense least squares, to 1e-3 px after both are put in the same gauge."""
    _, _, pairs, table = _subpixel_grid(16, 17, seed=3, sigma=0.3)
    assert 16 * 17 > A.DENSE_MAX
    cells = sorted({c for p in pairs for c in p[1:]})
    index = {c: i for i, c in enumerate(cells)}
    ref = np.array([index[p[1]] for p in pairs])
    mov = np.array([index[p[2]] for p in pairs])
    kinds = np.array([p[0] for p in pairs])
    d, _ = A.pair_offsets(kinds, table[:, :2], H, W, H_CROP[1], V_CROP[0])
    rng = np.random.default_rng(0)
    w = rng.uniform(0.2, 1.0, len(pairs))
    coords = np.array(cells)
    got = A._laplacian_solve(coords, ref, mov, d, w, np.zeros((len(cells), 2)))
    L = np.zeros((len(cells), len(cells)))
    np.add.at(L, (ref, mov), -w); np.add.at(L, (mov, ref), -w); np.add.at(L, (ref, ref), w); np.add.at(L, (mov, mov), w)
    b = np.zeros((len(cells), 2))
    np.add.at(b, mov, w[:, None] * d); np.subtract.at(b, ref, w[:, None] * d)
    want = np.linalg.lstsq(L, b, rcond=None)[0]
    np.testing.assert_allclose(got - got.mean(axis=0), want - want.mean(axis=0), rtol=0, atol=1e-3)


def test_one_confident_wrong_pair_is_dropped():
    truth, prior, pairs, table = _grid(8, 8, seed=3)
    bad = next(i for i, p in enumerate(pairs) if p[1] == (3, 3) and p[0] == R.PAIR_H)
    table[bad, 0] += 9          # 9 px off in y, still inside the crop width of the prior
    table[bad, 3] = 0.6         # and above NCC_MIN
    pl = _solve(pairs, table, prior)
    np.testing.assert_array_equal(pl.positions, _rel([truth[c] for c in pl.cells]))
    assert pl.n_accepted == len(pairs) and pl.n_kept == len(pairs) - 1


def _expected(cells, groups, prior, truth):
    """Positions the solve should give before its final translation: every group (a connected component) at its truth,
    moved by the whole pixels that put its mean on its prior mean; cells in no group at their prior."""
    out = {c: np.array(prior[c], dtype=float) for c in cells}
    for group in groups:
        t = np.array([truth[c] for c in group], dtype=float)
        p = np.array([prior[c] for c in group], dtype=float)
        off = np.rint(p.mean(axis=0) - t.mean(axis=0))
        for c in group:
            out[c] = np.array(truth[c]) + off
    return _rel([out[c] for c in cells]).astype(np.int64)


def test_tile_whose_pairs_all_lack_ncc_sits_at_its_prior():
    truth, prior, pairs, table = _grid(5, 6, seed=4)
    lonely = (2, 3)
    table[[i for i, p in enumerate(pairs) if lonely in p[1:]], 3] = np.nan
    pl = _solve(pairs, table, prior)
    assert [c for c, ok in zip(pl.cells, pl.by_pairs) if not ok] == [lonely]
    np.testing.assert_array_equal(pl.positions, _expected(pl.cells, [[c for c in pl.cells if c != lonely]], prior, truth))


def test_two_components_are_each_centred_on_their_prior_mean():
    truth, prior, pairs, table = _grid(6, 5, seed=5)
    # every vertical pair from row 2 to row 3 rejected: rows 0-2 and rows 3-5 are separate components
    table[[i for i, p in enumerate(pairs) if p[0] == R.PAIR_V and p[1][0] == 2], 3] = 0.05
    pl = _solve(pairs, table, prior)
    assert pl.by_pairs.all() and pl.n_accepted == len(pairs) - 5
    top, bottom = [c for c in pl.cells if c[0] < 3], [c for c in pl.cells if c[0] >= 3]
    np.testing.assert_array_equal(pl.positions, _expected(pl.cells, [top, bottom], prior, truth))
    # the split shows: the two halves do not keep their true offset from each other
    assert not np.array_equal(pl.positions, _rel([truth[c] for c in pl.cells]))


def test_solve_is_deterministic_and_ignores_the_order_of_tied_weights():
    truth, prior, pairs, table = _grid(6, 6, seed=6, noise=0.0, ncc=0.8)
    table[7, 0] += 5            # one wrong edge with the same weight as every other
    a, b = _solve(pairs, table, prior), _solve(pairs, table.copy(), prior)
    np.testing.assert_array_equal(a.positions, b.positions)
    # the same edges listed in another order: the tree may differ, the kept set and the positions may not
    perm = np.random.default_rng(0).permutation(len(pairs))
    c = _solve([pairs[i] for i in perm], table[perm], prior)
    np.testing.assert_array_equal(c.positions, a.positions)
    assert (a.n_kept, a.n_accepted) == (c.n_kept, c.n_accepted)


@pytest.mark.parametrize('dy', [-37, -1, 0, 5])
@pytest.mark.parametrize('dx', [-60, 0, 3, 590])
def test_overlap_window_matches_brute_force(dy, dx):
    h, w = 40, 64 + 600
    canvas_a = np.zeros((3 * h, 3 * w), dtype=bool)
    canvas_b = np.zeros_like(canvas_a)
    canvas_a[h:2 * h, w:2 * w] = True
    canvas_b[h + dy:2 * h + dy, w + dx:2 * w + dx] = True
    both = np.argwhere(canvas_a & canvas_b)
    ry, rx, my, mx, oh, ow = A.overlap_window((dy, dx), h, w)
    if len(both) == 0:
        assert (oh, ow) == (0, 0)
        return
    (y0, x0), (y1, x1) = both.min(axis=0), both.max(axis=0)
    assert (oh, ow) == (y1 - y0 + 1, x1 - x0 + 1) and oh * ow == len(both)
    assert (ry, rx) == (y0 - h, x0 - w)                     # in the reference tile's pixels
    assert (my, mx) == (y0 - h - dy, x0 - w - dx)           # in the moving tile's pixels


def test_ncc_from_exact_sums_equals_corrcoef():
    rng = np.random.default_rng(1)
    sums, sizes, want = [], [], []
    for n, hi in ((7, 255), (1000, 65535), (4096, 3)):
        a = rng.integers(0, hi + 1, n)
        b = (a // 2 + rng.integers(0, hi // 2 + 1, n)).astype(np.int64)
        sums.append([a.sum(), b.sum(), (a * a).sum(), (b * b).sum(), (a * b).sum()])
        sizes.append(n)
        want.append(np.corrcoef(a, b)[0, 1])
    got = A.ncc_from_sums(np.array(sums, dtype=np.int64), sizes)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    # a constant side, an empty window: NaN; the largest window of 65535s does not overflow (python integers)
    n = 2048 * 2048
    full = [65535 * n, 65535 * n, 65535 ** 2 * n, 65535 ** 2 * n, 65535 ** 2 * n]
    assert np.isnan(A.ncc_from_sums([full, [0] * 5], [n, 0])).all()


def test_pair_offsets_convert_like_the_medians():
    pairs = R.grid_pair_list(2, 2)
    table = np.array([[2.5, 60.4, 0], [-3.5, 1.6, 0], [1.4, 63.5, 0], [0.0, 0.0, 0]], dtype=np.float64)
    kinds = np.array([p[0] for p in pairs])
    _, d = A.pair_offsets(kinds, table[:, :2], H, W, H_CROP[1], V_CROP[0])
    for i, (kind, _, _) in enumerate(pairs):
        if kind == R.PAIR_H:
            dy, dx = R.horizontal_shift_from(table[i, :2], H_CROP[1])
            assert tuple(d[i]) == (dy, W + dx)
        else:
            dy, dx = R.vertical_shift_from(table[i, :2], V_CROP[0])
            assert tuple(d[i]) == (H + dy, dx)


def test_overwrite_rects_split_overlaps_at_their_midpoint():
    pl = A.Placement([(0, 0), (0, 1), (1, 0)], np.array([[3, 0], [0, W - 51], [H - 41, 2]]), np.ones(3, bool), (0, 0))
    rects = A.overwrite_rects(pl, H, W)
    o = W - (W - 51)            # 51 columns: the left tile gives up 25, the right one 26
    assert rects[(0, 0)][3] == W - o // 2 and rects[(0, 1)][1] == o - o // 2
    assert rects[(0, 0)][5] + rects[(0, 0)][3] == rects[(0, 1)][5]          # neither gap nor double column
    ov = 3 + H - (H - 41)       # 44 rows between (0, 0) and (1, 0)
    assert rects[(0, 0)][2] == H - ov // 2 and rects[(1, 0)][0] == ov - ov // 2
    assert rects[(0, 0)][4] + rects[(0, 0)][2] == rects[(1, 0)][4]
    assert rects[(0, 1)][2] == H and rects[(0, 1)][0] == 0     # no neighbour below: no crop
    assert all(r[:4] == (0, 0, H, W) for r in A.full_rects(pl, H, W).values())


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _width4_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from image_stitcher_amd import sharding as sh
        for n_pairs in (1984, 7, 2):
            full = np.arange(n_pairs * 4, dtype=np.float64).reshape(n_pairs, 4) * 0.25 - 3.0
            full[::3, 3] = np.nan                        # pairs without an ncc travel as NaN
            mine = sh.contiguous_blocks(n_pairs, rank, world)
            table = sh.all_gather_pair_table(full[mine], n_pairs, rank, world, width=4)
            assert table.shape == (n_pairs, 4)
            np.testing.assert_array_equal(table, full)
        open(os.path.join(out_dir, f'w4_ok{rank}'), 'w').close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('world', [2, 3])
def test_pair_table_of_width_four_all_gathers_over_gloo(tmp_path, world):
    mp.spawn(_width4_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    assert all((tmp_path / f'w4_ok{r}').exists() for r in range(world))
    full = np.ones((3, 4))
    np.testing.assert_array_equal(sharding.all_gather_pair_table(full, 3, 0, 1, width=4), full)


def test_cli_global_registration_switch(tmp_path):
    from image_stitcher_amd import stitcher_cli, synth
    from image_stitcher_amd.stitcher import Stitcher
    args = stitcher_cli.parse_args(['-i', 'x', '-r', '--global-registration'])
    assert args.global_registration and args.use_registration
    assert not stitcher_cli.parse_args(['-i', 'x']).global_registration
    root = str(tmp_path / 'acq')
    synth.write_acquisition(synth.GridSpec(rows=1, cols=2, tile_h=32, tile_w=48, ov_y=8, ov_x=8), root)
    on = Stitcher(stitcher_cli.create_params(stitcher_cli.parse_args(['-i', root, '-r'])), global_registration=True)
    off = Stitcher(stitcher_cli.create_params(stitcher_cli.parse_args(['-i', root])), global_registration=True)
    assert on.global_registration and on._per_unit_registration
    assert not off.global_registration and not off._per_unit_registration      # needs -r, like --all-pairs-registration


def test_synthetic_tile_jitter_moves_each_origin_and_keeps_the_stage():
    from image_stitcher_amd import synth
    base = synth.GridSpec(rows=3, cols=4, tile_h=32, tile_w=48, ov_y=8, ov_x=8)
    jit = synth.GridSpec(rows=3, cols=4, tile_h=32, tile_w=48, ov_y=8, ov_x=8, tile_jitter_px=5)
    moves = [np.subtract(jit.origin(r, c), base.origin(r, c)) for r in range(3) for c in range(4)]
    assert all(np.abs(m).max() <= 5 for m in moves) and len({tuple(m) for m in moves}) > 6
    assert all(jit.stage_mm(r, c) == base.stage_mm(r, c) for r in range(3) for c in range(4))
    np.testing.assert_array_equal(synth.GridSpec(rows=2, cols=2, tile_h=16, tile_w=16, ov_y=4, ov_x=4, tile_jitter_px=0).tile_stack(),
                                  synth.GridSpec(rows=2, cols=2, tile_h=16, tile_w=16, ov_y=4, ov_x=4).tile_stack())
    with pytest.raises(ValueError):
        synth.write_acquisition_device(jit, '/nonexistent', device=None)
