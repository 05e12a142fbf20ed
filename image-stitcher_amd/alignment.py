"""Global registration: every tile at its own integer position, from a least-squares solve over all registered pairs.

``--all-pairs-registration`` reduces the all-pairs table to one per-axis median, so every tile still sits on one rigid
lattice.  Here the table is used whole: each pair's measured offset is an edge between two tiles, edges the overlap does
not support are dropped, and the tile positions that best agree with the remaining edges are solved for.  Host
arithmetic on the gathered table only (numpy; the one device step, the overlap moments behind each pair's confidence,
runs where the pair was registered: registration.register_pair_subset).

    offsets        pair_offsets: the moving tile's offset d from the reference tile, as registered_rect would place two
                   neighbours with that pair's own shift (python round, crop width; stitcher.py:511,524)
    windows        overlap_window: the overlap of the two full tiles at d
    confidence     ncc_from_sums: zero-normalised cross-correlation of that overlap, from exact integer sums
    solve          solve_positions: maximum spanning forest by ncc -> tree positions -> Huber-weighted least squares
                   over all accepted edges -> edges that agree with it -> least squares over their sub-pixel offsets
                   per connected component; the gauge from the prior (the all-pairs lattice)
"""
from __future__ import annotations

import dataclasses
import math
from typing import Dict, List, Sequence, Tuple

import numpy as np

# Least zero-normalised cross-correlation of a pair's full-tile overlap for its offset to be used.  Two views of the
# same texture give values near 1 and unrelated or blank fields values near 0 (a constant field has none: NaN), so a
# threshold well between the two keeps noisy true matches and drops false ones.  Chosen on synthetic acquisitions; the
# value is NOT measured on real acquisitions.
NCC_MIN = 0.3
# Most a kept edge may disagree with the robust least-squares positions, per axis, in pixels (and where the Huber weights
# of the outlier search start to fall).  A true match disagrees by its sub-pixel noise (a few tenths of a pixel on
# synthetic data); a false peak that slipped past NCC_MIN is off by many pixels.  NOT measured on real acquisitions.
RESID_MAX = 2.0
# Components up to this many tiles are solved densely; larger ones by preconditioned conjugate gradients.
DENSE_MAX = 256
# Most robust (Huber) re-weightings of the outlier search; the weights normally settle in two to four.
HUBER_ITERS = 8

PAIR_H, PAIR_V = 0, 1     # = registration.PAIR_H / PAIR_V (kinds of grid_pair_list)


def pair_offsets(kinds: np.ndarray, shifts: np.ndarray, height: int, width: int, h_n1: int, v_n0: int):
    """Offsets of the moving tile from the reference tile per pair: (float [n, 2] sub-pixel, int64 [n, 2] rounded).
    Horizontal pair: (s0, W + s1 - n1); vertical pair: (H + s0 - n0, s1) -- what registered_rect gives two neighbours
    with that pair's own shift; the rounded form uses python's round (banker's, = numpy.rint) like pair_table_medians.
    Rows with a non-finite shift come out NaN / 0."""
    kinds = np.asarray(kinds, dtype=np.int64)
    s = np.asarray(shifts, dtype=np.float64).reshape(-1, 2)
    ok = np.isfinite(s).all(axis=1)
    s = np.where(ok[:, None], s, 0.0)
    horizontal = (kinds == PAIR_H)[:, None]
    base = np.where(horizontal, [0.0, float(width - h_n1)], [float(height - v_n0), 0.0])
    exact = s + base
    rounded = np.rint(s).astype(np.int64) + base.astype(np.int64)
    exact[~ok] = np.nan
    rounded[~ok] = 0
    return exact, rounded


def overlap_window(d, height: int, width: int) -> Tuple[int, int, int, int, int, int]:
    """(ref_y0, ref_x0, mov_y0, mov_x0, h, w) of the overlap of two full height x width tiles, the moving one at offset
    d = (dy, dx) from the reference one; all zeros when they do not overlap."""
    dy, dx = int(d[0]), int(d[1])
    h, w = height - abs(dy), width - abs(dx)
    if h <= 0 or w <= 0:
        return 0, 0, 0, 0, 0, 0
    return max(0, dy), max(0, dx), max(0, -dy), max(0, -dx), h, w


def overlap_windows(ref: Sequence[int], mov: Sequence[int], d: np.ndarray, height: int, width: int) -> np.ndarray:
    """[n, 8] int32 window records (ref_tile, mov_tile, ref_y0, ref_x0, mov_y0, mov_x0, h, w) = native.OVERLAP_DTYPE."""
    out = np.zeros((len(d), 8), dtype=np.int32)
    for i in range(len(d)):
        out[i] = (int(ref[i]), int(mov[i])) + overlap_window(d[i], height, width)
    return out


def ncc_from_sums(sums, n_pixels) -> np.ndarray:
    """Zero-normalised cross-correlation from exact sums [k, 5] (sum a, sum b, sum a^2, sum b^2, sum ab) over
    ``n_pixels`` [k]: (n Sab - Sa Sb) / sqrt((n Saa - Sa^2)(n Sbb - Sb^2)).  The three terms are formed exactly in python
    integers (they exceed int64); NaN when either variance is 0 or the window is empty."""
    sums = np.asarray(sums).reshape(-1, 5)
    n_pixels = np.asarray(n_pixels).reshape(-1)
    out = np.full(len(sums), np.nan)
    for i in range(len(sums)):
        n = int(n_pixels[i])
        sa, sb, saa, sbb, sab = (int(v) for v in sums[i])
        va, vb = n * saa - sa * sa, n * sbb - sb * sb
        if n <= 0 or va <= 0 or vb <= 0:
            continue
        out[i] = (n * sab - sa * sb) / math.sqrt(va * vb)      # exact integers up to the square root and the division
    return out


@dataclasses.dataclass
class Placement:
    """Result of the global solve for one (timepoint, region)."""
    cells: List[Tuple[int, int]]          # grid (row, col) of every present tile
    positions: np.ndarray                 # int64 [n, 2] (y, x) canvas positions, smallest y and x are 0
    by_pairs: np.ndarray                  # bool [n]: placed by pairs (else at its prior)
    canvas_hw: Tuple[int, int]            # (height, width) = (max y + H, max x + W)
    n_pairs: int = 0
    n_accepted: int = 0                   # pairs that passed the acceptance tests
    n_kept: int = 0                       # of those, the ones that agree with the spanning-forest positions
    rms_residual: float = 0.0             # of the kept edges against the least-squares positions, px

    def position_of(self) -> Dict[Tuple[int, int], Tuple[int, int]]:
        return {c: (int(p[0]), int(p[1])) for c, p in zip(self.cells, self.positions)}

    def summary(self) -> str:
        prior = int((~self.by_pairs).sum())
        return (f"[registration] global: {self.n_accepted} / {self.n_pairs} pairs accepted, {self.n_kept} kept, "
                f"RMS residual {self.rms_residual:.3f} px; {len(self.cells) - prior} tiles placed by pairs, {prior} at the "
                f"all-pairs lattice; canvas {self.canvas_hw[0]} x {self.canvas_hw[1]}")


def _find(parent: List[int], i: int) -> int:
    while parent[i] != i:
        parent[i] = parent[parent[i]]
        i = parent[i]
    return i


def _spanning_forest(n: int, ref: np.ndarray, mov: np.ndarray, weight: np.ndarray) -> np.ndarray:
    """Kruskal: indices (into the edge arrays) of a maximum spanning forest; heavier edges first, ties by the edge's
    (ref, mov) node pair, so that the forest does not depend on the order the edges are listed in."""
    parent = list(range(n))
    chosen = []
    for e in np.lexsort((mov, ref, -weight)):
        a, b = _find(parent, int(ref[e])), _find(parent, int(mov[e]))
        if a != b:
            parent[a] = b
            chosen.append(int(e))
    return np.array(chosen, dtype=np.int64)


def _components(n: int, ref: np.ndarray, mov: np.ndarray) -> np.ndarray:
    """Component label (smallest member index) per node."""
    parent = list(range(n))
    for a, b in zip(ref.tolist(), mov.tolist()):
        ra, rb = _find(parent, a), _find(parent, b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([_find(parent, i) for i in range(n)], dtype=np.int64)


def _integrate_tree(n: int, ref: np.ndarray, mov: np.ndarray, d: np.ndarray) -> np.ndarray:
    """Positions along forest edges (each tree's smallest node at 0; nodes without an edge at 0)."""
    adj: List[List[Tuple[int, int, float, float]]] = [[] for _ in range(n)]
    for a, b, (dy, dx) in zip(ref.tolist(), mov.tolist(), d.tolist()):
        adj[a].append((b, 1, dy, dx))
        adj[b].append((a, -1, dy, dx))
    pos = np.zeros((n, 2))
    seen = np.zeros(n, dtype=bool)
    for root in range(n):
        if seen[root]:
            continue
        seen[root] = True
        stack = [root]
        while stack:
            u = stack.pop()
            for v, sign, dy, dx in adj[u]:
                if not seen[v]:
                    seen[v] = True
                    pos[v] = pos[u] + sign * np.array([dy, dx])
                    stack.append(v)
    return pos


def _laplacian_solve(coords: np.ndarray, ref: np.ndarray, mov: np.ndarray, d: np.ndarray, w: np.ndarray,
                     start: np.ndarray) -> np.ndarray:
    """Weighted least-squares positions [m, 2] of nodes at grid cells ``coords`` [m, 2]: minimise
    sum_e w_e |p[mov] - p[ref] - d_e|^2.  Any gauge per connected component (the caller fixes it); ``start``: first iterate
    of the iterative solve."""
    m = len(coords)
    wd = w[:, None] * d
    b = np.stack([np.bincount(mov, wd[:, k], m) - np.bincount(ref, wd[:, k], m) for k in range(2)])     # [2, m]
    deg = np.bincount(ref, w, m) + np.bincount(mov, w, m)
    if m <= DENSE_MAX:
        L = np.diag(deg)
        np.subtract.at(L, (ref, mov), w)
        np.subtract.at(L, (mov, ref), w)
        return np.linalg.lstsq(L, b.T, rcond=None)[0]
    # Conjugate gradients on the (singular, consistent) Laplacian system, both axes at once, with a two-level
    # preconditioner: Jacobi plus an exact solve on aggregates of B x B grid cells (the Galerkin coarse Laplacian P^T L P,
    # a few hundred unknowns).  The coarse level takes out the smooth modes that make plain Jacobi CG need ~n_side
    # iterations per digit on an n_side x n_side grid.
    inv_deg = np.where(deg > 0, 1.0 / np.where(deg > 0, deg, 1.0), 0.0)
    B = max(2, int(np.ceil(np.sqrt(m / 256))))
    blk = np.asarray(coords, dtype=np.int64) // B
    _, agg = np.unique(blk[:, 0] * (int(blk[:, 1].max()) + 1) + blk[:, 1], return_inverse=True)
    agg = agg.reshape(-1)
    kc = int(agg.max()) + 1
    ca, cb = agg[ref], agg[mov]
    cross = ca != cb
    Lc = np.zeros((kc, kc))
    for i, j, sign in ((ca, cb, -1.0), (cb, ca, -1.0), (ca, ca, 1.0), (cb, cb, 1.0)):
        np.add.at(Lc, (i[cross], j[cross]), sign * w[cross])
    Lc_pinv = np.linalg.pinv(Lc, hermitian=True)
    ends = np.concatenate([mov, ref])
    w2 = np.concatenate([w, w])

    def matvec(x):          # x, result: [2, m] (axis-major: every operation below runs on contiguous rows)
        diff = x[:, mov] - x[:, ref]
        both = np.concatenate([diff, -diff], axis=1) * w2
        return np.stack([np.bincount(ends, both[0], m), np.bincount(ends, both[1], m)])

    def precondition(r):
        coarse = np.stack([np.bincount(agg, r[0], kc), np.bincount(agg, r[1], kc)]) @ Lc_pinv
        return r * inv_deg + coarse[:, agg]

    x = np.array(start, dtype=np.float64).T.copy()
    r = b - matvec(x)
    z = precondition(r)
    p = z.copy()
    rz = np.einsum('ij,ij->i', r, z)
    # Stop at |r|_2 <= 1e-6 sqrt(m) per axis.  The position error is at most |r|_2 / lambda_2 (the least nonzero
    # eigenvalue); lambda_2 of an unweighted n_side x n_side grid is ~(pi / n_side)^2, 1e-3 at 100 x 100, so every
    # position is then within 0.1 px of the exact solution before it is rounded to whole pixels.  (tests/test_alignment_cpu.py
    # checks the result against the dense solve.)
    tol = 1e-6 * np.sqrt(m)
    for _ in range(2000):
        if np.sqrt(np.einsum('ij,ij->i', r, r)).max() <= tol:
            break
        q = matvec(p)
        pq = np.einsum('ij,ij->i', p, q)
        alpha = np.where(pq > 0, rz / np.where(pq > 0, pq, 1.0), 0.0)[:, None]
        x += alpha * p
        r -= alpha * q
        z = precondition(r)
        rz_new = np.einsum('ij,ij->i', r, z)
        beta = np.where(rz > 0, rz_new / np.where(rz > 0, rz, 1.0), 0.0)[:, None]
        p = z + beta * p
        rz = rz_new
    return x.T


def _gauge(p: np.ndarray, prior: np.ndarray) -> np.ndarray:
    """Translate one component's positions so their mean is its tiles' prior mean, to within half a pixel: the fractional
    part of the translation is the one that brings the positions closest to whole pixels (circular mean of their
    fractions), so that rounding keeps every tile's position relative to the others as well as it can."""
    out = p.copy()
    for k in range(2):
        frac = np.angle(np.exp(2j * np.pi * p[:, k]).mean()) / (2 * np.pi) if len(p) > 1 else p[0, k] - np.floor(p[0, k])
        lattice = p[:, k] - frac                               # the positions moved onto whole pixels as well as they go
        out[:, k] = lattice + np.rint(prior[:, k].mean() - lattice.mean())
    return out


def _huber(resid: np.ndarray) -> np.ndarray:
    """Weights of an edge from its residual [k, 2]: 1 within RESID_MAX, RESID_MAX / |r| beyond (max over the axes)."""
    big = np.abs(resid).max(axis=1) if len(resid) else np.zeros(0)
    return np.minimum(1.0, RESID_MAX / np.maximum(big, 1e-300))


def solve_positions(pairs, table: np.ndarray, height: int, width: int, h_crop: Tuple[int, int], v_crop: Tuple[int, int],
                    prior: Dict[Tuple[int, int], Tuple[int, int]]) -> Placement:
    """The global solve of one (timepoint, region).

    ``pairs``: registration.grid_pair_list order; ``table``: [n_pairs, 4] {dy, dx, err, ncc} (raw sub-pixel shifts of
    the crop pairs, their error and the overlap ncc); ``h_crop`` / ``v_crop``: the (n0, n1) registration crop of each
    direction; ``prior``: every present cell's (y, x) on the all-pairs lattice -- where it sits without this mode.

    An edge is accepted when its shift is finite, the full-tile overlap at its offset holds at least a quarter of its
    direction's crop (n0 * n1 / 4 pixels), its ncc is at least NCC_MIN and its offset is within the direction's crop width
    of the prior's offset for that pair (the crop could not have seen farther).

    Outliers: a maximum spanning forest by ncc (ties by the pair's cells) gives tree positions, the start of a robust
    least-squares solve over every accepted edge with Huber weights (1 within RESID_MAX px, falling as RESID_MAX / |r|
    beyond), re-weighted from the residuals until the weights settle.  Tree positions alone are not the test: they drift
    along long tree paths by the sum of the edges' noise (several px on a 100 x 100 grid) and would reject true edges; a
    Huber-weighted edge still pulls with a bounded force, so the drift is taken out while a wrong offset cannot drag its
    neighbours more than a fraction of RESID_MAX.  Kept = accepted edges within RESID_MAX px of the robust positions on both
    axes.

    Positions: least squares over the kept edges' SUB-PIXEL offsets, per connected component, the gauge from the
    component's prior mean, rounded to whole pixels at the end.  Where the whole-pixel offsets of a component's kept edges
    agree with one placement exactly (every cycle closes), that placement is taken: it honours every pair to the pixel,
    which rounding a sub-pixel solution need not.  A tile with no kept edge stays at its prior."""
    cells = sorted(prior)
    index = {c: i for i, c in enumerate(cells)}
    n = len(cells)
    coords = np.array(cells, dtype=np.int64).reshape(-1, 2)
    prior_arr = np.array([prior[c] for c in cells], dtype=np.float64).reshape(-1, 2)
    table = np.asarray(table, dtype=np.float64).reshape(len(pairs), -1)
    kinds = np.array([p[0] for p in pairs], dtype=np.int64)
    ref = np.array([index[p[1]] for p in pairs], dtype=np.int64)
    mov = np.array([index[p[2]] for p in pairs], dtype=np.int64)
    exact, rounded = pair_offsets(kinds, table[:, :2], height, width, h_crop[1], v_crop[0])
    ncc = table[:, 3] if table.shape[1] > 3 else np.full(len(pairs), np.nan)
    crop_area = np.where(kinds == PAIR_H, h_crop[0] * h_crop[1], v_crop[0] * v_crop[1])
    crop_width = np.where(kinds == PAIR_H, h_crop[1], v_crop[0])
    area = np.maximum(0, height - np.abs(rounded[:, 0])) * np.maximum(0, width - np.abs(rounded[:, 1]))
    prior_d = prior_arr[mov] - prior_arr[ref] if len(pairs) else np.zeros((0, 2))
    with np.errstate(invalid='ignore'):
        accepted = (np.isfinite(exact).all(axis=1) & (4 * area >= crop_area) & (ncc >= NCC_MIN)
                    & (np.abs(rounded - prior_d) <= crop_width[:, None]).all(axis=1))
    acc = np.flatnonzero(accepted)
    ra, ma, da = ref[acc], mov[acc], exact[acc]
    tree = _spanning_forest(n, ra, ma, ncc[acc]) if len(acc) else np.zeros(0, dtype=np.int64)
    x = _integrate_tree(n, ra[tree], ma[tree], da[tree])
    w = _huber(x[ma] - x[ra] - da)
    for _ in range(HUBER_ITERS):
        if not len(acc):
            break
        x = _laplacian_solve(coords, ra, ma, da, w, x)
        again = _huber(x[ma] - x[ra] - da)
        if np.abs(again - w).max() < 1e-3:
            break
        w = again
    resid = x[ma] - x[ra] - da
    kept = acc[(np.abs(resid) <= RESID_MAX).all(axis=1)]

    pos = prior_arr.copy()
    by_pairs = np.zeros(n, dtype=bool)
    by_pairs[ref[kept]] = by_pairs[mov[kept]] = True
    label = _components(n, ref[kept], mov[kept])
    whole = rounded.astype(np.float64)
    for comp in np.unique(label[by_pairs]):
        nodes = np.flatnonzero(label == comp)
        local = np.full(n, -1, dtype=np.int64)
        local[nodes] = np.arange(len(nodes))
        edges = kept[label[ref[kept]] == comp]
        er, em = local[ref[edges]], local[mov[edges]]
        t = _spanning_forest(len(nodes), er, em, ncc[edges])
        z = _integrate_tree(len(nodes), er[t], em[t], whole[edges][t])
        if np.array_equal(z[em] - z[er], whole[edges]):
            p = z               # the whole-pixel offsets close every cycle: the placement that honours all of them
        else:
            p = _laplacian_solve(coords[nodes], er, em, exact[edges], np.ones(len(edges)), x[nodes])
        pos[nodes] = _gauge(p, prior_arr[nodes])
    rms = 0.0
    if len(kept):
        r = pos[mov[kept]] - pos[ref[kept]] - exact[kept]
        rms = float(np.sqrt((r ** 2).sum(axis=1).mean()))
    q = np.rint(pos).astype(np.int64)
    if n:
        q -= q.min(axis=0)
    canvas = (int(q[:, 0].max()) + height, int(q[:, 1].max()) + width) if n else (height, width)
    return Placement(cells, q, by_pairs, canvas, len(pairs), len(acc), len(kept), rms)


def overwrite_rects(placement: Placement, height: int, width: int) -> Dict[Tuple[int, int], Tuple[int, int, int, int, int, int]]:
    """sq_rect (src_y0, src_x0, h, w, dst_y, dst_x) per cell for overwrite fusion: each tile is cropped along each grid
    axis at the midpoint of its solved overlap with the grid neighbour on that side -- with overlap o > 0 between A (above
    / left) and B, A gives up o // 2 and B gives up o - o // 2, so the two leave neither a gap nor a double row.  No
    crop at the grid border, next to a missing neighbour, or where the neighbours do not overlap (o <= 0)."""
    at = placement.position_of()
    out = {}
    for (r, c), (y, x) in at.items():
        top = bottom = left = right = 0
        if (r - 1, c) in at:
            o = at[(r - 1, c)][0] + height - y
            top = o - o // 2 if o > 0 else 0
        if (r + 1, c) in at:
            o = y + height - at[(r + 1, c)][0]
            bottom = o // 2 if o > 0 else 0
        if (r, c - 1) in at:
            o = at[(r, c - 1)][1] + width - x
            left = o - o // 2 if o > 0 else 0
        if (r, c + 1) in at:
            o = x + width - at[(r, c + 1)][1]
            right = o // 2 if o > 0 else 0
        out[(r, c)] = (top, left, max(0, height - top - bottom), max(0, width - left - right), y + top, x + left)
    return out


def full_rects(placement: Placement, height: int, width: int) -> Dict[Tuple[int, int], Tuple[int, int, int, int, int, int]]:
    """sq_rect per cell for feather fusion: the full tile at its solved position."""
    return {c: (0, 0, height, width, int(p[0]), int(p[1])) for c, p in zip(placement.cells, placement.positions)}


def positions_csv(placement: Placement, fov_of: Dict[Tuple[int, int], int]) -> str:
    """``fov,row,col,y_px,x_px,source`` lines (header first), one per placed tile in fov order; source is 'pairs' or
    'prior'."""
    lines = ['fov,row,col,y_px,x_px,source']
    rows = []
    for (r, c), p, ok in zip(placement.cells, placement.positions, placement.by_pairs):
        rows.append((fov_of.get((r, c), -1), r, c, int(p[0]), int(p[1]), 'pairs' if ok else 'prior'))
    for row in sorted(rows):
        lines.append(','.join(str(v) for v in row))
    return '\n'.join(lines) + '\n'
