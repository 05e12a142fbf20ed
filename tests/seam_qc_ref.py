"""The numpy definition of the words sq_seam_stats writes per (plane, seam) (include/squidstitch.h), and an independent
restatement of what image_stitcher_amd/seamqc.py makes of them: the seam list, the derived columns and the table of an
acquisition's planes.  Not a test module."""
import math
from fractions import Fraction

import numpy as np

HEADER = 'region,channel,z_level,ref_fov,mov_fov,kind,dy,dx,pixels,mean_ref,mean_mov,mad,ncc,best_dy,best_dx,best_ncc,flags'


def n_words(radius):
    return 3 + 3 * (2 * radius + 1) ** 2


def _total(a):
    """The exact sum of a non-negative integer array as a Python integer (uint64 partial sums per row, added as objects)."""
    a = np.asarray(a, dtype=np.uint64)
    return sum(int(v) for v in a.reshape(a.shape[0], -1).sum(axis=1, dtype=np.uint64)) if a.size else 0


def pair_words(ref, mov, window, radius):
    """The words of one pair as Python integers: ``window`` = (ref_y0, ref_x0, mov_y0, mov_x0, hc, wc), the core at e = 0."""
    ry, rx, my, mx, hc, wc = (int(v) for v in window)
    a = np.asarray(ref)[ry:ry + hc, rx:rx + wc].astype(np.uint64)
    assert a.shape == (hc, wc)
    b0 = np.asarray(mov)[my:my + hc, mx:mx + wc].astype(np.uint64)
    out = [_total(a), _total(a * a), _total(np.where(a > b0, a - b0, b0 - a))]
    for ey in range(-radius, radius + 1):
        for ex in range(-radius, radius + 1):
            assert my - ey >= 0 and mx - ex >= 0
            b = np.asarray(mov)[my - ey:my - ey + hc, mx - ex:mx - ex + wc].astype(np.uint64)
            assert b.shape == (hc, wc)
            out += [_total(b), _total(b * b), _total(a * b)]
    return out


def words_of(tiles, pairs, radius):
    """[m, k, words] int64 of a [m, n, H, W] stack and [k, 8] records (ref_tile, mov_tile, then a window)."""
    tiles = np.asarray(tiles)
    out = np.zeros((tiles.shape[0], len(pairs), n_words(radius)), dtype=np.int64)
    for p in range(tiles.shape[0]):
        for i, rec in enumerate(pairs):
            rec = [int(v) for v in rec]
            out[p, i] = pair_words(tiles[p, rec[0]], tiles[p, rec[1]], rec[2:], radius)
    return out


def seams_of(rects, h, w, radius, min_pixels):
    """Every pair of fovs of ``{fov: (src_y0, src_x0, h, w, dst_y, dst_x)}`` whose core has at least min_pixels pixels, by brute
    force: [(ref_fov, mov_fov, dy, dx, kind, n, window)] sorted by (ref_fov, mov_fov)."""
    o = {f: (int(r[4]) - int(r[0]), int(r[5]) - int(r[1])) for f, r in rects.items()}
    found = []
    for f in sorted(o):
        for g in sorted(o):
            if g <= f:
                continue
            dy, dx = o[g][0] - o[f][0], o[g][1] - o[f][1]
            ho, wo = h - abs(dy), w - abs(dx)
            hc, wc = ho - 2 * radius, wo - 2 * radius
            if hc < 1 or wc < 1 or hc * wc < min_pixels:
                continue
            window = (max(dy, 0) + radius, max(dx, 0) + radius, max(-dy, 0) + radius, max(-dx, 0) + radius, hc, wc)
            found.append((f, g, dy, dx, 'h' if ho >= wo else 'v', hc * wc, window))
    return found


def derive(words, n, radius):
    """(mean_ref, mean_mov, mad, ncc, best) -- ncc and best = (ey, ex, ncc) are None for a featureless pair.  The order of the
    offsets is that of exact rationals: sign(num) num^2 / vb."""
    w = [int(v) for v in words]
    side = 2 * radius + 1
    sa, saa, sad = w[:3]
    va = n * saa - sa * sa
    cand = {}
    for i in range(side * side):
        sb, sbb, sab = w[3 + 3 * i:6 + 3 * i]
        cand[(i // side - radius, i % side - radius)] = (n * sab - sa * sb, n * sbb - sb * sb, sb)
    num0, vb0, sb0 = cand[(0, 0)]
    means = (float(Fraction(sa, n)), float(Fraction(sb0, n)), float(Fraction(sad, n)))
    if va == 0 or vb0 == 0:
        return means + (None, None)
    score = {e: Fraction(num * abs(num), vb) for e, (num, vb, _) in cand.items() if vb > 0}
    top = max(score.values())
    ey, ex = min((e for e in score if score[e] == top), key=lambda e: (e[0] * e[0] + e[1] * e[1], e[0], e[1]))
    return means + (num0 / math.sqrt(va * vb0), (ey, ex, cand[(ey, ex)][0] / math.sqrt(va * cand[(ey, ex)][1])))


def _cell(v):
    return '' if v is None else (repr(v) if isinstance(v, float) else str(v))


def row_of(region, channel, z, seam, words, radius, min_ncc):
    """One CSV row (strings); ``words`` None: unmeasured."""
    f, g, dy, dx, kind, n, _ = seam
    head = [region, channel, str(z), str(f), str(g), kind, str(dy), str(dx), str(n)]
    if words is None:
        return head + [''] * 7 + ['unmeasured']
    mean_ref, mean_mov, mad, ncc, best = derive(words, n, radius)
    if ncc is None:
        return head + [_cell(mean_ref), _cell(mean_mov), _cell(mad), '', '', '', '', 'featureless']
    flags = (['low_ncc'] if ncc < min_ncc else []) + (['shifted'] if best[:2] != (0, 0) else [])
    return head + [_cell(mean_ref), _cell(mean_mov), _cell(mad), _cell(ncc), str(best[0]), str(best[1]), _cell(best[2]),
                   '|'.join(flags)]


def table_of(entries, channel_order, rects, h, w, radius, min_pixels, min_ncc, region='R0', unmeasured=()):
    """The CSV's rows (lists of strings, the header first) from entries [(fov, z_level, channel, plane)] and the tiles'
    rectangles {fov: rect}: for every (channel, z) the seams both of whose tiles have an entry, sorted by (channel order, z,
    ref_fov, mov_fov).  ``unmeasured``: (ref_fov, mov_fov) pairs reported without words."""
    planes = {}
    for fov, z, channel, plane in entries:
        planes.setdefault((channel_order.index(channel), z), {})[fov] = plane
    seams = seams_of(rects, h, w, radius, min_pixels)
    lines = [HEADER.split(',')]
    for (ci, z) in sorted(planes):
        have = planes[(ci, z)]
        for seam in seams:
            f, g = seam[0], seam[1]
            if f in have and g in have:
                words = None if (f, g) in unmeasured else pair_words(have[f], have[g], seam[6], radius)
                lines.append(row_of(region, channel_order[ci], z, seam, words, radius, min_ncc))
    return lines
