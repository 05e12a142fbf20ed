"""--seam-qc: the per-seam alignment table derived from the words sq_seam_stats writes for every (plane, pair of overlapping
tiles) of the staged planes (include/squidstitch.h; an extension, the reference has none).  Host only: Python integers, one
square root and one division per ncc, so that a second implementation (tests/seam_qc_ref.py) agrees bit for bit.

Geometry.  A tile of H x W pixels with rectangle (src_y0, src_x0, h, w, dst_y, dst_x) has the full-tile canvas origin
o = (dst_y - src_y0, dst_x - src_x0) -- for coordinate, registered (cropped or not), global and row-band-clipped rectangles
alike.  Of two tiles of one region, ref is the one with the smaller fov index and mov the other; d = o_mov - o_ref, and
alignment.overlap_window(d, H, W) is their overlap (ry0, rx0, my0, mx0, ho, wo).

Core.  The overlap inset by R on all four sides: hc = ho - 2R, wc = wo - 2R, n = hc * wc; the ref window starts at
(ry0 + R, rx0 + R), the mov window at (my0 + R, mx0 + R).  A pair is a seam of the region when n >= seam_qc_min_pixels --
purely geometric: off-grid stage positions, ragged grids and diagonal corner neighbours need no special case.  A seam is
listed for a (channel, z) plane when both files of that plane exist.  kind is 'h' when ho >= wo, else 'v'.

Words per (plane, seam).  With a(y, x) = ref[ry + y, rx + x] and b_e(y, x) = mov[my + y - ey, mx + x - ex] over the core, for
every e = (ey, ex) in [-R, R]^2:  Sa, Saa, Sad = sum |a - b_0|;  then, row-major over (ey, ex): Sb_e, Sbb_e, Sab_e --
3 + 3 (2R + 1)^2 non-negative integers.  When the tiles agree at e, their true displacement is d + e.

Derived, in Python integers:  va = n Saa - Sa^2,  vb_e = n Sbb_e - Sb_e^2,  num_e = n Sab_e - Sa Sb_e,
ncc_e = num_e / math.sqrt(va * vb_e) where both variances are > 0 (alignment.ncc_from_sums's arithmetic).  best is the e with
the largest ncc, compared exactly: e1 beats e2 iff num1 |num1| vb2 > num2 |num2| vb1; ties go to the smaller ey^2 + ex^2, then
the smaller ey, then the smaller ex.  Columns: mean_ref = Sa / n, mean_mov = Sb_0 / n, mad = Sad / n, ncc = ncc_0, best_dy,
best_dx, best_ncc.

Flags, joined with '|' in this order: 'unmeasured' (no call staged both tiles together -- only when row-band calls split a
seam exactly at a band edge; the row keeps its geometry, the other cells stay empty), 'featureless' (va == 0 or vb_0 == 0: a
blank tile; the ncc and best cells are empty), 'low_ncc' (ncc < seam_qc_min_ncc), 'shifted' (best != (0, 0)).

The values are the staged planes exactly as the fusion reads them: after --dpc, --despeckle and --background-subtract, before
the flatfield divide.  ncc does not depend on gain or offset, so smooth vignetting barely moves it; the means are raw counts."""
from __future__ import annotations

import json
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import alignment

MAX_RADIUS = 3
CSV_HEADER = ('region', 'channel', 'z_level', 'ref_fov', 'mov_fov', 'kind', 'dy', 'dx', 'pixels', 'mean_ref', 'mean_mov', 'mad',
              'ncc', 'best_dy', 'best_dx', 'best_ncc', 'flags')
FLAGS = ('unmeasured', 'featureless', 'low_ncc', 'shifted')


def n_words(radius: int) -> int:
    return 3 + 3 * (2 * int(radius) + 1) ** 2


def _is_int(v) -> bool:
    return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, np.integer))


def check_options(seam_qc, radius, min_pixels, min_ncc):
    """The Stitcher's four arguments, validated: (bool, int in 0..3, int >= 1, float in [-1, 1]); ValueError otherwise."""
    if not isinstance(seam_qc, (bool, np.bool_)):
        raise ValueError(f"seam_qc must be a bool, got {seam_qc!r}")
    if not _is_int(radius) or not 0 <= int(radius) <= MAX_RADIUS:
        raise ValueError(f"seam_qc_radius must be an integer in 0..{MAX_RADIUS}, got {radius!r}")
    if not _is_int(min_pixels) or int(min_pixels) < 1:
        raise ValueError(f"seam_qc_min_pixels must be an integer of at least 1, got {min_pixels!r}")
    if isinstance(min_ncc, (bool, np.bool_)) or not isinstance(min_ncc, (int, float, np.integer, np.floating)) or \
            not -1.0 <= float(min_ncc) <= 1.0:
        raise ValueError(f"seam_qc_min_ncc must be a number in [-1, 1], got {min_ncc!r}")
    return bool(seam_qc), int(radius), int(min_pixels), float(min_ncc)


def origin_of(rect) -> Tuple[int, int]:
    """The full-tile canvas origin (dst_y - src_y0, dst_x - src_x0) of a rectangle."""
    src_y0, src_x0, _, _, dst_y, dst_x = (int(v) for v in rect)
    return dst_y - src_y0, dst_x - src_x0


def region_seams(rects: Dict[int, Sequence[int]], height: int, width: int, radius: int, min_pixels: int) -> List[dict]:
    """The seams among the tiles ``{fov: rectangle}`` of one region, sorted by (ref_fov, mov_fov): dicts with ref_fov, mov_fov,
    dy, dx (d = o_mov - o_ref), kind, pixels (n) and window = (ref_y0, ref_x0, mov_y0, mov_x0, hc, wc), the core windows at
    e = 0.  Tiles are bucketed by origin, so only near neighbours are compared."""
    height, width, radius = int(height), int(width), int(radius)
    origins = {int(f): origin_of(r) for f, r in rects.items()}
    buckets: Dict[Tuple[int, int], List[int]] = {}
    for f, (oy, ox) in origins.items():
        buckets.setdefault((oy // height, ox // width), []).append(f)
    seams = []
    for f in sorted(origins):
        oy, ox = origins[f]
        by, bx = oy // height, ox // width
        near = [g for ny in (by - 1, by, by + 1) for nx in (bx - 1, bx, bx + 1) for g in buckets.get((ny, nx), ()) if g > f]
        for g in sorted(near):
            dy, dx = origins[g][0] - oy, origins[g][1] - ox
            ry0, rx0, my0, mx0, ho, wo = alignment.overlap_window((dy, dx), height, width)
            hc, wc = ho - 2 * radius, wo - 2 * radius
            if hc <= 0 or wc <= 0 or hc * wc < min_pixels:
                continue
            seams.append({'ref_fov': f, 'mov_fov': g, 'dy': dy, 'dx': dx, 'kind': 'h' if ho >= wo else 'v', 'pixels': hc * wc,
                          'window': (ry0 + radius, rx0 + radius, my0 + radius, mx0 + radius, hc, wc)})
    return seams


def pair_table(seams: Sequence[dict], index_of: Dict[int, int]) -> np.ndarray:
    """[k, 8] int32 records (ref_tile, mov_tile, ref_y0, ref_x0, mov_y0, mov_x0, h, w) = native.OVERLAP_DTYPE of ``seams``,
    ``index_of`` giving a fov's position in the staged tile list."""
    out = np.zeros((len(seams), 8), dtype=np.int32)
    for i, s in enumerate(seams):
        out[i] = (index_of[s['ref_fov']], index_of[s['mov_fov']]) + tuple(s['window'])
    return out


def _beats(num1: int, vb1: int, num2: int, vb2: int) -> int:
    """+1 when ncc1 > ncc2, -1 when ncc1 < ncc2, 0 when equal -- exactly (both share va > 0; vb1, vb2 > 0)."""
    l, r = num1 * abs(num1) * vb2, num2 * abs(num2) * vb1
    return (l > r) - (l < r)


def derive(words: Sequence[int], n: int, radius: int) -> dict:
    """mean_ref, mean_mov, mad of one (plane, seam) from its words, 'featureless', and -- None when featureless -- ncc, best_dy,
    best_dx, best_ncc."""
    radius, n = int(radius), int(n)
    side = 2 * radius + 1
    w = [int(v) for v in words]
    if len(w) != n_words(radius):
        raise ValueError(f"{len(w)} words, radius {radius} has {n_words(radius)}")
    sa, saa, sad = w[:3]

    def at(ey, ex):
        i = 3 + 3 * ((ey + radius) * side + (ex + radius))
        return w[i], w[i + 1], w[i + 2]

    va = n * saa - sa * sa
    sb0, sbb0, sab0 = at(0, 0)
    out = {'mean_ref': sa / n, 'mean_mov': sb0 / n, 'mad': sad / n, 'featureless': va <= 0 or n * sbb0 - sb0 * sb0 <= 0,
           'ncc': None, 'best_dy': None, 'best_dx': None, 'best_ncc': None}
    if out['featureless']:
        return out
    best = None      # (num, vb, ey, ex)
    for ey in range(-radius, radius + 1):
        for ex in range(-radius, radius + 1):
            sb, sbb, sab = at(ey, ex)
            vb, num = n * sbb - sb * sb, n * sab - sa * sb
            if vb <= 0:
                continue
            if (ey, ex) == (0, 0):
                out['ncc'] = num / math.sqrt(va * vb)
            if best is not None:
                c = _beats(num, vb, best[0], best[1])
                if c < 0 or (c == 0 and (ey * ey + ex * ex, ey, ex) >= (best[2] * best[2] + best[3] * best[3], best[2], best[3])):
                    continue
            best = (num, vb, ey, ex)
    out['best_dy'], out['best_dx'], out['best_ncc'] = best[2], best[3], best[0] / math.sqrt(va * best[1])
    return out


def make_row(region, channel: str, z_level: int, seam: dict, words: Optional[Sequence[int]], radius: int) -> dict:
    """One row of the table (flags are filled in by flag_rows); ``words`` None: the seam was not measured."""
    row = {'region': region, 'channel': channel, 'z_level': int(z_level), 'ref_fov': int(seam['ref_fov']),
           'mov_fov': int(seam['mov_fov']), 'kind': seam['kind'], 'dy': int(seam['dy']), 'dx': int(seam['dx']),
           'pixels': int(seam['pixels']), 'mean_ref': None, 'mean_mov': None, 'mad': None, 'ncc': None, 'best_dy': None,
           'best_dx': None, 'best_ncc': None, 'flags': '', 'measured': words is not None, 'featureless': False}
    if words is not None:
        row.update(derive(words, seam['pixels'], radius))
    return row


def flag_rows(rows: List[dict], min_ncc: float) -> List[dict]:
    """Fill 'flags' of the rows in place; returns them."""
    for r in rows:
        flags = []
        if not r['measured']:
            flags.append('unmeasured')
        elif r['featureless']:
            flags.append('featureless')
        else:
            if r['ncc'] < min_ncc:
                flags.append('low_ncc')
            if (r['best_dy'], r['best_dx']) != (0, 0):
                flags.append('shifted')
        r['flags'] = '|'.join(flags)
    return rows


def _cell(v) -> str:
    if v is None:
        return ''
    return repr(float(v)) if isinstance(v, (float, np.floating)) else str(v)


def csv_text(rows: List[dict]) -> str:
    """The CSV: integers as integers, floats with repr, cells that do not apply empty."""
    lines = [','.join(CSV_HEADER)]
    for r in rows:
        lines.append(','.join(_cell(r[k]) for k in CSV_HEADER))
    return '\n'.join(lines) + '\n'


def summary(rows: List[dict], channels: Sequence[str], radius: int, min_pixels: int, min_ncc: float) -> dict:
    """What the JSON beside the CSV says: the settings, the row count, the count of each flag, the flagged rows and, per
    channel over the measured rows that are not featureless, the median ncc per z and a histogram of "best_dy,best_dx"."""
    median_ncc: Dict[str, Dict[str, Optional[float]]] = {}
    best_hist: Dict[str, Dict[str, int]] = {}
    for name in channels:
        of = [r for r in rows if r['channel'] == name]
        if not of:
            continue
        good = [r for r in of if r['measured'] and not r['featureless']]
        median_ncc[name] = {}
        for z in sorted({r['z_level'] for r in of}):
            v = [r['ncc'] for r in good if r['z_level'] == z]
            median_ncc[name][str(z)] = float(np.median(np.array(v, dtype=np.float64))) if v else None
        hist: Dict[str, int] = {}
        for r in sorted(good, key=lambda r: (r['best_dy'], r['best_dx'])):
            k = f"{r['best_dy']},{r['best_dx']}"
            hist[k] = hist.get(k, 0) + 1
        best_hist[name] = hist
    counts = {f: sum(1 for r in rows if f in r['flags'].split('|')) for f in FLAGS}
    flagged = [{'channel': r['channel'], 'z_level': r['z_level'], 'ref_fov': r['ref_fov'], 'mov_fov': r['mov_fov'],
                'flags': r['flags']} for r in rows if r['flags']]
    return {'settings': {'seam_qc_radius': radius, 'seam_qc_min_pixels': min_pixels, 'seam_qc_min_ncc': min_ncc,
                         'describes': 'every pair of overlapping tiles of every staged plane as the fusion reads it: after dpc, '
                                      'despeckle and background removal, before the flatfield divide; mean_ref, mean_mov and mad '
                                      'are raw counts; a seam that agrees best at (best_dy, best_dx) is displaced by '
                                      '(dy + best_dy, dx + best_dx)'},
            'rows': len(rows), 'flag_counts': counts, 'flagged': flagged, 'median_ncc': median_ncc, 'best_histogram': best_hist}


def _put(path: str, text: str) -> None:
    tmp = f"{path}.{os.getpid()}.tmp"
    with open(tmp, 'w') as fh:
        fh.write(text)
    os.replace(tmp, path)


def write_report(folder: str, region, rows: List[dict], channels: Sequence[str], radius: int, min_pixels: int,
                 min_ncc: float) -> dict:
    """``<region>_stitched_seam_qc.csv`` and ``.json`` under ``folder``, each put in place atomically; returns the summary."""
    os.makedirs(folder, exist_ok=True)
    note = summary(rows, channels, radius, min_pixels, min_ncc)
    _put(os.path.join(folder, f"{region}_stitched_seam_qc.csv"), csv_text(rows))
    _put(os.path.join(folder, f"{region}_stitched_seam_qc.json"), json.dumps(note, indent=1) + '\n')
    return note
