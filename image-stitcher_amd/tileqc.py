"""--tile-qc: the per-tile quality table derived from the eight words sq_tile_stats writes for every staged tile plane
(include/squidstitch.h; an extension, the reference has none).  Host only: Python integers and true division, so that every
float is the correctly rounded quotient of exact integers and a second implementation (tests/tile_qc_ref.py) agrees bit for bit.

With n = h * w, nx = h * max(w - 2, 0), ny = max(h - 2, 0) * w and the words min, max, S, Q, top, zeros, Bx, By of a plane:

    mean               = S / n
    std                = sqrt((n * Q - S * S) / (n * n))
    brenner            = (Bx + By) / (nx + ny)            0.0 when nx + ny == 0
    focus              = brenner / mean^2                 the exposure-independent form, as ONE quotient of integers:
                         (Bx + By) * n * n / ((nx + ny) * S * S); 0.0 when S == 0 or nx + ny == 0
    saturated_fraction = top / n

and, over the rows of one (timepoint, region): best_z of a (fov, channel) is the z of its largest focus (the lowest z wins a
tie); the flags, joined with '|' in this order, are 'saturated' (saturated_fraction > saturation), 'constant' (min == max)
and 'low_focus' (focus < focus_ratio * numpy.median(focus of the rows of the same (channel, z)), only where those rows number
at least three, and never on a constant row)."""
from __future__ import annotations

import json
import math
import os
from typing import Dict, List, Sequence

import numpy as np

WORDS = 8
CSV_HEADER = ('region', 'fov', 'z_level', 'channel', 'pixels', 'min', 'max', 'mean', 'std', 'saturated', 'zeros', 'brenner_x',
              'brenner_y', 'focus', 'best_z', 'flags')
FLAGS = ('saturated', 'constant', 'low_focus')
MIN_ROWS_FOR_MEDIAN = 3


def _is_fraction(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and 0.0 <= float(v) <= 1.0


def check_options(tile_qc, saturation, focus_ratio):
    """The Stitcher's three arguments, validated: (bool, float in [0, 1], float in [0, 1]); ValueError otherwise."""
    if not isinstance(tile_qc, (bool, np.bool_)):
        raise ValueError(f"tile_qc must be a bool, got {tile_qc!r}")
    if not _is_fraction(saturation):
        raise ValueError(f"tile_qc_saturation must be a number in [0, 1], got {saturation!r}")
    if not _is_fraction(focus_ratio):
        raise ValueError(f"tile_qc_focus_ratio must be a number in [0, 1], got {focus_ratio!r}")
    return bool(tile_qc), float(saturation), float(focus_ratio)


def derive(words: Sequence[int], h: int, w: int) -> Dict[str, float]:
    """mean, std, brenner, focus and saturated_fraction of one plane from its eight words."""
    mn, mx, s, q, top, zeros, bx, by = (int(v) for v in words)
    h, w = int(h), int(w)
    n = h * w
    nd = h * max(w - 2, 0) + max(h - 2, 0) * w
    b = bx + by
    return {'mean': s / n,
            'std': math.sqrt((n * q - s * s) / (n * n)),
            'brenner': b / nd if nd else 0.0,
            'focus': (b * n * n) / (nd * s * s) if (nd and s) else 0.0,
            'saturated_fraction': top / n}


def make_row(region, fov: int, z_level: int, channel: str, words: Sequence[int], h: int, w: int) -> dict:
    """One row of the table (best_z and flags are filled in by flag_rows); 'saturated_fraction' rides along for the flags."""
    mn, mx, s, q, top, zeros, bx, by = (int(v) for v in words)
    d = derive(words, h, w)
    return {'region': region, 'fov': int(fov), 'z_level': int(z_level), 'channel': channel, 'pixels': int(h) * int(w), 'min': mn,
            'max': mx, 'mean': d['mean'], 'std': d['std'], 'saturated': top, 'zeros': zeros, 'brenner_x': bx, 'brenner_y': by,
            'focus': d['focus'], 'best_z': -1, 'flags': '', 'saturated_fraction': d['saturated_fraction']}


def flag_rows(rows: List[dict], saturation: float, focus_ratio: float) -> List[dict]:
    """Fill 'best_z' and 'flags' of the rows of one (timepoint, region) in place; returns them."""
    best: Dict[tuple, tuple] = {}
    planes: Dict[tuple, List[float]] = {}
    for r in rows:
        k = (r['fov'], r['channel'])
        if k not in best or r['focus'] > best[k][0] or (r['focus'] == best[k][0] and r['z_level'] < best[k][1]):
            best[k] = (r['focus'], r['z_level'])
        planes.setdefault((r['channel'], r['z_level']), []).append(r['focus'])
    medians = {k: float(np.median(np.array(v, dtype=np.float64))) for k, v in planes.items() if len(v) >= MIN_ROWS_FOR_MEDIAN}
    for r in rows:
        r['best_z'] = best[(r['fov'], r['channel'])][1]
        flags = []
        if r['saturated_fraction'] > saturation:
            flags.append('saturated')
        constant = r['min'] == r['max']
        if constant:
            flags.append('constant')
        med = medians.get((r['channel'], r['z_level']))
        if med is not None and not constant and r['focus'] < focus_ratio * med:
            flags.append('low_focus')
        r['flags'] = '|'.join(flags)
    return rows


def _cell(v) -> str:
    return repr(float(v)) if isinstance(v, (float, np.floating)) else str(v)


def csv_text(rows: List[dict]) -> str:
    """The CSV: integers as integers, floats with repr."""
    lines = [','.join(CSV_HEADER)]
    for r in rows:
        lines.append(','.join(_cell(r[k]) for k in CSV_HEADER))
    return '\n'.join(lines) + '\n'


def summary(rows: List[dict], channels: Sequence[str], saturation: float, focus_ratio: float) -> dict:
    """What the JSON beside the CSV says: the settings, the row count, per channel the median focus per z and a histogram of
    best_z (one count per fov), the count of each flag and the flagged rows."""
    median_focus: Dict[str, Dict[str, float]] = {}
    best_hist: Dict[str, Dict[str, int]] = {}
    for name in channels:
        of = [r for r in rows if r['channel'] == name]
        if not of:
            continue
        zs = sorted({r['z_level'] for r in of})
        median_focus[name] = {str(z): float(np.median(np.array([r['focus'] for r in of if r['z_level'] == z], dtype=np.float64)))
                              for z in zs}
        per_fov = {r['fov']: r['best_z'] for r in of}
        best_hist[name] = {str(z): sum(1 for b in per_fov.values() if b == z) for z in zs}
    counts = {f: sum(1 for r in rows if f in r['flags'].split('|')) for f in FLAGS}
    flagged = [{'fov': r['fov'], 'z_level': r['z_level'], 'channel': r['channel'], 'flags': r['flags']} for r in rows if r['flags']]
    return {'settings': {'tile_qc_saturation': saturation, 'tile_qc_focus_ratio': focus_ratio, 'brenner_step': 2,
                         'min_rows_for_median': MIN_ROWS_FOR_MEDIAN,
                         'describes': 'every tile plane as it is in its file, before despeckle, background removal and the '
                                      'flatfield divide'},
            'rows': len(rows), 'median_focus': median_focus, 'flag_counts': counts, 'flagged': flagged,
            'best_z_histogram': best_hist}


def _put(path: str, text: str) -> None:
    tmp = f"{path}.{os.getpid()}.tmp"
    with open(tmp, 'w') as fh:
        fh.write(text)
    os.replace(tmp, path)


def write_report(folder: str, region, rows: List[dict], channels: Sequence[str], saturation: float, focus_ratio: float) -> dict:
    """``<region>_stitched_tile_qc.csv`` and ``.json`` under ``folder``, each put in place atomically; returns the summary."""
    os.makedirs(folder, exist_ok=True)
    note = summary(rows, channels, saturation, focus_ratio)
    _put(os.path.join(folder, f"{region}_stitched_tile_qc.csv"), csv_text(rows))
    _put(os.path.join(folder, f"{region}_stitched_tile_qc.json"), json.dumps(note, indent=1) + '\n')
    return note
