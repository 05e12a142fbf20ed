"""The numpy definition of the eight words sq_tile_stats writes per plane (include/squidstitch.h), and an independent restatement
of what image_stitcher_amd/tileqc.py derives from them.  Not a test module."""
import math
from fractions import Fraction

import numpy as np

HEADER = ('region,fov,z_level,channel,pixels,min,max,mean,std,saturated,zeros,brenner_x,brenner_y,focus,best_z,flags')


def tile_words(plane):
    """[min, max, S, Q, pixels at the dtype's maximum, pixels at 0, Bx, By] of one [h, w] uint8 / uint16 plane, as Python
    integers, from an int64 copy of it."""
    top = int(np.iinfo(plane.dtype).max)
    a = np.asarray(plane).astype(np.int64)
    assert a.ndim == 2 and a.size > 0
    dx = a[:, 2:] - a[:, :-2]
    dy = a[2:, :] - a[:-2, :]
    return [int(a.min()), int(a.max()), int(a.sum()), int((a * a).sum()), int((a == top).sum()), int((a == 0).sum()),
            int((dx * dx).sum()), int((dy * dy).sum())]


def words_of(planes):
    """[n, 8] int64 of a [n, h, w] stack."""
    return np.array([tile_words(p) for p in planes], dtype=np.int64).reshape(len(planes), 8)


def _rounded(fr):
    return float(fr)      # Fraction -> float is the correctly rounded quotient


def derive(words, h, w):
    """(mean, std, brenner, focus, saturated_fraction): every quotient taken exactly and rounded once."""
    mn, mx, s, q, top, zeros, bx, by = (int(v) for v in words)
    n = h * w
    nd = h * max(w - 2, 0) + max(h - 2, 0) * w
    mean = _rounded(Fraction(s, n))
    std = math.sqrt(_rounded(Fraction(n * q - s * s, n * n)))
    brenner = _rounded(Fraction(bx + by, nd)) if nd else 0.0
    focus = _rounded(Fraction((bx + by) * n * n, nd * s * s)) if (nd and s) else 0.0
    return mean, std, brenner, focus, _rounded(Fraction(top, n))


def flag_rows(rows, saturation, focus_ratio):
    """rows: dicts with fov, z_level, channel, min, max, focus, saturated_fraction -> [(best_z, flags)] in the rows' order."""
    out = []
    for r in rows:
        same = [o for o in rows if o['fov'] == r['fov'] and o['channel'] == r['channel']]
        top = max(o['focus'] for o in same)
        best_z = min(o['z_level'] for o in same if o['focus'] == top)
        plane = np.array([o['focus'] for o in rows if o['channel'] == r['channel'] and o['z_level'] == r['z_level']])
        flags = []
        if r['saturated_fraction'] > saturation:
            flags.append('saturated')
        if r['min'] == r['max']:
            flags.append('constant')
        elif len(plane) >= 3 and r['focus'] < focus_ratio * float(np.median(plane)):
            flags.append('low_focus')
        out.append((best_z, '|'.join(flags)))
    return out


def table_of(entries, channel_order, h, w, saturation=0.01, focus_ratio=0.5, region='R0'):
    """The CSV's rows (lists of strings, the header first) from entries [(fov, z_level, channel, plane)], sorted by (channel
    order, z, fov)."""
    entries = sorted(entries, key=lambda e: (channel_order.index(e[2]), e[1], e[0]))
    rows = []
    for fov, z, channel, plane in entries:
        wd = tile_words(plane)
        mean, std, _, focus, sat = derive(wd, h, w)
        rows.append(dict(fov=fov, z_level=z, channel=channel, min=wd[0], max=wd[1], focus=focus, saturated_fraction=sat, words=wd,
                         mean=mean, std=std))
    flagged = flag_rows(rows, saturation, focus_ratio)
    lines = [HEADER.split(',')]
    for r, (best_z, flags) in zip(rows, flagged):
        wd = r['words']
        lines.append([region, str(r['fov']), str(r['z_level']), r['channel'], str(h * w), str(wd[0]), str(wd[1]), repr(r['mean']),
                      repr(r['std']), str(wd[4]), str(wd[5]), str(wd[6]), str(wd[7]), repr(r['focus']), str(best_z), flags])
    return lines


def box3(img):
    """The edge-replicated 3 x 3 box mean of a plane, in its dtype (truncated): a defocused version of it."""
    p = np.pad(img.astype(np.int64), 1, mode='edge')
    h, w = img.shape
    acc = sum(p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))
    return (acc // 9).astype(img.dtype)
