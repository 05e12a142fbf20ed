"""--seam-qc without a device: the numpy definition of the words (tests/seam_qc_ref.py) against a per-pixel loop, the seam list
and the derived table (image_stitcher_amd/seamqc.py) against hand-made cases and against the reference's restatement, the flags
of the command line, and the declarations."""
import json
import math
import os
import re

import numpy as np
import pytest

import seam_qc_ref as R
from image_stitcher_amd import native, seamqc, stitcher_cli, synth
from image_stitcher_amd.stitcher import Stitcher
from image_stitcher_amd.stitcher_parameters import StitchingParameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _loop_words(ref, mov, window, radius):
    ry, rx, my, mx, hc, wc = window
    sa = saa = sad = 0
    for y in range(hc):
        for x in range(wc):
            a, b = int(ref[ry + y, rx + x]), int(mov[my + y, mx + x])
            sa, saa, sad = sa + a, saa + a * a, sad + abs(a - b)
    out = [sa, saa, sad]
    for ey in range(-radius, radius + 1):
        for ex in range(-radius, radius + 1):
            sb = sbb = sab = 0
            for y in range(hc):
                for x in range(wc):
                    a, b = int(ref[ry + y, rx + x]), int(mov[my + y - ey, mx + x - ex])
                    sb, sbb, sab = sb + b, sbb + b * b, sab + a * b
            out += [sb, sbb, sab]
    return out


@pytest.mark.parametrize('dtype', ['uint8', 'uint16'])
@pytest.mark.parametrize('radius', [0, 1, 3])
def test_reference_words_against_a_pixel_loop(radius, dtype):
    top = int(np.iinfo(np.dtype(dtype)).max)
    rng = np.random.default_rng(radius + 10)
    ref, mov = (rng.integers(0, top + 1, (12, 15)).astype(dtype) for _ in range(2))
    for window in ((3, 4, 3, 3, 5, 7), (0, 0, radius, radius, 1, 1), (11, 14, 12 - 1 - radius, 15 - 1 - radius, 1, 1),
                   (2, 0, radius, 15 - 6 - radius, 12 - 2 * radius - 2, 6)):
        got = R.pair_words(ref, mov, window, radius)
        assert got == _loop_words(ref, mov, window, radius) and len(got) == R.n_words(radius) == seamqc.n_words(radius)
    full = np.full((8, 8), top, dtype)
    w = R.pair_words(full, full, (1, 1, 1, 1, 6, 6), 1)
    assert w[:3] == [36 * top, 36 * top * top, 0] and w[3:] == [36 * top, 36 * top * top, 36 * top * top] * 9


def _full(oy, ox, h=20, w=30):
    return (0, 0, h, w, oy, ox)


def test_region_seams_of_a_two_by_two_grid_by_hand():
    rects = {0: _full(0, 0), 1: _full(0, 24), 2: _full(16, 0), 3: _full(16, 24)}
    seams = seamqc.region_seams(rects, 20, 30, 1, 8)
    got = [(s['ref_fov'], s['mov_fov'], s['dy'], s['dx'], s['kind'], s['pixels'], s['window']) for s in seams]
    assert got == [(0, 1, 0, 24, 'h', 72, (1, 25, 1, 1, 18, 4)),         # ho x wo = 20 x 6: side by side, 'h'
                   (0, 2, 16, 0, 'v', 56, (17, 1, 1, 1, 2, 28)),         # 4 x 30: one above the other, 'v'
                   (0, 3, 16, 24, 'v', 8, (17, 25, 1, 1, 2, 4)),         # a corner, 4 x 6
                   (1, 2, 16, -24, 'v', 8, (17, 1, 1, 25, 2, 4)),        # the other corner: a negative dx
                   (1, 3, 16, 0, 'v', 56, (17, 1, 1, 1, 2, 28)),
                   (2, 3, 0, 24, 'h', 72, (1, 25, 1, 1, 18, 4))]
    assert got == R.seams_of(rects, 20, 30, 1, 8)
    # the min_pixels cut drops the two corners
    assert [(s['ref_fov'], s['mov_fov']) for s in seamqc.region_seams(rects, 20, 30, 1, 9)] == [(0, 1), (0, 2), (1, 3), (2, 3)]
    # cropped, registered and row-band-clipped rectangles have the same origin: the same seams
    cropped = {f: (2, 3, 20 - 2, 30 - 3, r[4] + 2, r[5] + 3) for f, r in rects.items()}
    assert seamqc.region_seams(cropped, 20, 30, 1, 8) == seams
    # an overlap of 2R columns or fewer is no seam, nor is a gap
    assert seamqc.region_seams(rects, 20, 30, 3, 1) == [] == R.seams_of(rects, 20, 30, 3, 1)      # wo = 6, ho = 4
    assert [(s['ref_fov'], s['mov_fov']) for s in seamqc.region_seams(rects, 20, 30, 2, 1)] == [(0, 1), (2, 3)]    # hc = 0 elsewhere
    apart = {0: _full(0, 0), 1: _full(0, 30), 2: _full(0, 61)}
    assert seamqc.region_seams(apart, 20, 30, 0, 1) == []
    # the pair table names positions in the staged list
    table = seamqc.pair_table(seams[:2], {0: 3, 1: 0, 2: 1})
    assert table.dtype == np.int32 and table.tolist() == [[3, 0, 1, 25, 1, 1, 18, 4], [3, 1, 17, 1, 1, 1, 2, 28]]


def test_region_seams_against_brute_force_on_a_jittered_ragged_grid():
    rng = np.random.default_rng(3)
    rects = {}
    for r in range(5):
        for c in range(6):
            if (r, c) in ((1, 1), (3, 4)):
                continue
            rects[r * 6 + c] = _full(100 + r * 17 + int(rng.integers(-3, 4)), 50 + c * 25 + int(rng.integers(-3, 4)))
    rects[40] = _full(-30, -40)      # a tile at negative coordinates, apart from the others
    for radius, min_pixels in ((0, 1), (2, 20), (3, 60)):
        seams = seamqc.region_seams(rects, 20, 30, radius, min_pixels)
        got = [(s['ref_fov'], s['mov_fov'], s['dy'], s['dx'], s['kind'], s['pixels'], s['window']) for s in seams]
        assert got == R.seams_of(rects, 20, 30, radius, min_pixels) and got


def _words(a, shifted, radius):
    """Words from a core vector ``a`` and {e: the vector b_e} (missing offsets: zeros)."""
    a = [int(v) for v in a]
    b0 = shifted.get((0, 0), [0] * len(a))
    out = [sum(a), sum(v * v for v in a), sum(abs(x - y) for x, y in zip(a, b0))]
    for ey in range(-radius, radius + 1):
        for ex in range(-radius, radius + 1):
            b = shifted.get((ey, ex), [0] * len(a))
            out += [sum(b), sum(v * v for v in b), sum(x * y for x, y in zip(a, b))]
    return out


def test_derive_breaks_ties_exactly():
    a = [0, 5, 2, 9]
    worse = [1, 5, 2, 7]
    d = seamqc.derive(_words(a, {(0, 0): worse, (1, 0): a, (0, 1): a, (0, -1): a, (-1, 0): a, (-1, -1): a}, 1), 4, 1)
    assert (d['best_dy'], d['best_dx'], d['best_ncc']) == (-1, 0, 1.0) and d['ncc'] < 1.0      # ey^2 + ex^2, then the smaller ey
    d = seamqc.derive(_words(a, {(0, 0): worse, (0, 1): a, (0, -1): a, (1, 1): a}, 1), 4, 1)
    assert (d['best_dy'], d['best_dx']) == (0, -1)                                              # then the smaller ex
    d = seamqc.derive(_words(a, {(0, 0): a, (-1, 0): a, (0, -1): a}, 1), 4, 1)
    assert (d['best_dy'], d['best_dx'], d['ncc'], d['mad']) == (0, 0, 1.0, 0.0)                 # the placement wins a tie
    d = seamqc.derive(_words(a, {(0, 0): worse, (2, -2): [2 * v + 3 for v in a]}, 2), 4, 2)    # gain and offset do not matter
    assert (d['best_dy'], d['best_dx'], d['best_ncc']) == (2, -2, 1.0)
    assert (d['mean_ref'], d['mean_mov'], d['mad']) == (4.0, 3.75, 0.75)
    # every column agrees with the reference's restatement
    for words, n, radius in ((_words(a, {(0, 0): worse, (1, 0): a, (-1, 0): a}, 1), 4, 1), (_words(a, {(0, 0): worse}, 0), 4, 0)):
        d, want = seamqc.derive(words, n, radius), R.derive(words, n, radius)
        assert (d['mean_ref'], d['mean_mov'], d['mad'], d['ncc']) == want[:4]
        assert (d['best_dy'], d['best_dx'], d['best_ncc']) == want[4]
    with pytest.raises(ValueError):
        seamqc.derive([0] * 30, 4, 0)


def test_derive_compares_integers_where_the_floats_are_equal():
    """n = 1, Sa = 0, Saa = 1 (va = 1) and Sb = 0 make vb_e = Sbb_e and num_e = Sab_e free to choose.  With K = 2^40:
    e1 = (0, 1) has num = K, vb = 4 K^2: ncc = 1/2 exactly.  e2 = (0, -1) has num = K + 1, vb = 4 (K + 1)^2 + 1: ncc is below
    1/2 by a part in 2^83, and its float is 0.5 too.  e2 comes first in the scan and ties on ey^2 + ex^2, so an order taken
    from the floats picks it; the integers pick e1."""
    k = 2 ** 40
    words = [0, 1, 0]
    for e in [(ey, ex) for ey in (-1, 0, 1) for ex in (-1, 0, 1)]:
        words += {(0, 1): [0, 4 * k * k, k], (0, -1): [0, 4 * (k + 1) ** 2 + 1, k + 1]}.get(e, [0, 1, 0])
    f1, f2 = k / math.sqrt(1 * 4 * k * k), (k + 1) / math.sqrt(1 * (4 * (k + 1) ** 2 + 1))
    assert f1 == f2 == 0.5
    d = seamqc.derive(words, 1, 1)
    assert (d['best_dy'], d['best_dx'], d['best_ncc'], d['ncc']) == (0, 1, 0.5, 0.0)
    assert R.derive(words, 1, 1)[4] == (0, 1, 0.5)
    # and the other way round when the exact order is the other way
    words[3 + 3 * 5:3 + 3 * 6] = [0, 4 * k * k + 1, k]
    words[3 + 3 * 3:3 + 3 * 4] = [0, 4 * (k + 1) ** 2, k + 1]
    d = seamqc.derive(words, 1, 1)
    assert (d['best_dy'], d['best_dx']) == (0, -1) == R.derive(words, 1, 1)[4][:2]


def test_derive_featureless_on_zero_variance():
    a, flat = [0, 5, 2, 9], [7, 7, 7, 7]
    for words in (_words(flat, {(0, 0): a, (0, 1): a}, 1), _words(a, {(0, 0): flat, (0, 1): a}, 1)):
        d = seamqc.derive(words, 4, 1)
        assert d['featureless'] and d['ncc'] is None and d['best_dy'] is None and d['best_dx'] is None and d['best_ncc'] is None
        assert R.derive(words, 4, 1)[3:] == (None, None)
    # an offset whose window is constant is skipped, the pair is not featureless
    d = seamqc.derive(_words(a, {(0, 0): [1, 5, 2, 7], (0, -1): flat, (1, 1): a}, 1), 4, 1)
    assert not d['featureless'] and (d['best_dy'], d['best_dx']) == (1, 1)


def _rows():
    a, worse = [0, 5, 2, 9], [1, 5, 2, 7]
    seams = seamqc.region_seams({0: _full(0, 0), 1: _full(0, 24), 2: _full(16, 0)}, 20, 30, 1, 8)
    assert [(s['ref_fov'], s['mov_fov']) for s in seams] == [(0, 1), (0, 2), (1, 2)]
    for s in seams:
        s['pixels'] = 4      # (the constructed words are those of four pixels)
    cases = [('A', 0, seams[0], _words(a, {(0, 0): a}, 1)),
             ('A', 0, seams[1], _words(a, {(0, 0): worse, (1, 0): a}, 1)),
             ('A', 1, seams[0], _words(a, {(0, 0): [9, 2, 5, 0], (0, 1): [9, 2, 5, 1]}, 1)),
             ('B', 0, seams[1], _words(a, {(0, 0): [3, 3, 3, 3]}, 1)),
             ('B', 0, seams[2], None)]
    rows = [seamqc.make_row('R0', channel, z, seam, words, 1) for channel, z, seam, words in cases]
    return seamqc.flag_rows(rows, 0.5), cases


def test_csv_and_json_round_trip(tmp_path):
    rows, cases = _rows()
    assert [r['flags'] for r in rows] == ['', 'shifted', 'low_ncc|shifted', 'featureless', 'unmeasured']
    text = seamqc.csv_text(rows)
    lines = [line.split(',') for line in text.splitlines()]
    assert text.endswith('\n') and lines[0] == list(seamqc.CSV_HEADER) == R.HEADER.split(',') and len(lines) == 6
    col = {k: i for i, k in enumerate(lines[0])}
    for line, row in zip(lines[1:], rows):
        for k in ('z_level', 'ref_fov', 'mov_fov', 'dy', 'dx', 'pixels', 'best_dy', 'best_dx'):      # integers as integers
            assert line[col[k]] == ('' if row[k] is None else str(int(row[k])))
        for k in ('mean_ref', 'mean_mov', 'mad', 'ncc', 'best_ncc'):                                # floats round-trip
            assert (line[col[k]] == '') if row[k] is None else (float(line[col[k]]) == row[k] and '.' in line[col[k]])
    assert lines[5][col['mean_ref']:] == ['', '', '', '', '', '', '', 'unmeasured']
    assert lines[4][col['ncc']:] == ['', '', '', '', 'featureless'] and lines[4][col['mean_mov']] == '3.0'
    # the reference's restatement writes the same cells
    for line, (channel, z, s, words) in zip(lines[1:], cases):
        seam = (s['ref_fov'], s['mov_fov'], s['dy'], s['dx'], s['kind'], s['pixels'], s['window'])
        assert line == R.row_of('R0', channel, z, seam, words, 1, 0.5)
    note = seamqc.write_report(str(tmp_path), 'R0', rows, ['A', 'B', 'C'], 1, 8, 0.5)
    assert sorted(os.listdir(tmp_path)) == ['R0_stitched_seam_qc.csv', 'R0_stitched_seam_qc.json']
    assert open(tmp_path / 'R0_stitched_seam_qc.csv').read() == text
    assert json.load(open(tmp_path / 'R0_stitched_seam_qc.json')) == note
    assert note['rows'] == 5 and note['flag_counts'] == {'unmeasured': 1, 'featureless': 1, 'low_ncc': 1, 'shifted': 2}
    assert note['settings']['seam_qc_radius'] == 1 and note['settings']['seam_qc_min_pixels'] == 8
    assert note['settings']['seam_qc_min_ncc'] == 0.5
    assert [f['flags'] for f in note['flagged']] == ['shifted', 'low_ncc|shifted', 'featureless', 'unmeasured']
    assert note['flagged'][0] == {'channel': 'A', 'z_level': 0, 'ref_fov': 0, 'mov_fov': 2, 'flags': 'shifted'}
    assert note['best_histogram'] == {'A': {'0,0': 1, '0,1': 1, '1,0': 1}, 'B': {}}
    assert note['median_ncc']['A'] == {'0': float(np.median([rows[0]['ncc'], rows[1]['ncc']])), '1': rows[2]['ncc']}
    assert note['median_ncc']['B'] == {'0': None}


def test_cli_parsing_and_defaults():
    a = stitcher_cli.parse_args(['-i', 'x'])
    assert (a.seam_qc, a.seam_qc_radius, a.seam_qc_min_pixels, a.seam_qc_min_ncc) == (False, 2, 256, 0.5)
    a = stitcher_cli.parse_args(['-i', 'x', '--seam-qc', '--seam-qc-radius', '3', '--seam-qc-min-pixels', '300', '--seam-qc-min-ncc',
                                 '-0.25'])
    assert (a.seam_qc, a.seam_qc_radius, a.seam_qc_min_pixels, a.seam_qc_min_ncc) == (True, 3, 300, -0.25)
    with pytest.raises(SystemExit):
        stitcher_cli.parse_args(['-i', 'x', '--seam-qc', 'yes'])
    with pytest.raises(SystemExit):
        stitcher_cli.parse_args(['-i', 'x', '--seam-qc-radius', '1.5'])
    doc = stitcher_cli.__doc__
    for flag in ('--seam-qc', '--seam-qc-radius', '--seam-qc-min-pixels', '--seam-qc-min-ncc'):
        assert '``' + flag + '``' in doc and any(names == (flag,) for names, _ in stitcher_cli.FLAGS)
    assert 'raw counts' in dict((names[0], kw['help']) for names, kw in stitcher_cli.FLAGS)['--seam-qc']


def test_construction_refusals(tmp_path):
    spec = synth.GridSpec(rows=1, cols=1, tile_h=16, tile_w=16, ov_y=0, ov_x=0, seed=1)
    root = str(tmp_path / 'acq')
    synth.write_acquisition(spec, root)
    params = StitchingParameters(input_folder=root)
    for bad in (4, -1, 1.0, True, '2', None):
        with pytest.raises(ValueError, match='seam_qc_radius'):
            Stitcher(params, seam_qc=True, seam_qc_radius=bad)
    for bad in (-1, 0, 2.5, True, '256', None):
        with pytest.raises(ValueError, match='seam_qc_min_pixels'):
            Stitcher(params, seam_qc=True, seam_qc_min_pixels=bad)
    for bad in (-1.01, 1.01, True, '0.5', None, float('nan')):
        with pytest.raises(ValueError, match='seam_qc_min_ncc'):
            Stitcher(params, seam_qc=True, seam_qc_min_ncc=bad)
    with pytest.raises(ValueError, match='seam_qc_radius'):
        Stitcher(params, seam_qc_radius=4)                           # refused with or without the option
    for bad in (1, 0, 'yes', None):
        with pytest.raises(ValueError, match='seam_qc'):
            Stitcher(params, seam_qc=bad)
    st = Stitcher(params)
    assert (st.seam_qc, st.seam_qc_radius, st.seam_qc_min_pixels, st.seam_qc_min_ncc) == (False, 2, 256, 0.5)
    assert st.seam_qc_table == {} and not st._seam_qc_pending and st._seam_qc_words == {}
    st = Stitcher(params, seam_qc=True, seam_qc_radius=np.int32(0), seam_qc_min_pixels=1, seam_qc_min_ncc=-1)
    assert (st.seam_qc, st.seam_qc_radius, st.seam_qc_min_pixels, st.seam_qc_min_ncc) == (True, 0, 1, -1.0)


def test_entry_point_is_declared():
    header = open(os.path.join(ROOT, 'include', 'squidstitch.h')).read()
    assert re.search(r'int\s+sq_seam_stats\s*\(', header)
    assert re.search(r'#define\s+SQ_SEAM_MAX_RADIUS\s+3\b', header) and native.SQ_SEAM_MAX_RADIUS == 3 == seamqc.MAX_RADIUS
    assert 'tests/seam_qc_ref.py' in header
    assert '#define SQ_VERSION 108' in header and native.SQ_VERSION == 108
    assert 'sq_seam_stats' in native.EXPORTS and len(native.EXPORTS['sq_seam_stats'][1]) == 15
    assert [native.seam_words(r) for r in range(4)] == [6, 30, 78, 150] == [seamqc.n_words(r) for r in range(4)]
    with pytest.raises(ValueError):
        native.seam_words(4)
    makefile = open(os.path.join(ROOT, 'image-stitcher_amd', 'csrc', 'Makefile')).read()
    assert 'seam.hip' in makefile
    source = open(os.path.join(ROOT, 'image-stitcher_amd', 'csrc', 'seam.hip')).read()
    assert 'tests/seam_qc_ref.py' in source and 'SQ_SEAM_MAX_RADIUS' in source
    if os.path.exists(native.LIB_PATH):
        L = native.lib()
        assert L.sq_version() == 108
        # host-side refusals need no device: nothing is launched
        pairs = native.as_overlaps(np.array([[0, 1, 3, 3, 3, 3, 2, 2]]))

        def call(tiles=8, n_planes=1, n_tiles=2, h=8, w=8, ps=128, ts=64, pitch=8, dtype=native.SQ_U16, host=pairs.ctypes.data,
                 dev=8, n_pairs=1, radius=3, out=8):
            return L.sq_seam_stats(tiles, n_planes, n_tiles, h, w, ps, ts, pitch, dtype, host, dev, n_pairs, radius, out, None)

        assert call(n_pairs=0) == 0 and call(n_planes=0) == 0 and call(n_pairs=0, tiles=None, host=None, dev=None, out=None) == 0
        for bad in (dict(tiles=None), dict(host=None), dict(dev=None), dict(out=None), dict(radius=4), dict(radius=-1),
                    dict(pitch=7), dict(dtype=native.SQ_F32), dict(n_planes=-1), dict(n_pairs=-1), dict(h=0), dict(ts=10),
                    dict(n_planes=2, ps=100), dict(n_tiles=1), dict(tiles=9), dict(out=12)):
            assert call(**bad) == -1, bad
        for rec in ([0, 2, 3, 3, 3, 3, 2, 2], [-1, 1, 3, 3, 3, 3, 2, 2], [0, 1, 3, 3, 2, 3, 2, 2], [0, 1, 3, 3, 3, 3, 3, 2],
                    [0, 1, 7, 3, 3, 3, 2, 2], [0, 1, 3, 3, 3, 3, -1, 2]):
            bad = native.as_overlaps(np.array([rec]))
            assert call(host=bad.ctypes.data) == -1, rec
        big = native.as_overlaps(np.array([[0, 1, 0, 0, 3, 3, 65536, 32769]]))
        assert call(h=65536 + 6, w=32769 + 6, pitch=32769 + 6, ts=1 << 40, ps=1 << 42, host=big.ctypes.data) == -3      # > 2^31 pixels
