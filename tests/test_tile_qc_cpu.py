"""--tile-qc without a device: the numpy definition of the eight words (tests/tile_qc_ref.py) against a per-pixel loop, the
derived table (image_stitcher_amd/tileqc.py) against exact rational arithmetic and against the reference's restatement, the flag
rules, the fixture the GPU tests run on, and the declarations."""
import dataclasses
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import tile_qc_ref as R
from image_stitcher_amd import native, stitcher_cli, synth, tileqc
from image_stitcher_amd.stitcher import Stitcher
from image_stitcher_amd.stitcher_parameters import StitchingParameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIXTURE = synth.GridSpec(rows=3, cols=4, tile_h=64, tile_w=96, ov_y=8, ov_x=12, nz=3, channels=tuple(synth.DEFAULT_CHANNELS[:2]),
                         seed=5, blank_fovs=(7,))


def _loop_words(plane):
    top = int(np.iinfo(plane.dtype).max)
    h, w = plane.shape
    mn, mx, s, q, sat, zero, bx, by = None, None, 0, 0, 0, 0, 0, 0
    for y in range(h):
        for x in range(w):
            v = int(plane[y, x])
            mn = v if mn is None else min(mn, v)
            mx = v if mx is None else max(mx, v)
            s += v
            q += v * v
            sat += v == top
            zero += v == 0
            if x + 2 < w:
                bx += (int(plane[y, x + 2]) - v) ** 2
            if y + 2 < h:
                by += (int(plane[y + 2, x]) - v) ** 2
    return [mn, mx, s, q, sat, zero, bx, by]


@pytest.mark.parametrize('dtype', ['uint8', 'uint16'])
@pytest.mark.parametrize('shape', [(1, 1), (1, 5), (5, 1), (2, 2), (3, 3), (7, 9)])
def test_reference_words_against_a_pixel_loop(shape, dtype):
    top = int(np.iinfo(np.dtype(dtype)).max)
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    planes = [rng.integers(0, top + 1, shape).astype(dtype), np.zeros(shape, dtype), np.full(shape, top, dtype)]
    sparse = rng.integers(0, 4, shape)
    planes.append(np.where(sparse == 0, 0, np.where(sparse == 1, top, 7)).astype(dtype))
    for plane in planes:
        assert R.tile_words(plane) == _loop_words(plane)
    if shape[1] <= 2:
        assert all(R.tile_words(p)[6] == 0 for p in planes)
    if shape[0] <= 2:
        assert all(R.tile_words(p)[7] == 0 for p in planes)
    np.testing.assert_array_equal(R.words_of(np.stack(planes)), np.array([_loop_words(p) for p in planes]))


def test_full_scale_plane_is_exact():
    h, w = 300, 257
    plane = np.full((h, w), 65535, np.uint16)
    words = R.tile_words(plane)
    assert words == [65535, 65535, 65535 * h * w, 65535 * 65535 * h * w, h * w, 0, 0, 0]
    for d in (R.derive(words, h, w), tuple(tileqc.derive(words, h, w)[k] for k in ('mean', 'std', 'brenner', 'focus',
                                                                                  'saturated_fraction'))):
        assert d == (65535.0, 0.0, 0.0, 0.0, 1.0)


def _exact(words, h, w):
    mn, mx, s, q, top, zeros, bx, by = words
    n, nd = h * w, h * max(w - 2, 0) + max(h - 2, 0) * w
    return (float(Fraction(s, n)), math.sqrt(float(Fraction(n * q - s * s, n * n))),
            float(Fraction(bx + by, nd)) if nd else 0.0,
            float(Fraction((bx + by) * n * n, nd * s * s)) if nd and s else 0.0, float(Fraction(top, n)))


def test_derive_against_exact_rationals():
    rng = np.random.default_rng(3)
    cases = [(np.zeros((4, 5), np.uint16)), np.full((1, 1), 9, np.uint8), np.full((2, 2), 255, np.uint8)]
    for shape in ((1, 2), (2, 1), (1, 3), (3, 1), (3, 3), (7, 9), (64, 96), (33, 1301)):
        for dtype in ('uint8', 'uint16'):
            cases.append(rng.integers(0, int(np.iinfo(np.dtype(dtype)).max) + 1, shape).astype(dtype))
    cases.append(((np.indices((300, 257)).sum(axis=0) % 2) * 65535).astype(np.uint16))      # the largest Bx, By and Q
    for plane in cases:
        h, w = plane.shape
        words = R.tile_words(plane)
        want = _exact(words, h, w)
        d = tileqc.derive(words, h, w)
        assert (d['mean'], d['std'], d['brenner'], d['focus'], d['saturated_fraction']) == want, plane.shape
        assert R.derive(words, h, w) == want
    d = tileqc.derive(R.tile_words(np.zeros((4, 5), np.uint16)), 4, 5)
    assert d['focus'] == 0.0 and d['mean'] == 0.0 and d['std'] == 0.0            # S == 0
    assert tileqc.derive(R.tile_words(np.full((2, 2), 7, np.uint8)), 2, 2)['brenner'] == 0.0      # nx + ny == 0


def _row(fov, z, channel, focus, mn=0, mx=10, sat=0.0):
    return {'region': 'R0', 'fov': fov, 'z_level': z, 'channel': channel, 'min': mn, 'max': mx, 'focus': focus,
            'saturated_fraction': sat, 'best_z': -1, 'flags': ''}


def _flags(rows, saturation=0.01, focus_ratio=0.5):
    want = R.flag_rows(rows, saturation, focus_ratio)
    got = tileqc.flag_rows([dict(r) for r in rows], saturation, focus_ratio)
    assert [(r['best_z'], r['flags']) for r in got] == want
    return want


def test_flag_rules():
    # best z: the largest focus, the lowest z on a tie
    rows = [_row(0, 0, 'a', 1.0), _row(0, 1, 'a', 3.0), _row(0, 2, 'a', 3.0), _row(1, 0, 'a', 2.0), _row(1, 1, 'a', 2.0),
            _row(1, 2, 'a', 1.0), _row(0, 0, 'b', 0.0), _row(0, 1, 'b', 0.0)]
    assert [b for b, _ in _flags(rows)] == [1, 1, 1, 0, 0, 0, 0, 0]
    # fewer than three rows of a (channel, z): never low_focus
    rows = [_row(0, 0, 'a', 10.0), _row(1, 0, 'a', 0.1)]
    assert [f for _, f in _flags(rows)] == ['', '']
    rows.append(_row(2, 0, 'a', 10.0))
    assert [f for _, f in _flags(rows)] == ['', 'low_focus', '']
    assert [f for _, f in _flags(rows, focus_ratio=0.0)] == ['', '', '']      # strict <
    # the median is over the rows of the same (channel, z) only
    other = [_row(f, 1, 'a', 100.0) for f in range(3)] + [_row(f, 0, 'b', 100.0) for f in range(3)]
    assert [f for _, f in _flags(rows + other)][:3] == ['', 'low_focus', '']
    # a constant row is never low_focus, and it takes part in the median
    rows = [_row(0, 0, 'a', 10.0), _row(1, 0, 'a', 0.0, mn=500, mx=500), _row(2, 0, 'a', 10.0), _row(3, 0, 'a', 4.0)]
    assert [f for _, f in _flags(rows)] == ['', 'constant', '', '']           # median 7: 4.0 is above 3.5
    # saturated: strictly above the fraction; joined in the order saturated | constant | low_focus
    rows = [_row(0, 0, 'a', 10.0, sat=0.01), _row(1, 0, 'a', 10.0, sat=0.0100001), _row(2, 0, 'a', 1.0, sat=0.5),
            _row(3, 0, 'a', 0.0, mn=65535, mx=65535, sat=1.0)]
    assert [f for _, f in _flags(rows)] == ['', 'saturated', 'saturated|low_focus', 'saturated|constant']
    assert [f for _, f in _flags(rows, saturation=1.0)] == ['', '', 'low_focus', 'constant']


def _entries(spec, edit=None):
    """[(fov, z, channel, plane)] of the files write_acquisition makes of ``spec`` (monochrome channels)."""
    out = []
    for r in range(spec.rows):
        for c in range(spec.cols):
            fov = spec.fov_index(r, c)
            for z in range(spec.nz):
                for ci, ch in enumerate(spec.channels):
                    img = spec.tile(r, c, 0, 0, z, ci)
                    if fov in spec.blank_fovs:
                        img = np.full_like(img, 500 % (int(np.iinfo(img.dtype).max) + 1))
                    if edit is not None:
                        img = edit(fov, z, ci, img)
                    out.append((fov, z, ch, img))
    return out


@pytest.mark.parametrize('dtype', ['uint16', 'uint8'])
def test_the_fixture_is_sound(dtype):
    """With the defaults exactly the rows of the blank fov 7 are flagged, as constant, and every other row is far from the 0.5
    threshold: within 0.9 ... 1.1 of its plane's median (the reference's own figures on this fixture: 0.92 ... 1.06).  One tile
    rewritten as its 3 x 3 box mean drops to about 0.19 of the median and is the only low_focus row; another given 2 % pixels
    at the dtype's maximum is the only saturated row."""
    spec = dataclasses.replace(FIXTURE, dtype=dtype)
    top = int(np.iinfo(np.dtype(dtype)).max)
    names = list(spec.channels)
    table = R.table_of(_entries(spec), names, spec.tile_h, spec.tile_w)
    head, rows = table[0], table[1:]
    assert ','.join(head) == R.HEADER and len(rows) == 12 * 3 * 2
    col = {k: i for i, k in enumerate(head)}
    assert [r[col['flags']] for r in rows if r[col['fov']] == '7'] == ['constant'] * 6
    assert all(r[col['flags']] == '' for r in rows if r[col['fov']] != '7')
    assert [(r[col['channel']], int(r[col['z_level']]), int(r[col['fov']])) for r in rows] == \
        [(ch, z, f) for ch in names for z in range(3) for f in range(12)]
    for ch in names:
        for z in range(3):
            plane = [float(r[col['focus']]) for r in rows if r[col['channel']] == ch and int(r[col['z_level']]) == z]
            ratios = np.delete(np.array(plane), 7) / np.median(plane)
            assert 0.9 < ratios.min() and ratios.max() < 1.1, (ch, z, ratios)

    def edit(fov, z, ci, img):
        if (fov, z, ci) == (5, 1, 0):
            return R.box3(img)
        if (fov, z, ci) == (2, 2, 1):
            img = img.copy()
            img.reshape(-1)[::50] = top      # 2 % of the pixels
        return img

    rows = R.table_of(_entries(spec, edit), names, spec.tile_h, spec.tile_w)[1:]
    flagged = {(int(r[col['fov']]), int(r[col['z_level']]), r[col['channel']]): r[col['flags']] for r in rows if r[col['flags']]}
    want = {(7, z, ch): 'constant' for z in range(3) for ch in names}
    want[(5, 1, names[0])] = 'low_focus'
    want[(2, 2, names[1])] = 'saturated'
    assert flagged == want
    plane = [float(r[col['focus']]) for r in rows if r[col['channel']] == names[0] and r[col['z_level']] == '1']
    assert 0.1 < plane[5] / np.median(plane) < 0.3
    # the best z of the defocused tile's (fov, channel) is no longer z = 1, and tileqc writes this very table
    got = []
    for fov, z, ch, img in sorted(_entries(spec, edit), key=lambda e: (names.index(e[2]), e[1], e[0])):
        got.append(tileqc.make_row('R0', fov, z, ch, R.tile_words(img), spec.tile_h, spec.tile_w))
    tileqc.flag_rows(got, 0.01, 0.5)
    text = tileqc.csv_text(got)
    assert text == '\n'.join(','.join(r) for r in [head] + rows) + '\n'
    assert all(r['best_z'] != 1 for r in got if (r['fov'], r['channel']) == (5, names[0]))
    note = tileqc.summary(got, names, 0.01, 0.5)
    assert note['rows'] == 72 and note['flag_counts'] == {'saturated': 1, 'constant': 6, 'low_focus': 1}
    assert len(note['flagged']) == 8 and set(note['median_focus']) == set(names) == set(note['best_z_histogram'])
    assert all(sum(h.values()) == 12 for h in note['best_z_histogram'].values())


def test_cli_parsing_and_defaults():
    a = stitcher_cli.parse_args(['-i', 'x'])
    assert a.tile_qc is False and a.tile_qc_saturation == 0.01 and a.tile_qc_focus_ratio == 0.5
    a = stitcher_cli.parse_args(['-i', 'x', '--tile-qc', '--tile-qc-saturation', '0.2', '--tile-qc-focus-ratio', '0.75'])
    assert a.tile_qc is True and a.tile_qc_saturation == 0.2 and a.tile_qc_focus_ratio == 0.75
    with pytest.raises(SystemExit):
        stitcher_cli.parse_args(['-i', 'x', '--tile-qc', 'yes'])
    with pytest.raises(SystemExit):
        stitcher_cli.parse_args(['-i', 'x', '--tile-qc-saturation', 'much'])
    doc = stitcher_cli.__doc__
    assert 'eighteen switches' in doc
    for flag in ('--tile-qc', '--tile-qc-saturation', '--tile-qc-focus-ratio'):
        assert '``' + flag + '``' in doc and any(names == (flag,) for names, _ in stitcher_cli.FLAGS)


def test_construction_refusals(tmp_path):
    spec = synth.GridSpec(rows=1, cols=1, tile_h=16, tile_w=16, ov_y=0, ov_x=0, seed=1)
    root = str(tmp_path / 'acq')
    synth.write_acquisition(spec, root)
    params = StitchingParameters(input_folder=root)
    for bad in (-0.01, 1.01, True, '0.5', None, float('nan')):
        with pytest.raises(ValueError, match='tile_qc_saturation'):
            Stitcher(params, tile_qc=True, tile_qc_saturation=bad)
        with pytest.raises(ValueError, match='tile_qc_focus_ratio'):
            Stitcher(params, tile_qc=True, tile_qc_focus_ratio=bad)
    with pytest.raises(ValueError, match='tile_qc_saturation'):
        Stitcher(params, tile_qc_saturation=2)                       # refused with or without the option
    for bad in (1, 0, 'yes', None):
        with pytest.raises(ValueError, match='tile_qc'):
            Stitcher(params, tile_qc=bad)
    st = Stitcher(params)
    assert (st.tile_qc, st.tile_qc_saturation, st.tile_qc_focus_ratio) == (False, 0.01, 0.5)
    assert st.tile_qc_table == {} and not st._tile_qc_pending
    st = Stitcher(params, tile_qc_saturation=0.3, tile_qc_focus_ratio=1)      # values without the option: accepted and unused
    assert (st.tile_qc, st.tile_qc_saturation, st.tile_qc_focus_ratio) == (False, 0.3, 1.0)
    st = Stitcher(params, tile_qc=True, tile_qc_saturation=0, tile_qc_focus_ratio=np.float32(0.25))
    assert (st.tile_qc, st.tile_qc_saturation, st.tile_qc_focus_ratio) == (True, 0.0, 0.25)


def test_entry_point_is_declared():
    header = open(os.path.join(ROOT, 'include', 'squidstitch.h')).read()
    assert re.search(r'int\s+sq_tile_stats\s*\(', header)
    assert re.search(r'#define\s+SQ_TILE_STATS_WORDS\s+8\b', header)
    rows = re.search(r'#define\s+SQ_TILE_STATS_ROWS_PER_THREAD\s+(\d+)\b', header)
    assert rows and int(rows.group(1)) == native.SQ_TILE_STATS_ROWS_PER_THREAD
    assert 'tests/tile_qc_ref.py' in header
    assert '#define SQ_VERSION 108' in header and native.SQ_VERSION == 108
    assert 'sq_tile_stats' in native.EXPORTS and len(native.EXPORTS['sq_tile_stats'][1]) == 9
    assert native.SQ_TILE_STATS_WORDS == 8 == tileqc.WORDS
    makefile = open(os.path.join(ROOT, 'image-stitcher_amd', 'csrc', 'Makefile')).read()
    assert 'tilestats.hip' in makefile
    source = open(os.path.join(ROOT, 'image-stitcher_amd', 'csrc', 'tilestats.hip')).read()
    assert 'tests/tile_qc_ref.py' in source and 'SQ_TILE_STATS_ROWS_PER_THREAD' in source
    if os.path.exists(native.LIB_PATH):
        L = native.lib()
        assert L.sq_version() == 108
        # host-side refusals need no device: nothing is launched
        assert L.sq_tile_stats(None, 0, 4, 4, 16, 4, native.SQ_U16, None, None) == 0            # no planes
        assert L.sq_tile_stats(None, 1, 4, 4, 16, 4, native.SQ_U16, None, None) == -1           # NULL
        assert L.sq_tile_stats(None, -1, 4, 4, 16, 4, native.SQ_U16, None, None) == -1
        assert L.sq_tile_stats(None, 1, 4, 4, 16, 3, native.SQ_U16, None, None) == -1           # pitch < w
        assert L.sq_tile_stats(None, 1, 4, 4, 16, 4, native.SQ_F32, None, None) == -1
        assert L.sq_tile_stats(None, 1, 65536, 32769, 1 << 40, 32769, native.SQ_U16, None, None) == -3      # h * w > 2^31
