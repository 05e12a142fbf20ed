"""--channel-affine without a device: the definition three ways (tests/affine_ref.py's loop and vectorised form,
image-stitcher_amd/channelaffine.py), A = 0 against the channel shift's definition, the kernel's way to the same map and taps, the
64-bit bound, the option check and the command line, and the chain's buffers and bytes."""
import itertools
import os
import re

import numpy as np
import pytest

import affine_cases
import affine_ref
import shift_cases
import shift_ref
from image_stitcher_amd import channelaffine, native, stitcher_cli
from image_stitcher_amd.stitcher import Stitcher
from image_stitcher_amd.stitcher_parameters import StitchingParameters
from image_stitcher_amd.tilechain import BUFFERS, TileChain, warp_and_bin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize('dtype', affine_cases.DTYPES)
def test_loop_vectorised_and_module_agree(dtype):
    changed = {name: 0 for name in affine_cases.PLANE_NAMES}
    for (h, w), (s, a) in itertools.product(affine_cases.SMALL, affine_cases.PARAMS):
        planes = affine_cases.planes(dtype, h, w)
        want = affine_cases.reference(dtype, h, w, s, a)
        for i, name in enumerate(affine_cases.PLANE_NAMES):
            if name in ('noise', 'gradient') and h * w <= 2000:      # (the Python loop: the planes whose values differ everywhere)
                np.testing.assert_array_equal(affine_ref.loop(planes[i], s, a), want[i], err_msg=f'{(h, w)} {s} {a} {name}')
            np.testing.assert_array_equal(channelaffine.affine_image(planes[i], s, a), want[i], err_msg=f'{(h, w)} {s} {a} {name}')
            changed[name] += int((want[i] != planes[i]).any())
        if (s, a) == ((0, 0), affine_cases.ZERO) or (h, w) == (1, 1):
            np.testing.assert_array_equal(want, planes)
    # the sets change the planes with structure and leave the constant ones as they are
    assert changed['noise'] and changed['gradient'] and changed['checkerboard'] and not changed['maximum'] and not changed['zero']


def test_the_loop_on_one_larger_plane():
    h, w = 71, 143
    for s, a in (affine_cases.PARAMS[3], affine_cases.PARAMS[-1]):
        np.testing.assert_array_equal(affine_ref.loop(affine_cases.planes('uint16', h, w)[0], s, a),
                                      affine_cases.reference('uint16', h, w, s, a)[0])


def test_the_clamp_is_active_and_inactive_on_each_border():
    """Between them the sets make the clamp act, and leave it alone, on each of the four borders of the first six shapes."""
    seen = set()
    for (h, w), (s, a) in itertools.product(affine_cases.SMALL, affine_cases.PARAMS):
        dv, du, _, _ = affine_ref.maps(h, w, s, a)
        ys, xs = 256 * np.arange(h)[:, None] + dv, 256 * np.arange(w)[None, :] + du
        for border, out, inside in (('top', (ys < 0)[0], (ys >= 0)[0]), ('bottom', (ys > 256 * (h - 1))[-1], (ys <= 256 * (h - 1))[-1]),
                                    ('left', (xs < 0)[:, 0], (xs >= 0)[:, 0]), ('right', (xs > 256 * (w - 1))[:, -1], (xs <= 256 * (w - 1))[:, -1])):
            if out.any():
                seen.add((border, 'active'))
            if inside.all():
                seen.add((border, 'inactive'))
    assert len(seen) == 8, sorted(seen)


@pytest.mark.parametrize('dtype', shift_cases.DTYPES)
def test_zero_coefficients_are_the_channel_shift(dtype):
    for (h, w), shift in itertools.product(shift_cases.shapes(dtype), shift_cases.SHIFTS):
        planes = shift_cases.planes(dtype, h, w)
        want = shift_cases.reference(dtype, h, w, shift)
        np.testing.assert_array_equal(affine_ref.affine_image(planes, shift, affine_cases.ZERO), want, err_msg=f'{(h, w)} {shift}')
        np.testing.assert_array_equal(channelaffine.affine_image(planes[0], shift, affine_cases.ZERO), want[0])
    np.testing.assert_array_equal(affine_ref.loop(shift_cases.planes(dtype, 37, 53)[0], shift_cases.MIXED, affine_cases.ZERO),
                                  shift_ref.loop(shift_cases.planes(dtype, 37, 53)[0], *shift_cases.MIXED))


def test_the_numerator_fits_int64_and_the_displacement_int32():
    side, top = 65535, affine_ref.MAX_PPM
    largest = 16 * (top * (side - 1) + top * (side - 1)) + 62500
    assert largest == 104854462500 and 1.04e11 < largest < 1.05e11 < 2 ** 63
    # the vectorised form at the corners of the largest plane equals Python integers, which cannot overflow
    for a in ((top,) * 4, (-top,) * 4, (top, -top, -top, top)):
        for y, x in ((0, 0), (0, side - 1), (side - 1, 0), (side - 1, side - 1)):
            v, u = 2 * y - (side - 1), 2 * x - (side - 1)
            want = ((16 * (a[0] * v + a[1] * u) + 62500) // 125000, (16 * (a[2] * v + a[3] * u) + 62500) // 125000)
            got = (affine_ref._floor_div(np.array([16 * (np.int64(a[0]) * v + np.int64(a[1]) * u) + 62500]), 125000)[0],
                   affine_ref._floor_div(np.array([16 * (np.int64(a[2]) * v + np.int64(a[3]) * u) + 62500]), 125000)[0])
            assert (int(got[0]), int(got[1])) == want
            assert all(abs(256 * (side - 1) + 16384 + q) < 2 ** 31 for q in want)
    assert channelaffine.max_displacement(side, side, (16384, 16384), (top,) * 4) == (16384 + largest // 125000,) * 2
    assert largest // 125000 == 838835
    # floor division of negative numerators: rounded half up
    assert affine_ref._floor_div(np.array([-1, -125000, -125001, 0, 124999, 125000]), 125000).tolist() == [-1, -1, -2, 0, 0, 1]


@pytest.mark.parametrize('dtype', affine_cases.DTYPES)
def test_the_kernels_form_equals_the_definition(dtype):
    """What csrc/affine.hip computes: quotient and remainder of a vector's first column stepped along the row, the fast path's
    taps out of a span of VEC + 2 columns of two or three rows, the slow path's at clamped indices; every element written once.
    Both paths are taken."""
    vec = affine_cases.VEC[dtype]
    fast = slow = 0
    for (h, w), (s, a) in itertools.product(((1, 1), (2, 2), (5, vec), (5, vec + 1), (5, vec + 2), (9, 3 * vec + 2), (37, 53)), affine_cases.PARAMS):
        plane = affine_cases.planes(dtype, h, w)[0]
        for mis in (0, 3):
            got, f, sl = affine_ref.kernel_form(plane, s, a, vec, mis)
            np.testing.assert_array_equal(got, affine_cases.reference(dtype, h, w, s, a)[0], err_msg=f'{(h, w)} {s} {a} mis={mis}')
            fast, slow = fast + f, slow + sl
    assert fast > 100 and slow > 100
    # over a vector's columns the displacement changes by less than a pixel at the largest coefficient: two columns, two rows
    assert 32 * affine_ref.MAX_PPM * 15 // 125000 == 192 < 256


# ---------------------------------------------------------------------------------------------------- the option
def test_check_option(tmp_path):
    assert channelaffine.check_option(None) == {} and channelaffine.check_option({}) == {}
    got = channelaffine.check_option({'A': (1, -2, 3, -4), 'B': [0, 0, 0, 0], 'C': (50000, -50000, 0, 0)})
    assert got == {'A': (1, -2, 3, -4), 'C': (50000, -50000, 0, 0)} and type(got) is dict
    assert all(type(v) is int for a in got.values() for v in a)
    for bad in ({'A': (1.0, 2, 3, 4)}, {'A': (True, 2, 3, 4)}, {'A': ('1', 2, 3, 4)}, {'A': (1, 2, 3, 50001)}, {'A': (-50001, 0, 0, 0)},
                {'A': (1, 2, 3)}, {'A': (1, 2, 3, 4, 5)}, {'A': 5}, {'A': '1234'}, {'A': None}, {'A': (np.int64(3), 2, 3, 4)},
                {5: (1, 2, 3, 4)}, [('A', (1, 2, 3, 4))], 'A', 7):
        with pytest.raises(ValueError):
            channelaffine.check_option(bad)
    for bad in (dict(channel_affines={'A': (1.0, 2, 3, 4)}), dict(channel_affines={'A': (1, 2, 3, 50001)}), dict(channel_affines='A')):
        with pytest.raises(ValueError):
            Stitcher(StitchingParameters(input_folder=str(tmp_path)), **bad)
    st = Stitcher(StitchingParameters(input_folder=str(tmp_path)), channel_affines={'A': (0, 0, 0, 0)})
    assert st.channel_affines == {} and st._channel_affine_index == {}
    assert Stitcher(StitchingParameters(input_folder=str(tmp_path))).channel_affines == {}


def test_parse_ppm_and_command_line(tmp_path, capsys):
    for text, want in (('0', 0), ('-152', -152), ('+17452', 17452), ('50000', 50000), ('-50000', -50000), ('007', 7)):
        assert channelaffine.parse_ppm(text) == want
    for bad in ('50001', '-50001', '1.0', '1e3', '', ' 1', '1 ', '0x10', '1_0', '--1', 'one', None, 1, 0.5, '1/2'):
        with pytest.raises(ValueError):
            channelaffine.parse_ppm(bad)
    args = stitcher_cli.parse_args(['-i', 'x', '--channel-affine', 'Fluorescence 488 nm Ex', '-152', '17452', '-17452', '-152',
                                    '--channel-affine', 'B', '3000', '0', '0', '3000', '--channel-shift', 'B', '0.3', '-0.78125'])
    assert stitcher_cli.channel_affines_of(args.channel_affine) == {'Fluorescence 488 nm Ex': (-152, 17452, -17452, -152),
                                                                    'B': (3000, 0, 0, 3000)}
    assert stitcher_cli.channel_shifts_of(args.channel_shift) == {'B': (77, -200)}
    assert stitcher_cli.channel_affines_of(stitcher_cli.parse_args(['-i', 'x']).channel_affine) is None
    with pytest.raises(ValueError, match="'B'"):
        stitcher_cli.channel_affines_of([['B', '1', '1', '1', '1'], ['B', '2', '2', '2', '2']])
    for bad in (['B', '1.5', '1', '1', '1'], ['B', '1', '1', '1', '50001'], ['B', '1e1', '1', '1', '1']):
        with pytest.raises(ValueError):
            stitcher_cli.channel_affines_of([bad])
    with pytest.raises(SystemExit):
        stitcher_cli.parse_args(['-i', 'x', '--channel-affine', 'B', '1', '2', '3'])
    with pytest.raises(SystemExit):      # refused before anything is read
        stitcher_cli.main(['-i', str(tmp_path), '--channel-affine', 'B', '1', '2', '3', '4', '--channel-affine', 'B', '1', '2', '3', '4'])
    assert "'B' is given twice" in capsys.readouterr().err
    help_text = next(kw['help'] for names, kw in stitcher_cli.FLAGS if names == ('--channel-affine',))
    assert 'centre + (1 + A 1e-6) p' in help_text and 'parts per million' in help_text


def test_rgb_and_page_stacks():
    rgb = np.random.default_rng(5).integers(0, 256, (20, 30, 3)).astype(np.uint8)
    s = [(77, -200), (0, 0), (-256, 300)]
    a = [(2994, -3501, 3501, 2994), (0, 0, 0, 0), (0, 30000, 0, 0)]
    got = channelaffine.affine_image(rgb, s, a)
    np.testing.assert_array_equal(got, affine_ref.affine_file_image(rgb, s, a))
    np.testing.assert_array_equal(got[:, :, 1], rgb[:, :, 1])
    assert (got[:, :, 0] != rgb[:, :, 0]).any() and (got[:, :, 2] != rgb[:, :, 2]).any()
    one = channelaffine.affine_image(rgb, (77, -200), (2994, -3501, 3501, 2994))      # one map for every colour plane
    np.testing.assert_array_equal(one[:, :, 2], affine_ref.affine_image(rgb[:, :, 2], (77, -200), (2994, -3501, 3501, 2994)))
    page = rgb[None, :, :, 0]
    np.testing.assert_array_equal(channelaffine.affine_image(page, s[0], a[0])[0], got[:, :, 0])
    assert channelaffine.affine_image(rgb, (0, 0), (0, 0, 0, 0)) is rgb
    for bad in (dict(s=(1.0, 0), a=(0, 0, 0, 1)), dict(s=(0, 0), a=(0, 0, 1)), dict(s=(0, 0), a=(0, 0, 0, 50001)), dict(s=(16385, 0), a=(0, 0, 0, 1))):
        with pytest.raises(ValueError):
            channelaffine.affine_image(rgb[:, :, 0], bad['s'], bad['a'])
    with pytest.raises(ValueError):
        channelaffine.affine_image(rgb.astype(np.float32)[:, :, 0], (0, 0), (0, 0, 0, 1))


def test_header_exports_and_constants():
    with open(os.path.join(ROOT, 'include', 'squidstitch.h')) as fh:
        header = fh.read()
    assert re.search(r'int\s+sq_affine_tiles\s*\(', header)
    assert re.search(r'#define\s+SQ_AFFINE_MAX_PPM\s+50000\b', header) and re.search(r'#define\s+SQ_AFFINE_MAX_SIDE\s+65535\b', header)
    assert re.search(r'#define\s+SQ_AFFINE_PLANES_PER_THREAD\s+16\b', header)
    assert re.search(r'#define\s+SQ_VERSION\s+108\b', header)
    assert 'sq_affine_tiles' in native.EXPORTS and native.EXPORTS['sq_affine_tiles'] == native.EXPORTS['sq_shift_tiles']
    assert (native.SQ_AFFINE_MAX_PPM, native.SQ_AFFINE_MAX_SIDE, native.SQ_AFFINE_PLANES_PER_THREAD) == (50000, 65535, 16)
    assert channelaffine.MAX_PPM == affine_ref.MAX_PPM == native.SQ_AFFINE_MAX_PPM
    assert affine_cases.WALK == native.SQ_AFFINE_PLANES_PER_THREAD
    with open(os.path.join(ROOT, 'image-stitcher_amd', 'csrc', 'Makefile')) as fh:
        assert re.search(r'^SRCS\s*=.*\baffine\.hip\b', fh.read(), re.M)
    if os.path.exists(os.path.join(ROOT, 'image-stitcher_amd', 'csrc', 'libsquidstitch.so')):
        assert hasattr(native.lib(), 'sq_affine_tiles')


def test_modules_are_written_apart():
    with open(os.path.join(ROOT, 'tests', 'affine_ref.py')) as fh:
        assert not re.search(r'^\s*(from|import)\s+\S*(channelaffine|image_stitcher_amd)', fh.read(), re.M)
    with open(os.path.join(ROOT, 'image-stitcher_amd', 'channelaffine.py')) as fh:
        assert not re.search(r'^\s*(from|import)\s+\S*affine_ref', fh.read(), re.M)


# ---------------------------------------------------------------------------------------------------- the chain's bytes
FH, FW, NUM_Z = 97, 131, 2
DPC_PLANES = range(2 * NUM_Z, 3 * NUM_Z)
GRID = list(itertools.product(('off', 'shift', 'affine', 'both'), (0, 20000), (1, 2), ('none', 'hot'), (False, True), (False, True),
                              ('uint8', 'uint16')))
A1, A3 = (2994, -3501, 3501, 2994), (0, 30000, 0, 0)


def _chain(mode, ppm=0, k=1, despeckle='none', tophat=False, dpc=False, dtype='uint16', **more):
    kw = dict(num_z=NUM_Z) if mode != 'off' else {}
    if mode in ('shift', 'both'):
        kw['channel_shifts'] = {0: (77, -200), 3: (0, 256)}
    if mode in ('affine', 'both'):
        kw['channel_affines'] = {1: A1, 3: A3}
    kw.update(more)
    return TileChain(distortion_ppm=ppm, binning=k, binning_method='mean', dpc_planes=DPC_PLANES if dpc else (), dpc_gain=1,
                     despeckle=despeckle, despeckle_threshold=40, tophat_radius=5 if tophat else None, seam_qc_radius=2,
                     file_shape=(FH, FW), tile_shape=(FH // k, FW // k), dtype=dtype, **kw)


@pytest.mark.parametrize('n', [1, 6])
def test_chain_bytes_and_buffers_with_affines_on_and_off(n):
    for mode, ppm, k, despeckle, tophat, dpc, dtype in GRID:
        chain = _chain(mode, ppm, k, despeckle, tophat, dpc, dtype)
        on = mode != 'off'
        b = np.dtype(dtype).itemsize
        raw, tile = n * FH * FW * b, n * (FH // k) * (FW // k) * b
        for derived in ((False, True) if dpc else (False,)):
            # ONE 'shift' buffer whichever of the two options is on: the mapped copy of the staged planes
            want = raw + derived * raw + bool(ppm) * (raw + derived * raw) + on * raw + (k > 1) * (tile + derived * tile) + \
                (despeckle != 'none') * tile + tophat * tile
            assert chain.plane_bytes(n, derived) == want, (mode, ppm, k, despeckle, tophat, dpc, dtype, derived)
        assert chain.writer_plane_bytes(n) == raw + bool(ppm) * raw + on * raw + (k > 1) * tile
        assert [name for name, _, _ in chain.buffers].count('shift') == on
        if mode in ('off', 'shift'):      # None, empty and all-zero leave the chain as it is without the argument
            for kw in (dict(channel_affines=None), dict(channel_affines={})):
                other = _chain(mode, ppm, k, despeckle, tophat, dpc, dtype, **kw)
                assert other.buffers == chain.buffers and other.plane_bytes(n, dpc) == chain.plane_bytes(n, dpc)
                assert other.plane_affines([0, 1, 2, 3]) is None
    assert len([b for b in BUFFERS if b[0] == 'shift']) == 1
    assert _chain('affine', dtype='uint8').key('shift', 1, 4) == ('shift', 1, 4, FH, FW, '|u1')


def test_plane_tuples():
    both = _chain('both')
    # channels 0 .. 3 of two z levels each: a shift, an affine, nothing, both
    assert both.plane_affines([0, 1]) is None and both.plane_shifts([0, 1]) == [(77, -200)] * 2      # today's path
    assert both.plane_affines([4, 5]) is None and both.plane_shifts([4, 5]) is None
    assert both.plane_affines([1, 2, 4, 6]) == [(77, -200, 0, 0, 0, 0), (0, 0) + A1, (0, 0, 0, 0, 0, 0), (0, 256) + A3]
    assert both.plane_affines([]) is None and both.plane_affines(None) is None
    assert _chain('affine').plane_affines([0, 2, 7]) == [(0,) * 6, (0, 0) + A1, (0, 0) + A3]
    assert _chain('shift').plane_affines([0, 1, 2]) is None and _chain('off').plane_affines([0]) is None


def test_the_head_launches_one_of_the_two(monkeypatch):
    calls = []
    monkeypatch.setattr(native, 'shift_tiles', lambda tiles, shifts, out=None: calls.append(('shift', shifts, out)) or tiles)
    monkeypatch.setattr(native, 'affine_tiles', lambda tiles, params, out=None: calls.append(('affine', params, out)) or tiles)
    tiles, buf = [object()] * 3, list(range(5))
    tuples = [(0, 0) + A1] * 3
    assert warp_and_bin(tiles, 0, 1, 'mean', None, None, None, buf, tuples) is tiles
    assert calls == [('affine', tuples, [0, 1, 2])]
    del calls[:]
    warp_and_bin(tiles, 0, 1, 'mean', None, None, [(1, 1)] * 3, buf, None)
    warp_and_bin(tiles, 0, 1, 'mean', None, None, [(1, 1)] * 3, buf)
    assert [c[0] for c in calls] == ['shift', 'shift']
    del calls[:]
    warp_and_bin(tiles, 0, 1, 'mean')
    assert calls == []
