"""Cases of tests/test_register_numerics_gpu.py: crop sizes, the dispatch path each one is there for (as
native.register_describe reports it), their inputs and the float64 reference with the conditions that keep an argmax
comparison honest.  Nothing here needs a device: tests/test_register_plan_cpu.py checks every stated path and the coverage
of the whole table on the host."""
import numpy as np

from image_stitcher_amd import native, synth
from oracle import stitch_oracle as O

# Held to, not tuned: a float64 FFT of N points is off by a few eps * log2 N relative; the longest chain here (three
# transforms of under 2^16 points for a Bluestein line, one more axis, two DFT sums) stays below about 1e-13, and any
# single-precision step (a float32 twiddle, a sincos of an unreduced argument) shows at 1e-8 or above.
TOL = 1e-10
GAP = 1e-9            # the runner-up of a correlation surface lies below the peak by more than this, relative
MIN_BIN = 1.0         # the smallest cross-power bin is larger than this (phase mode divides by it)


def case(n0, n1, path, u=10, seed=77, y0=0, x0=0, pad=0, name=None):
    """One pair of n0 x n1 uint16 crops at (y0, x0) of tiles `pad` pixels taller and wider, identity min-max."""
    return dict(name=name or f'{n0}x{n1}' + (f'-u{u}' if u != 10 else ''), n0=n0, n1=n1, u=u, seed=seed, y0=y0, x0=x0,
                pad=pad, path=path, n_pairs=1, dtype='uint16')


POW2 = dict(m0=0, m1=0, gen0=False, gen1=False, long0=False, long1=False, columns_single=False)
DIRECT = dict(m0=0, m1=0, long0=False, long1=False)
SMALL = dict(rl_fwd=1, upsample_rows=(1, 32))

SINGLE_CASES = [
    # power of two, every tc
    case(64, 64, dict(POW2, tc=8, share=1, col_threads=256, radix0=[], radix1=[], **SMALL)),
    case(128, 32, dict(POW2, tc=4, share=2, col_threads=256)),
    case(256, 32, dict(POW2, tc=2, share=4, col_threads=256)),
    case(512, 16, dict(POW2, tc=1, share=8, col_threads=256)),
    case(2048, 16, dict(POW2, tc=1, share=8, col_threads=512, rl_fwd=4)),
    case(2, 64, dict(POW2, tc=8)),
    case(64, 2, dict(POW2, tc=8)),
    # mixed radix, each butterfly on each axis
    case(36, 60, dict(DIRECT, gen0=True, gen1=True, radix0=[4, 3, 3], radix1=[4, 3, 5], tc=8)),
    case(90, 50, dict(DIRECT, gen0=True, gen1=True, radix0=[2, 3, 3, 5], radix1=[2, 5, 5], tc=8)),
    case(1001, 24, dict(DIRECT, gen0=True, gen1=True, radix0=[7, 11, 13], radix1=[4, 2, 3], tc=2, share=4, col_threads=256)),
    case(24, 1001, dict(DIRECT, gen0=True, gen1=True, radix0=[4, 2, 3], radix1=[7, 11, 13], tc=8)),
    case(2002, 26, dict(DIRECT, gen0=True, gen1=True, radix0=[2, 7, 11, 13], radix1=[2, 13], tc=1, col_threads=256)),
    case(1500, 16, dict(DIRECT, gen0=True, gen1=False, radix0=[4, 3, 5, 5, 5], tc=1)),
    case(3, 7, dict(DIRECT, gen0=True, gen1=True, radix0=[3], radix1=[7], tc=8)),
    # Bluestein in LDS
    case(17, 34, dict(m0=36, m1=75, long0=False, long1=False, columns_single=True, columns_single_threads=512, tc=0, share=8)),
    case(34, 17, dict(m0=75, m1=36, long0=False, long1=False, columns_single=True, tc=0)),
    case(521, 26, dict(m0=1152, m1=0, long0=False, columns_single=True, columns_single_threads=512, gen0=True, gen1=True)),
    case(26, 521, dict(m0=0, m1=1152, long1=False, columns_single=False, gen1=True, tc=8)),
    case(2084, 16, dict(m0=4320, m1=0, long0=False, columns_single=True, columns_single_threads=512, gen0=True)),
    case(16, 3122, dict(m0=0, m1=6400, long1=False, gen1=True, rl_fwd=1, rl_inv=1, threads_fwd=1024, threads_inv=1024)),
    case(4859, 8, dict(m0=9720, m1=0, long0=False, columns_single=True, columns_single_threads=1024, gen0=True)),
    # one directly transformed column per block, and the last size of the tc-column kernel
    case(4620, 16, dict(DIRECT, columns_single=True, columns_single_threads=512, tc=0, share=8, gen0=True, col_threads=0)),
    case(6000, 16, dict(DIRECT, columns_single=True, columns_single_threads=1024, tc=0, gen0=True)),
    case(4608, 16, dict(DIRECT, columns_single=False, tc=1, share=8, col_threads=512, gen0=True, columns_single_threads=0)),
    # lines too long for the LDS
    case(10, 10000, dict(m0=0, m1=0, long0=False, long1=True, gen1=True, rl_fwd=1, threads_fwd=512), seed=78),
    case(16384, 6, dict(m0=0, m1=0, long0=True, long1=False, gen0=False, columns_single=True, columns_single_threads=512,
                        share=0), seed=78),
    case(8, 12288, dict(m0=0, m1=0, long1=True, gen1=True, radix1=[4, 4, 4, 4, 4, 4, 3]), seed=78),
    case(16, 4861, dict(m0=0, long0=False, long1=True, gen1=True), seed=78),
    case(4862, 12, dict(m1=0, long0=True, long1=False, columns_single=True), seed=78),
    case(9733, 6, dict(m1=0, long0=True, long1=False, columns_single=True), seed=78),
    # row remainder and alignment: odd crop origin inside tiles 64 wider
    case(64, 8, dict(POW2, tc=8), y0=5, x0=31, pad=64, name='64x8-x31'),
    case(64, 9, dict(DIRECT, gen0=False, gen1=True, radix1=[3, 3]), y0=0, x0=1, pad=64, name='64x9-x1'),
    case(64, 15, dict(DIRECT, gen0=False, gen1=True, radix1=[3, 5]), y0=3, x0=17, pad=64, name='64x15-x17'),
    case(64, 44, dict(DIRECT, gen0=False, gen1=True, radix1=[4, 11]), y0=7, x0=55, pad=64, name='64x44-x55'),
]
# upsample_factor 1, 4, 10 and 100 (region 150)
for _n0, _n1, _path in ((64, 64, POW2), (128, 44, dict(DIRECT, tc=4, share=2)), (17, 1001, dict(m0=36, m1=0, columns_single=True))):
    for _u in (1, 4, 10, 100):
        if (_n0, _n1, _u) != (64, 64, 10):
            SINGLE_CASES.append(case(_n0, _n1, dict(_path, upsample_rows=None if _u == 1 else (1, 32)), u=_u))

# the Bluestein lengths above that have to be non-trivial ones
for _c in SINGLE_CASES:
    if _c['name'] in ('16x4861', '4862x12', '9733x6'):
        _c['bluestein_long'] = True

BATCH_PATHS = {
    # 257 pairs of 128 x 44: 6 column blocks per pair, 1542 in all = 96 spans of 16 and a tail of 6
    'batch257': dict(n_pairs=257, n0=128, n1=44, u=10, dtype='uint16',
                     path=dict(DIRECT, upsample_rows=(4, 16), tc=4, share=2, rl_fwd=8, gen0=False, gen1=True, grid_col=(6, 257))),
    'batch300': dict(n_pairs=300, n0=32, n1=32, u=10, dtype='uint8',
                     path=dict(POW2, tc=8, share=1, rl_fwd=8, upsample_rows=(4, 16))),
}


def batch_case(n_pairs, n0, n1, path, holds, dtype='uint16', u=10):
    """A batch of n_pairs crops from batch_inputs (12 tiles, 32 rows and 52 columns of room, real min-max).  `holds`:
    what the case is there for beyond the `path` keys, as (what, predicate of the describe struct) -- the crossing of a
    launch choice with the batch, which assert_path checks too."""
    name = f'{n_pairs}x{n0}x{n1}' + ('-uint8' if dtype == 'uint8' else '') + (f'-u{u}' if u != 10 else '')
    return dict(name=name, n_pairs=n_pairs, n0=n0, n1=n1, u=u, dtype=dtype, path=path, holds=holds)


def _blocks(d):
    return d['grid_col'][0] * d['grid_col'][1]


def _spans(share):
    """The column-block remap works within spans of 8 * share blocks, which cross pair boundaries."""
    return [(f'share {share}: a span of {8 * share} column blocks crosses pairs', lambda d: 8 * share > d['grid_col'][0] and _blocks(d) >= 8 * share)]


def _tail(share):
    """... and the blocks after the last whole span are left unmapped."""
    return _spans(share) + [('a tail of column blocks is left unmapped', lambda d: _blocks(d) % (8 * share) != 0)]


def _partial_rows(n0):
    """The last block of both row kernels has fewer lines than the others; an odd n0's last line repeats its row."""
    return [('the last forward block is partial', lambda d: d['rl_fwd'] > 1 and n0 % d['rl_fwd'] != 0),
            ('the last inverse block is partial', lambda d: d['rl_inv'] > 1 and ((n0 + 1) // 2) % d['rl_inv'] != 0)]


_ODD = [('odd n0, several row pairs per block', lambda d: d['rl_inv'] > 1)]
_MIXED = dict(DIRECT, gen0=True, gen1=True)
_BLUE_BOTH = dict(m0=75, m1=36, long0=False, long1=False, rl_fwd=4, rl_inv=2, columns_single=True, share=8, grid_col=(16, 64))

# Every launch choice that depends on the number of pairs, together with a batch: held to the float64 oracle at TOL by
# test_batch_paths (tests/test_register_numerics_gpu.py), every pair of every case.  Largest deviation over the pairs
# of a case measured on an MI355X (the `register-numerics` lines of pytest -s), ccmax as a fraction of its scale under
# normalisation None and 'phase', the amplitudes relative (the same under both).  The bound stays TOL:
#   case               ccmax None  ccmax phase  amplitude  |  case               ccmax None  ccmax phase  amplitude
#   96x45x36            1.4e-15     4.2e-16     9.4e-16    |  5x521x26            9.0e-16     2.9e-16     7.5e-16
#   64x45x36-uint8      1.8e-15     1.4e-16     6.7e-16    |  40x32x4861          1.3e-14     1.5e-15     5.3e-15
#   64x34x17            1.6e-15     1.3e-14     9.1e-16    |  16x4862x64          1.9e-15     3.8e-16     1.6e-15
#   64x34x17-uint8      1.6e-15     1.3e-15     8.2e-16    |  6x16x4861-uint8     6.2e-15     4.7e-16     2.5e-15
#   130x32x97           2.5e-15     7.3e-16     1.4e-15    |  130x250x36          1.7e-15     4.1e-16     1.0e-15
#   5x512x16            1.0e-15     2.3e-16     8.1e-16    |  8x64x64-u100        6.5e-16     5.6e-16     8.4e-16
#   5x256x32            8.3e-16     2.3e-16     1.0e-15    |  24x250x20-u4        1.1e-15     3.6e-16     5.4e-16
#   5x4620x16           2.2e-15     3.0e-16     6.5e-16    |  24x45x36-u1         1.4e-16     2.3e-16     8.5e-16
BATCH_CASES = [
    # lines per block with a partial last block, odd n0
    batch_case(96, 45, 36, dict(_MIXED, rl_fwd=8, rl_inv=4, radix0=[3, 3, 5], radix1=[4, 3, 3]), _partial_rows(45) + _ODD),
    batch_case(64, 45, 36, dict(_MIXED, rl_fwd=4, rl_inv=2), _partial_rows(45) + _ODD, dtype='uint8'),
    # Bluestein rows with several lines per block, Bluestein columns one per block across pairs
    batch_case(64, 34, 17, _BLUE_BOTH, _partial_rows(34) + _spans(8)),
    batch_case(64, 34, 17, _BLUE_BOTH, _partial_rows(34) + _spans(8), dtype='uint8'),
    batch_case(130, 32, 97, dict(m0=0, m1=200, long1=False, rl_fwd=5, rl_inv=4),
               [('rl_fwd is no power of two and leaves a partial block', lambda d: d['rl_fwd'] & (d['rl_fwd'] - 1) and 32 % d['rl_fwd'] != 0)]),
    # the remap of the column blocks across pairs, every share, and one column per block
    batch_case(5, 512, 16, dict(POW2, tc=1, share=8, grid_col=(16, 5)), _tail(8)),
    batch_case(5, 256, 32, dict(POW2, tc=2, share=4, grid_col=(12, 5)), _tail(4)),
    batch_case(5, 4620, 16, dict(DIRECT, columns_single=True, tc=0, share=8, gen0=True, grid_col=(16, 5)), _tail(8)),
    batch_case(5, 521, 26, dict(m0=1152, m1=0, long0=False, columns_single=True, share=8, rl_fwd=4), _tail(8)),
    # long lines: more lines than scratch lines, so a workgroup takes several, of different pairs
    batch_case(40, 32, 4861, dict(m0=0, m1=10240, long0=False, long1=True, grid_fwd=(512, 1), grid_inv=(512, 1)),
               [('more forward lines than workgroups', lambda d: d['grid_fwd'][0] < 40 * 32),
                ('more inverse lines than workgroups', lambda d: d['grid_inv'][0] < 40 * 16)]),
    batch_case(16, 4862, 64, dict(m0=10240, m1=0, long0=True, long1=False, columns_single=True, grid_col=(512, 1),
                                  upsample_rows=(4, 16), grid_up_rows=(38, 16)),
               [('more columns than workgroups', lambda d: d['grid_col'][0] < 16 * 33),
                ('several row blocks of the wide upsampling kernel', lambda d: d['grid_up_rows'][0] > 1)]),
    batch_case(6, 16, 4861, dict(m0=0, m1=10240, long1=True), [], dtype='uint8'),
    # the wide upsampling kernel with a partial last row block (125 row pairs: 64 + 61)
    batch_case(130, 250, 36, dict(DIRECT, upsample_rows=(4, 16), grid_up_rows=(2, 130), tc=4, share=2, grid_col=(6, 130)),
               [('the last row block of the wide upsampling kernel is partial', lambda d: 125 % 64 != 0 and d['grid_up_rows'][0] == 2)]
               + _tail(2)),
    # the other upsample factors
    batch_case(8, 64, 64, dict(POW2, upsample_rows=(1, 32)), [], u=100),
    batch_case(24, 250, 20, dict(DIRECT, rl_fwd=8, rl_inv=4, upsample_rows=(1, 32)), _partial_rows(250), u=4),
    batch_case(24, 45, 36, dict(_MIXED, upsample_rows=None), [], u=1),
]
# the four whose pair table test_batch_results_do_not_depend_on_the_position runs reversed as well
REVERSED_CASES = ('64x34x17', '5x512x16', '40x32x4861', '16x4862x64')


def batch_case_inputs(c):
    """(tiles, pairs, planted) of a BATCH_CASES entry."""
    dtype = np.dtype(c['dtype'])
    return batch_inputs(12, c['n0'] + 32, c['n1'] + 52, c['n0'], c['n1'], c['n_pairs'], dtype.type,
                        seed=91 if dtype == np.uint16 else 102)


def describe(c):
    return native.register_describe(c['n_pairs'], c['n0'], c['n1'], c['u'], c['dtype'])


def assert_path(c):
    """The case runs where it says it does."""
    d = describe(c)
    for key, want in c['path'].items():
        assert d[key] == want, f"{c.get('name')}: {key} is {d[key]}, the case is there for {want}"
    if c.get('bluestein_long'):
        m = d['m0'] if d['long0'] else d['m1']
        assert m > 9728, f"{c.get('name')}: Bluestein length {m} fits the LDS"
    for what, holds in c.get('holds', ()):
        assert holds(d), f"{c.get('name')}: not so: {what} ({d})"
    return d


def identity_minmax(n_tiles):
    """A (min > max) entry per tile: the kernel takes the pixels as they are."""
    return np.array([[1, 0]] * n_tiles, dtype=np.int32)


def single_pair_inputs(c):
    """(tiles [2, H, W] uint16, pairs[1]) of a single-pair case: the construction of test_long_non_power_of_two_lines, a
    planted shift of (3, -5) -- 0 along an axis of at most 12 points -- and noise on the moving crop."""
    n0, n1, pad, y0, x0 = c['n0'], c['n1'], c['pad'], c['y0'], c['x0']
    H, W = n0 + pad, n1 + pad
    dy, dx = (3 if n0 > 12 else 0), (-5 if n1 > 12 else 0)
    big = synth.scene_patch(c['seed'], 0, 0, H + 64, W + 64)
    ref = big[32:32 + H, 32:32 + W].copy()
    mov = big[32 - dy:32 - dy + H, 32 - dx:32 - dx + W].copy()
    mov[y0:y0 + n0, x0:x0 + n1] += synth.noise_patch(3, n0, n1, 200)
    pairs = np.zeros(1, dtype=native.PAIR_DTYPE)
    pairs[0] = (0, 1, y0, x0, y0, x0)
    return np.stack([ref, mov]).astype(np.uint16), pairs


def batch_inputs(n_tiles, H, W, n0, n1, n_pairs, dtype, seed, constant_tile=None):
    """Tiles cut from one scene at small per-tile offsets with per-tile noise, and a pair table whose every row has crop
    origins of its own (odd x0 included) and a planted shift of its own within +-5 pixels."""
    big = synth.scene_patch(seed, 0, 0, H + 32, W + 32)
    origins = [(8 + (t * 3) % 7, 8 + (t * 5) % 11) for t in range(n_tiles)]
    tiles = []
    for t, (oy, ox) in enumerate(origins):
        if np.dtype(dtype) == np.uint8:
            # strong noise in grey levels: the scene is a 2 x 2 box sum with next to no energy at the Nyquist frequencies,
            # and of a few hundred integer crops some would have such a bin exactly zero
            img = np.clip(big[oy:oy + H, ox:ox + W] * 255 // 42000 + synth.noise_patch(seed * 1000 + t, H, W, 40), 0, 255)
        else:
            img = big[oy:oy + H, ox:ox + W] + synth.noise_patch(100 + t, H, W, 200)
        tiles.append(img)
    tiles = np.stack(tiles).astype(dtype)
    if constant_tile is not None:
        tiles[constant_tile] = 777 if np.dtype(dtype) == np.uint16 else 77
    rng = np.random.default_rng(seed)
    ry, rx = H - n0, W - n1                       # room of a crop inside its tile
    pairs = np.zeros(n_pairs, dtype=native.PAIR_DTYPE)
    planted = []
    k = 0
    while k < n_pairs:
        a, b = (int(v) for v in rng.choice(n_tiles, 2, replace=False))
        dy, dx = (int(v) for v in rng.integers(-5, 6, 2))
        ya, xa = int(rng.integers(0, ry + 1)), int(rng.integers(0, rx + 1))
        # scene row of the reference crop = that of the moving crop + dy
        yb, xb = ya + origins[a][0] - origins[b][0] - dy, xa + origins[a][1] - origins[b][1] - dx
        if not (0 <= yb <= ry and 0 <= xb <= rx):
            continue
        pairs[k] = (a, b, ya, xa, yb, xb)
        planted.append((dy, dx))
        k += 1
    return tiles, pairs, planted


def batch257_inputs():
    return batch_inputs(12, 160, 96, 128, 44, 257, np.uint16, seed=91)


def batch300_inputs():
    return batch_inputs(10, 48, 48, 32, 32, 300, np.uint8, seed=102)


def reference(ref, mov, u, norm):
    """The oracle's answer for one pair of crops, after the conditions that make comparing integers with it meaningful
    have been checked on the reference alone: in the whole-pixel and in the upsampled correlation the runner-up is below
    the peak by more than GAP (relative), no cross-power bin is small enough for phase mode's division to amplify
    rounding, and at u = 1 (where the device reports |cc| only) the peak value is a positive real number."""
    shifts, err, phase, d = O.phase_cross_correlation(ref, mov, u, norm)
    f, g = np.fft.fftn(ref), np.fft.fftn(mov)
    prod = f * g.conj()
    mag = np.abs(prod)
    assert mag.min() > MIN_BIN, f'smallest cross-power bin {mag.min()}'
    if norm == 'phase':
        prod = prod / np.maximum(mag, 100 * np.finfo(np.float64).eps)

    def gap_of(surface):
        a = np.abs(surface).ravel()
        second, first = np.partition(a, a.size - 2)[-2:]
        return (first - second) / first
    gap = gap_of(np.fft.ifftn(prod))
    assert gap > GAP, f'whole-pixel runner-up within {gap} of the peak'
    if u > 1:
        region = int(np.ceil(u * 1.5))
        offs = np.fix(region / 2.0) - np.round(np.array(d['coarse'], dtype=np.float64) * u) / u * np.float64(u)
        up_gap = gap_of(O._upsampled_dft(prod.conj(), region, np.float64(u), offs))
        assert up_gap > GAP, f'upsampled runner-up within {up_gap} of the peak'
        gap = min(gap, up_gap)
    n0, n1 = ref.shape
    if norm is None:
        scale = np.sqrt(d['src_amp'] * d['tgt_amp'])
    else:
        scale = float(n0 * n1) if u > 1 else 1.0
    if u == 1:
        assert d['ccmax_re'] > 0 and abs(d['ccmax_im']) <= 1e-13 * scale
    return dict(detail=d, shifts=shifts, error=err, phase=phase, scale=scale, gap=gap, min_bin=float(mag.min()))
