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
