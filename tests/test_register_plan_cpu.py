"""sq_register_describe (host only): the launch description sq_register_pairs launches from, against values worked out by
hand from the comments of csrc/register.hip, and the coverage of the case table of tests/test_register_numerics_gpu.py."""
import os
import re

import pytest

import register_cases as R
from image_stitcher_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def D(n_pairs, n0, n1, u=10, dtype='uint16'):
    return native.register_describe(n_pairs, n0, n1, u, dtype)


def test_entry_point_is_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'squidstitch.h')).read()
    assert re.search(r'int\s+sq_register_describe\s*\(', header) and 'typedef struct sq_register_plan' in header
    assert len(native.EXPORTS['sq_register_describe'][1]) == 6
    declared = int(re.search(r'#define\s+SQ_VERSION\s+(\d+)\b', header).group(1))
    assert declared == native.SQ_VERSION == native.lib().sq_version()


def test_transform_of_each_axis():
    # a power of two: no stages, no Bluestein length
    d = D(1, 64, 64)
    assert (d['m0'], d['m1'], d['gen0'], d['gen1'], d['radix0'], d['radix1']) == (0, 0, False, False, [], [])
    assert not d['long0'] and not d['long1']
    # smooth lengths: 4s first, then 2, 3, 5, 7, 11, 13
    assert D(1, 1500, 48)['radix0'] == [4, 3, 5, 5, 5] and D(1, 1500, 48)['radix1'] == [4, 4, 3]
    assert D(1, 2002, 26)['radix0'] == [2, 7, 11, 13] and D(1, 26, 1001)['radix1'] == [7, 11, 13]
    # Bluestein through the CHEAPEST smooth length in [2n - 1, 2n - 1 + n / 4]
    assert D(1, 2084, 16)['m0'] == 4320 and D(1, 2084, 16)['radix0'] == [4, 4, 2, 3, 3, 3, 5]      # not 4200 (a radix-7 stage)
    assert D(1, 16, 3122)['m1'] == 6400 and D(1, 16, 3122)['radix1'] == [4, 4, 4, 4, 5, 5]         # not 6250 = 2 5^5
    assert D(1, 4859, 8)['m0'] == 9720 and not D(1, 4859, 8)['long0']
    # 17: 33 = 3 11 costs 17.3 a point, 35 = 5 7 12.0, 36 = 4 3 3 6.8; 34: 72 = 4 2 3 3 costs 633.6, 75 = 3 5 5 622.5
    assert D(1, 17, 34)['m0'] == 36 and D(1, 17, 34)['m1'] == 75
    # 521: 1152 = 4 4 4 2 3 3 (13.2 a point, 15206) against 1080 = 4 2 3 3 3 5 (14.1 a point, 15228)
    assert D(1, 521, 26)['m0'] == 1152 and D(1, 521, 26)['radix0'] == [4, 4, 4, 2, 3, 3]
    # a mixed-radix Bluestein length makes the axis' kernels the general ones
    assert D(1, 2084, 16)['gen0'] and not D(1, 2084, 16)['gen1']


def test_lines_that_do_not_fit_the_lds():
    # 9728 points fit: a smooth 9720 does; 9728 = 2^9 19 itself needs a Bluestein line; 4861 needs >= 9721 points and no
    # smooth length lies in 9721 ... 9728
    assert not D(1, 9720, 8)['long0'] and not D(1, 8, 8192)['long1']
    assert D(1, 8, 9728)['long1'] and D(1, 8, 9728)['m1'] >= 2 * 9728 - 1
    d = D(1, 16, 4861)
    assert d['long1'] and d['m1'] > 9728 and not d['long0']
    assert (d['rl_fwd'], d['rl_inv'], d['threads_fwd'], d['threads_inv'], d['lds_fwd'], d['lds_inv']) == (1, 1, 512, 512, 0, 0)
    assert d['grid_fwd'] == (16, 1) and d['grid_inv'] == (8, 1)           # fewer lines than scratch slots
    d = D(3, 40, 4861)
    assert d['grid_fwd'] == (120, 1) and D(20, 40, 4861)['grid_fwd'] == (512, 1)
    d = D(1, 4861, 12)
    assert d['long0'] and d['columns_single'] and d['columns_single_threads'] == 512 and d['grid_col'] == (7, 1)
    assert (d['tc'], d['share'], d['col_threads'], d['lds_col']) == (0, 0, 0, 0)
    d = D(1, 10, 10000)
    assert d['long1'] and d['m1'] == 0 and d['gen1'] and d['radix1'] == [4, 4, 5, 5, 5, 5]
    d = D(1, 16384, 6)
    assert d['long0'] and d['m0'] == 0 and not d['gen0']


def test_columns():
    # two [tc][n0] complex arrays within 16 KiB: n0 64 -> 8, 128 -> 4, 256 -> 2, 512 and up -> 1; share = 8 / tc below 8
    for n0, tc, share in ((64, 8, 1), (128, 4, 2), (256, 2, 4), (512, 1, 8), (2048, 1, 8)):
        d = D(1, n0, 32)
        assert (d['tc'], d['share'], d['columns_single'], d['lds_col']) == (tc, share, False, 2 * tc * n0 * 16), n0
    # ... widened until a stage has a butterfly per thread: 1001 = 7 11 13 has 77 radix-13 butterflies a line
    assert D(1, 1001, 24)['tc'] == 2 and D(1, 2002, 26)['tc'] == 1
    # 256 threads, 512 from 64 KiB of columns on
    assert D(1, 1024, 32)['col_threads'] == 256 and D(1, 2048, 32)['col_threads'] == 512
    # the grid is a multiple of share: n1 = 44 -> 23 columns -> 6 blocks of 4
    assert D(257, 128, 44)['grid_col'] == (6, 257) and D(1, 512, 16)['grid_col'] == (16, 1)
    # the last size two columns fit the LDS at; past it one column per block, 512 threads up to 80 KiB of line
    d = D(1, 4608, 16)
    assert (d['tc'], d['columns_single'], d['col_threads'], d['columns_single_threads']) == (1, False, 512, 0)
    d = D(1, 4620, 16)
    assert (d['tc'], d['columns_single'], d['col_threads'], d['columns_single_threads'], d['share']) == (0, True, 0, 512, 8)
    assert d['lds_col'] == 4620 * 16 and d['grid_col'] == (16, 1)
    assert D(1, 6000, 16)['columns_single_threads'] == 1024
    # a Bluestein column always goes one per block
    d = D(1, 2084, 16)
    assert d['columns_single'] and d['columns_single_threads'] == 512 and d['lds_col'] == 4320 * 16
    assert D(1, 4859, 8)['columns_single_threads'] == 1024


def test_rows_depend_on_the_batch():
    # one pair of 64 x 64: never fewer than 512 blocks' worth of lines -> one line per block
    d = D(1, 64, 64)
    assert (d['rl_fwd'], d['rl_inv'], d['threads_fwd'], d['grid_fwd'], d['grid_inv']) == (1, 1, 64, (64, 1), (32, 1))
    assert d['lds_fwd'] == 64 * 16
    # 257 pairs of 128 x 44: 8 lines per block either way, 256 threads
    d = D(257, 128, 44)
    assert (d['rl_fwd'], d['rl_inv'], d['threads_fwd'], d['threads_inv']) == (8, 8, 256, 256)
    assert d['grid_fwd'] == (16, 257) and d['grid_inv'] == (8, 257) and d['lds_fwd'] == 8 * 44 * 16
    # the forward kernel keeps to 16 KB of lines, the inverse to 32 KB: 256-point lines -> 4 and 8
    d = D(992, 1024, 256)
    assert (d['rl_fwd'], d['rl_inv']) == (4, 8)
    # one line per block: threads by the line's bytes (a Bluestein line is m1 points)
    assert D(992, 256, 1024)['threads_fwd'] == 256 and D(1, 16, 2048)['threads_fwd'] == 1024
    assert D(1, 16, 1500)['threads_fwd'] == 512 and D(1, 16, 3122)['threads_fwd'] == 1024
    assert D(1, 16, 512)['threads_fwd'] == 128 and D(1, 16, 128)['threads_fwd'] == 64
    # the pixel type changes no launch shape
    assert D(300, 32, 32, 10, 'uint8') == D(300, 32, 32, 10, 'uint16')


def test_upsampling_kernel_depends_on_the_batch():
    assert D(1, 64, 64, 1)['upsample_rows'] is None and D(1, 64, 64, 1)['grid_up_rows'] == (0, 0)
    # 64 row pairs = one 64-row block per pair: the wide kernel from 256 pairs on
    assert D(255, 128, 44)['upsample_rows'] == (1, 32) and D(255, 128, 44)['grid_up_rows'] == (4, 255)
    assert D(256, 128, 44)['upsample_rows'] == (4, 16) and D(257, 128, 44)['grid_up_rows'] == (1, 257)
    assert D(1, 64, 64, 100)['upsample_rows'] == (1, 32)


def test_bad_arguments():
    for args in ((0, 64, 64), (65536, 64, 64), (1, 1, 64), (1, 64, 64, 0), (1, 64, 64, 101), (1, 65536, 4)):
        with pytest.raises(native.NativeError):
            D(*args)
    with pytest.raises(native.NativeError, match='dtype'):
        D(1, 64, 64, 10, 'float32')


def test_every_case_runs_where_it_says():
    for c in R.SINGLE_CASES + list(R.BATCH_PATHS.values()):
        R.assert_path(c)


def test_every_batch_case_runs_where_it_says():
    assert len({c['name'] for c in R.BATCH_CASES}) == len(R.BATCH_CASES)
    assert set(R.REVERSED_CASES) <= {c['name'] for c in R.BATCH_CASES}
    for c in R.BATCH_CASES:
        R.assert_path(c)


def test_the_batch_table_covers_every_crossing():
    """Every launch choice that make_plan takes from the number of pairs, met by a case of SEVERAL pairs."""
    cases = [(c, R.describe(c)) for c in R.BATCH_CASES]
    assert all(c['n_pairs'] > 1 for c, _ in cases)

    def some(holds):
        return any(holds(c, d) for c, d in cases)

    def nrp(c):
        return (c['n0'] + 1) // 2
    short1 = lambda d: not d['long1']
    # several lines per block: Bluestein rows, a partial last block, the repeated row of an odd n0, a cap of 5 lines
    assert some(lambda c, d: d['m1'] > 0 and short1(d) and d['rl_fwd'] > 1 and d['rl_inv'] > 1)
    assert some(lambda c, d: short1(d) and c['n0'] % d['rl_fwd'] != 0)
    assert some(lambda c, d: short1(d) and c['n0'] % 2 == 1 and d['rl_inv'] > 1 and nrp(c) % d['rl_inv'] != 0)
    assert some(lambda c, d: d['rl_fwd'] & (d['rl_fwd'] - 1))
    # the column-block remap with its tail, in the tc-column kernel and in the one-column kernel
    blocks = lambda d: d['grid_col'][0] * d['grid_col'][1]
    for share in (2, 4, 8):
        assert some(lambda c, d: d['share'] == share and not d['long0'] and blocks(d) >= 8 * share
                    and blocks(d) % (8 * share) != 0), share
    assert {d['tc'] for c, d in cases if not d['columns_single'] and blocks(d) % (8 * d['share'])} >= {1, 2, 4}
    assert some(lambda c, d: d['columns_single'] and not d['long0'] and not d['m0'])
    assert some(lambda c, d: d['columns_single'] and not d['long0'] and d['m0'])
    # long lines: a workgroup walks over several
    assert some(lambda c, d: d['long0'] and c['n_pairs'] * (c['n1'] // 2 + 1) > d['grid_col'][0])
    assert some(lambda c, d: d['long1'] and c['n_pairs'] * c['n0'] > d['grid_fwd'][0] and c['n_pairs'] * nrp(c) > d['grid_inv'][0])
    # uint8 on each kind of row transform
    u8 = lambda c: c['dtype'] == 'uint8'
    assert some(lambda c, d: u8(c) and d['gen1'] and not d['m1'])
    assert some(lambda c, d: u8(c) and d['m1'] and short1(d))
    assert some(lambda c, d: u8(c) and d['long1'])
    # the wide upsampling kernel over several row blocks, the last one partial; every other upsample factor
    assert some(lambda c, d: d['upsample_rows'] == (4, 16) and d['grid_up_rows'][0] > 1 and nrp(c) % 64 != 0)
    assert {c['u'] for c, _ in cases} >= {1, 4, 100}


def test_the_case_table_covers_every_path():
    plans = [R.describe(c) for c in R.SINGLE_CASES + list(R.BATCH_PATHS.values())]
    tc_kernel = [d for d in plans if not d['columns_single']]
    single = [d for d in plans if d['columns_single'] and not d['long0']]
    assert {d['tc'] for d in tc_kernel} == {1, 2, 4, 8}
    assert {d['col_threads'] for d in tc_kernel} == {256, 512}
    assert {d['columns_single_threads'] for d in single} == {512, 1024}
    for axis in '01':
        assert {d['gen' + axis] for d in plans} == {False, True}
        assert any(d['m' + axis] and not d['long' + axis] for d in plans)          # Bluestein in LDS
        assert any(d['long' + axis] and not d['m' + axis] for d in plans)          # long, direct
        assert any(d['long' + axis] and d['m' + axis] for d in plans)              # long, Bluestein
        for p in (2, 3, 4, 5, 7, 11, 13):
            assert any(p in d['radix' + axis] and not d['m' + axis] for d in plans), (axis, p)
    assert {d['upsample_rows'] for d in plans} == {None, (1, 32), (4, 16)}
    assert any(d['rl_fwd'] == 1 for d in plans) and any(d['rl_fwd'] > 1 for d in plans)
    assert any(d['share'] > 1 and not d['columns_single'] and (d['grid_col'][0] * d['grid_col'][1]) % (8 * d['share'])
               for d in plans)                                                     # the remap tail
    assert {c['u'] for c in R.SINGLE_CASES} == {1, 4, 10, 100}
    assert {c['dtype'] for c in R.BATCH_PATHS.values()} == {'uint8', 'uint16'}
