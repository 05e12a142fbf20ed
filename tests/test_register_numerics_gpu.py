"""The registration kernels hold float64 on every transform and batch path: not only the shift (an argmax that survives a
transform losing six digits) but the value of the cross-correlation at the refined peak and the two spectral energies agree
with oracle.stitch_oracle.phase_cross_correlation (numpy complex128) to TOL = 1e-10 of their natural scale.  ccmax is a
weighted sum over the whole cross-power spectrum: every forward transform, the product, the normalisation and both
upsampling kernels feed it.

Each case states which dispatch path it is there for and asserts it from native.register_describe (the struct
sq_register_pairs launches from); tests/register_cases.py holds the table, the inputs and the reference with the
conditions that keep the integer comparisons honest.  Every case prints its largest deviation (pytest -s shows them)."""
import numpy as np
import pytest

import register_cases as R
from image_stitcher_amd import native, registration
from oracle import stitch_oracle as O

pytestmark = pytest.mark.gpu

NORMS = (None, 'phase')


def _dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _run(tiles, pairs, n0, n1, u, norm, minmax, pointer_table=False):
    """One native.register_pairs call on `tiles` [N, H, W]; minmax 'identity' (pixels as they are) or 'real' (tile_minmax)."""
    import torch
    dev = _dev()
    stack = torch.from_numpy(tiles).to(dev)
    kw = {}
    if pointer_table:        # every tile an allocation of its own, named by a device pointer table
        keep = [stack[i].clone() for i in range(len(tiles))]
        kw = dict(tile_ptrs=native.pointer_table(keep, dev), shape=tiles.shape[1:], np_dtype=tiles.dtype)
        stack = None
    if minmax == 'identity':
        mm = torch.from_numpy(R.identity_minmax(len(tiles))).to(dev)
    else:
        assert minmax == 'real'
        mm = native.tile_minmax(stack, **kw)
    return native.register_pairs(stack, mm, pairs, n0, n1, u, registration.NORMALIZATIONS[norm], **kw)


def check(tiles, pairs, n0, n1, u, norm, minmax, exempt=(), res=None, label=''):
    """Run the batch once and hold every pair to the oracle on the crops the device sees (O.normalize_image'd tiles, or the
    raw ones under the identity table): integers equal, ccmax and both amplitudes within TOL of their scale.  Pairs in
    `exempt` (degenerate ones whose test asserts exact values instead) are left to the caller.  Returns the results."""
    if res is None:
        res = _run(tiles, pairs, n0, n1, u, norm, minmax)
    seen = tiles if minmax == 'identity' else np.stack([O.normalize_image(t, tiles.dtype.type) for t in tiles])
    worst_cc = worst_amp = 0.0
    for k, p in enumerate(pairs):
        if k in exempt:
            continue
        ref = seen[p['ref_tile']][p['ref_y0']:p['ref_y0'] + n0, p['ref_x0']:p['ref_x0'] + n1]
        mov = seen[p['mov_tile']][p['mov_y0']:p['mov_y0'] + n0, p['mov_x0']:p['mov_x0'] + n1]
        want = R.reference(ref, mov, u, norm)
        d, got, where = want['detail'], res[k], f'{label} pair {k} {norm} u={u}'
        assert got['coarse'].tolist() == d['coarse'], where
        assert got['fine'].tolist() == (d['fine'] if u > 1 else [0, 0]), where
        cc = abs(complex(got['ccmax_re'], got['ccmax_im']) - complex(d['ccmax_re'], d['ccmax_im'])) / want['scale']
        amp = max(abs(got['src_amp'] - d['src_amp']) / d['src_amp'], abs(got['tgt_amp'] - d['tgt_amp']) / d['tgt_amp'])
        worst_cc, worst_amp = max(worst_cc, cc), max(worst_amp, amp)
        assert cc <= R.TOL, f'{where}: ccmax off by {cc:.3e} of its scale'
        assert amp <= R.TOL, f'{where}: amplitude off by {amp:.3e}'
    print(f'register-numerics {label} norm={norm} u={u} pairs={len(pairs)}: ccmax {worst_cc:.3e} amp {worst_amp:.3e}')
    return res


@pytest.mark.parametrize('norm', NORMS)
@pytest.mark.parametrize('c', R.SINGLE_CASES, ids=[c['name'] for c in R.SINGLE_CASES])
def test_single_pair_paths(c, norm):
    R.assert_path(c)
    tiles, pairs = R.single_pair_inputs(c)
    check(tiles, pairs, c['n0'], c['n1'], c['u'], norm, 'identity', label=c['name'])


@pytest.fixture(scope='module')
def batch257():
    """The 257-pair batch, its pair table and the stack run's results per normalisation (shared, never modified)."""
    c = R.BATCH_PATHS['batch257']
    tiles, pairs, planted = R.batch257_inputs()
    runs = {norm: _run(tiles, pairs, c['n0'], c['n1'], c['u'], norm, 'real') for norm in NORMS}
    return dict(c=c, tiles=tiles, pairs=pairs, planted=planted, runs=runs)


@pytest.mark.parametrize('norm', NORMS)
def test_batch_of_257_pairs_wide_upsampling_and_remap_tail(batch257, norm):
    """12 tiles of 160 x 96, real min-max, crop origins and planted shift per pair: upsample_rows<4,16>, tc 4 with the
    share-2 remap of the column blocks and its tail, 8 rows per block."""
    b, c = batch257, batch257['c']
    d = R.assert_path(c)
    assert d['rl_fwd'] > 1 and d['upsample_rows'] == (4, 16) and (d['tc'], d['share']) == (4, 2)
    assert (d['grid_col'][0] * d['grid_col'][1]) % (8 * d['share']) != 0      # the remap tail runs
    assert (b['pairs']['ref_x0'] % 2 == 1).any() and (b['pairs']['mov_x0'] % 2 == 1).any()
    assert len(set(b['planted'])) > 50
    res = check(b['tiles'], b['pairs'], c['n0'], c['n1'], c['u'], norm, 'real', res=b['runs'][norm], label='batch257')
    shifts = registration.shifts_from_results(res, c['u'])[0]
    assert np.abs(shifts + np.array(b['planted'])).max() <= 0.15              # every pair its own planted shift


@pytest.mark.parametrize('norm', NORMS)
def test_batch_of_300_uint8_pairs(norm):
    """10 tiles of 48 x 48 uint8, real min-max: tc 8, the scalar pixel path, 8 rows per block."""
    c = R.BATCH_PATHS['batch300']
    d = R.assert_path(c)
    assert d['rl_fwd'] == 8 and d['tc'] == 8
    tiles, pairs, _ = R.batch300_inputs()
    assert tiles.dtype == np.uint8
    check(tiles, pairs, c['n0'], c['n1'], c['u'], norm, 'real', label='batch300-uint8')


_BATCH_INPUTS, _BATCH_RUNS = {}, {}


def _batch_run(c, norm):
    """(tiles, pairs, results) of a BATCH_CASES entry: inputs made once per case, run once per normalisation, shared by
    the tests below and never modified."""
    if c['name'] not in _BATCH_INPUTS:
        _BATCH_INPUTS[c['name']] = R.batch_case_inputs(c)[:2]
    tiles, pairs = _BATCH_INPUTS[c['name']]
    if (c['name'], norm) not in _BATCH_RUNS:
        _BATCH_RUNS[c['name'], norm] = _run(tiles, pairs, c['n0'], c['n1'], c['u'], norm, 'real')
    return tiles, pairs, _BATCH_RUNS[c['name'], norm]


@pytest.mark.parametrize('norm', NORMS)
@pytest.mark.parametrize('c', R.BATCH_CASES, ids=[c['name'] for c in R.BATCH_CASES])
def test_batch_paths(c, norm):
    """Every launch choice that depends on the number of pairs, in a batch with crop origins and a planted shift per pair
    and the real min-max table: every pair equal to the oracle in its integers and within TOL in ccmax and amplitudes.
    (The planted shift is not asserted: crops as small as 34 x 17 need not recover it.)"""
    R.assert_path(c)
    tiles, pairs, res = _batch_run(c, norm)
    assert tiles.dtype == np.dtype(c['dtype']) and len(pairs) == c['n_pairs'] > 1
    assert (pairs['ref_x0'] % 2 == 1).any() and (pairs['mov_x0'] % 2 == 1).any()
    check(tiles, pairs, c['n0'], c['n1'], c['u'], norm, 'real', res=res, label='batch-' + c['name'])


@pytest.mark.parametrize('norm', NORMS)
@pytest.mark.parametrize('name', R.REVERSED_CASES)
def test_batch_results_do_not_depend_on_the_position(name, norm):
    """The pair table reversed (the same plan: n_pairs is what it was): every pair's bytes are those of its old position,
    whichever pairs share its block, its span of column blocks or its scratch line."""
    c = next(c for c in R.BATCH_CASES if c['name'] == name)
    tiles, pairs, res = _batch_run(c, norm)
    back = _run(tiles, pairs[::-1].copy(), c['n0'], c['n1'], c['u'], norm, 'real')
    assert back[::-1].tobytes() == res.tobytes()


@pytest.mark.parametrize('norm', NORMS)
def test_pointer_table_and_second_run_give_the_same_bytes(batch257, norm):
    b, c = batch257, batch257['c']
    first = b['runs'][norm]
    again = _run(b['tiles'], b['pairs'], c['n0'], c['n1'], c['u'], norm, 'real')
    assert again.tobytes() == first.tobytes()
    by_pointer = _run(b['tiles'], b['pairs'], c['n0'], c['n1'], c['u'], norm, 'real', pointer_table=True)
    assert by_pointer.tobytes() == first.tobytes()


@pytest.mark.parametrize('norm', NORMS)
def test_constant_tile_in_a_batch(norm):
    """A constant tile stretches to 0 / 0 -> 0 everywhere: as the reference of one pair and the moving tile of another its
    pairs give ccmax == 0 and that amplitude == 0 exactly, and the pairs around them are what they are without it."""
    n0, n1, u = 128, 44, 10
    tiles, pairs, _ = R.batch_inputs(12, 160, 96, n0, n1, 40, np.uint16, seed=93, constant_tile=11)
    pairs = pairs[(pairs['ref_tile'] != 11) & (pairs['mov_tile'] != 11)][:24].copy()
    assert len(pairs) == 24
    as_ref, as_mov = 7, 16
    pairs[as_ref]['ref_tile'] = 11
    pairs[as_mov]['mov_tile'] = 11
    res = check(tiles, pairs, n0, n1, u, norm, 'real', exempt=(as_ref, as_mov), label='constant-tile')
    for k, amp in ((as_ref, 'src_amp'), (as_mov, 'tgt_amp')):
        assert res[k]['ccmax_re'] == 0 and res[k]['ccmax_im'] == 0 and res[k][amp] == 0
        assert res[k]['coarse'].tolist() == [0, 0] and res[k]['fine'].tolist() == [0, 0]
    other = {as_ref: 'tgt_amp', as_mov: 'src_amp'}
    for k, amp in other.items():
        assert res[k][amp] > 0
    # the same table without the two pairs: every other pair's bytes are the same
    keep = np.array([k for k in range(len(pairs)) if k not in (as_ref, as_mov)])
    alone = _run(tiles, pairs[keep], n0, n1, u, norm, 'real')
    assert alone.tobytes() == res[keep].tobytes()
