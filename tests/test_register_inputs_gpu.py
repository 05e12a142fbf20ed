"""How the tiles lie in memory when registration's four tile readers meet them: sq_tile_minmax, sq_normalize_tiles,
sq_register_pairs and sq_pair_overlap_moments take tile_pitch, tile_stride and a base pointer or a device pointer table
(include/squidstitch.h), and the Python binding only ever passes dense stacks.  Here they are called through ctypes on padded,
misaligned layouts (tests/tile_layouts.py: everything around a tile holds 0 and the dtype's maximum alternately, so a read
outside a tile's columns changes the answer) and through pointer tables of separately allocated, differently aligned tiles.

Everything is exact integer work or a comparison of bytes: no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import register_cases as R
import tile_layouts as T
from image_stitcher_amd import native, registration
from oracle import stitch_oracle as O

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _to_device(host):
    import torch
    return torch.from_numpy(np.ascontiguousarray(host)).to(_dev())


class Source:
    """The tile arguments of one call: (tile_ptrs, tile_base, tile_stride) and the pitch, with what keeps them alive."""

    def __init__(self, label, ptrs, base, stride, pitch, keep):
        self.label, self.ptrs, self.base, self.stride, self.pitch, self.keep = label, ptrs, base, stride, pitch, keep


def _upload(layout):
    """(device tensor of the layout's buffer, address of tile 0).  The buffer starts on a 16-byte line, as
    tile_layouts.row_phases takes it to."""
    buf = _to_device(layout.buffer)
    assert buf.data_ptr() % T.LINE == 0
    return buf, buf.data_ptr() + layout.base_offset * layout.buffer.itemsize


def base_source(layout):
    buf, address = _upload(layout)
    return Source(f'pitch {layout.pitch}, stride {layout.tile_stride}, offset {layout.base_offset}', None, address,
                  layout.tile_stride, layout.pitch, buf)


def table_source(singles):
    import torch
    uploads = [_upload(single) for single in singles]
    table = torch.tensor([address for _, address in uploads], dtype=torch.int64).to(_dev())
    return Source('pointer table', table.data_ptr(), None, 0, singles[0].pitch, (uploads, table))


def tile_minmax(src, n, h, w, dtype):
    """sq_tile_minmax -> host int64 [n, 2]; the row behind the table is left alone."""
    out = _to_device(np.full((n + 1, 2), -7, dtype=np.int32))
    status = native.lib().sq_tile_minmax(src.ptrs, src.base, src.stride, n, h, w, src.pitch, native.sq_dtype_of(dtype),
                                         out.data_ptr(), native._stream_ptr())
    assert status == 0, native.lib().sq_last_error().decode()
    got = out.cpu().numpy().astype(np.int64)
    assert got[n].tolist() == [-7, -7], f'{src.label}: wrote behind the min-max table'
    return got[:n], out


def dense_minmax(stack):
    flat = np.asarray(stack).reshape(len(stack), -1).astype(np.int64)
    return np.stack([flat.min(axis=1), flat.max(axis=1)], axis=1)


# ---- a. sq_tile_minmax sees every pixel position ----------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,w', [(d, w) for d in ('uint16', 'uint8') for w in T.MINMAX_WIDTHS[d]])
def test_tile_minmax_sees_every_pixel_position(dtype, w):
    """minmax_kernel splits a row by the alignment of its address: a scalar head up to the next 16-byte line, 16-byte vectors
    with a lane stride of 64 of them, a scalar tail.  A pixel it drops changes the answer only where it was the tile's extreme:
    so every position of rows 0, 4 and 8 is the tile's only maximum in one tile and its only minimum in another, in rows
    w + 3 apart whose phase changes from row to row and from tile to tile."""
    stack, max_at, min_at, base_offset, gap = T.minmax_case(dtype, w)
    n, h = len(stack), T.MINMAX_H
    layout = T.padded(stack, T.MINMAX_PAD, base_offset, gap)
    view = T.tiles_of(layout)
    want = dense_minmax(view)
    # before the device is touched: the planted values are the strict extremes of the [:, :w] view
    flat = np.asarray(view).reshape(n, -1)
    t = np.arange(n)
    np.testing.assert_array_equal(view[t, max_at[:, 0], max_at[:, 1]], want[:, 1])
    np.testing.assert_array_equal(view[t, min_at[:, 0], min_at[:, 1]], want[:, 0])
    assert ((flat == want[:, 1:2]).sum(axis=1) == 1).all() and ((flat == want[:, 0:1]).sum(axis=1) == 1).all()
    assert want.min() > 0 and want.max() < np.iinfo(dtype).max          # neither is a fill value
    assert T.first_rows_phases(layout) == set(range(T.vec(dtype)))
    for src in (base_source(layout), table_source(T.separate(stack, T.MINMAX_PAD))):
        got, _ = tile_minmax(src, n, h, w, dtype)
        wrong = np.flatnonzero((got != want).any(axis=1))
        assert len(wrong) == 0, (f'{dtype} w={w} {src.label}: {len(wrong)} of {n} tiles, the first {wrong[0]} (maximum at '
                                 f'{max_at[wrong[0]].tolist()}, minimum at {min_at[wrong[0]].tolist()}): got '
                                 f'{got[wrong[0]].tolist()}, numpy has {want[wrong[0]].tolist()}')


# ---- b. sq_normalize_tiles --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['normalize', 'normalize-u8'])
def test_normalize_tiles_on_padded_tiles_and_a_pointer_table(name):
    dtype, (n, h, w) = np.dtype(T.NAMED[name][0]), T.NAMED[name][1]
    rng = np.random.default_rng(6)
    stack = (rng.integers(100, 60000, (n, h, w)) if dtype == np.uint16 else rng.integers(10, 250, (n, h, w))).astype(dtype)
    stack[3] = 777 if dtype == np.uint16 else 77            # max == min: 0 / 0 -> 0 like the reference's cast
    want = np.stack([O.normalize_image(tile, dtype.type) for tile in stack])
    guard_value, guard = (0xA5A5 if dtype == np.uint16 else 0xA5), 64
    for src in (base_source(T.named(name, stack)), table_source(T.named_separate(name, stack))):
        mm, mm_dev = tile_minmax(src, n, h, w, dtype)
        np.testing.assert_array_equal(mm, dense_minmax(stack), err_msg=src.label)
        out = _to_device(np.full(guard + n * h * w + guard, guard_value, dtype=dtype))
        status = native.lib().sq_normalize_tiles(src.ptrs, src.base, src.stride, n, h, w, src.pitch, native.sq_dtype_of(dtype),
                                                 mm_dev.data_ptr(), out.data_ptr() + guard * dtype.itemsize, native._stream_ptr())
        assert status == 0, native.lib().sq_last_error().decode()
        got = out.cpu().numpy()
        assert (got[:guard] == guard_value).all() and (got[guard + n * h * w:] == guard_value).all(), f'{src.label}: guards'
        np.testing.assert_array_equal(got[guard:guard + n * h * w].reshape(n, h, w), want, err_msg=src.label)


# ---- c. sq_register_pairs ---------------------------------------------------------------------------------------------------
def register_pairs(src, shape, dtype, mm_dev, pairs, n0, n1, u, norm):
    """sq_register_pairs through the C ABI, as native.register_pairs_async calls it but for the tile arguments."""
    import torch
    L = native.lib()
    n, h, w = shape
    ws = torch.empty(native._size(L.sq_register_workspace_bytes(len(pairs), n0, n1, u), 'workspace'), dtype=torch.uint8, device=_dev())
    pairs_dev = _to_device(np.ascontiguousarray(pairs).view(np.uint8).reshape(-1))
    res = torch.zeros(len(pairs) * native.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=_dev())
    a = native._RegisterArgs()
    a.tile_ptrs_dev, a.tile_base_dev, a.tile_stride = src.ptrs, src.base, src.stride
    a.n_tiles, a.tile_h, a.tile_w, a.tile_pitch, a.tile_dtype = n, h, w, src.pitch, native.sq_dtype_of(dtype)
    a.minmax_dev, a.pairs_dev, a.n_pairs, a.n0, a.n1 = mm_dev.data_ptr(), pairs_dev.data_ptr(), len(pairs), n0, n1
    a.upsample_factor, a.normalization = u, registration.NORMALIZATIONS[norm]
    a.results_dev, a.workspace_dev, a.workspace_bytes = res.data_ptr(), ws.data_ptr(), ws.numel()
    assert L.sq_register_pairs(C.byref(a), native._stream_ptr()) == 0, L.sq_last_error().decode()
    return res.cpu().numpy().view(native.RESULT_DTYPE)


def dense_run(stack, pairs, n0, n1, u, norm, minmax):
    """The run the numerics tests hold to the oracle: the dense stack through the Python binding."""
    tiles = _to_device(stack)
    mm = native.tile_minmax(tiles) if minmax == 'real' else _to_device(R.identity_minmax(len(stack)))
    return native.register_pairs(tiles, mm, pairs, n0, n1, u, registration.NORMALIZATIONS[norm])


def assert_same_bytes(got, want, label):
    assert not (want['coarse'] == np.iinfo(np.int32).min).any()         # the dense run registered every pair
    if got.tobytes() != want.tobytes():
        wrong = [k for k in range(len(want)) if got[k].tobytes() != want[k].tobytes()]
        raise AssertionError(f'{label}: {len(wrong)} of {len(want)} pairs differ from the dense run, the first {wrong[0]}: '
                             f'{got[wrong[0]]} instead of {want[wrong[0]]}')


@pytest.fixture(scope='module')
def batch_u16():
    """12 tiles of 160 x 96, 40 pairs of 128 x 44 crops with origins of their own, and the dense run per normalisation (shared,
    never modified)."""
    n0, n1, u = 128, 44, 10
    stack, pairs, _ = R.batch_inputs(12, 160, 96, n0, n1, 40, np.uint16, seed=91)
    assert (pairs['ref_x0'] % 2 == 1).any() and (pairs['mov_x0'] % 2 == 1).any()
    assert len({(int(p['ref_y0']), int(p['ref_x0'])) for p in pairs}) > 30
    want = {norm: dense_run(stack, pairs, n0, n1, u, norm, 'real') for norm in (None, 'phase')}
    return dict(stack=stack, pairs=pairs, n0=n0, n1=n1, u=u, want=want)


@pytest.mark.parametrize('norm', [None, 'phase'])
@pytest.mark.parametrize('name', ['register-pitch99', 'register-pitch104', 'table'])
def test_register_pairs_on_padded_uint16_tiles_returns_the_bytes_of_the_dense_run(batch_u16, name, norm):
    """rows_forward_block reads the crops through 16-byte loads at any alignment: rows 99 apart (every row-to-row phase), rows
    104 apart behind an offset of 1 (every row one element behind a line), a gap between the tiles, and separately allocated
    tiles; the min-max table comes from sq_tile_minmax on the same layout."""
    b = batch_u16
    stack, shape = b['stack'], b['stack'].shape
    src = table_source(T.named_separate('register-pitch99', stack)) if name == 'table' else base_source(T.named(name, stack))
    mm, mm_dev = tile_minmax(src, *shape, stack.dtype)
    np.testing.assert_array_equal(mm, dense_minmax(stack))
    got = register_pairs(src, shape, stack.dtype, mm_dev, b['pairs'], b['n0'], b['n1'], b['u'], norm)
    assert_same_bytes(got, b['want'][norm], f'{name} {norm}')


@pytest.mark.parametrize('table', [False, True], ids=['pitch53', 'table'])
def test_register_pairs_on_padded_uint8_tiles_returns_the_bytes_of_the_dense_run(table):
    """The scalar pixel path: 10 tiles of 48 x 48 uint8, 32 x 32 crops, rows 53 apart."""
    n0, n1, u, norm = 32, 32, 10, 'phase'
    stack, pairs, _ = R.batch_inputs(10, 48, 48, n0, n1, 40, np.uint8, seed=102)
    assert stack.dtype == np.uint8
    want = dense_run(stack, pairs, n0, n1, u, norm, 'real')
    src = table_source(T.named_separate('register-u8', stack)) if table else base_source(T.named('register-u8', stack))
    mm, mm_dev = tile_minmax(src, *stack.shape, stack.dtype)
    np.testing.assert_array_equal(mm, dense_minmax(stack))
    assert_same_bytes(register_pairs(src, stack.shape, stack.dtype, mm_dev, pairs, n0, n1, u, norm), want, 'uint8')


def test_register_pairs_long_lines_on_padded_tiles_return_the_bytes_of_the_dense_run():
    """8 x 12288 crops, a line in the workspace instead of the LDS, in tiles whose rows are 12291 apart."""
    c = next(c for c in R.SINGLE_CASES if c['name'] == '8x12288')
    d = R.assert_path(c)
    assert d['long1'] and not d['long0']
    stack, pairs = R.single_pair_inputs(c)
    assert stack.shape == T.NAMED['register-long'][1]
    want = dense_run(stack, pairs, c['n0'], c['n1'], c['u'], 'phase', 'identity')
    mm_dev = _to_device(R.identity_minmax(len(stack)))
    for src in (base_source(T.named('register-long', stack)), table_source(T.named_separate('register-long', stack))):
        got = register_pairs(src, stack.shape, stack.dtype, mm_dev, pairs, c['n0'], c['n1'], c['u'], 'phase')
        assert_same_bytes(got, want, f'long lines, {src.label}')


# ---- d. sq_pair_overlap_moments ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['uint16', 'uint8'])
@pytest.mark.parametrize('w', T.MOMENTS_WIDTHS)
def test_pair_overlap_moments_on_padded_tiles_and_a_pointer_table(dtype, w):
    """The five sums of windows 1, 63, 64, 65 and 300 wide (a wave's lanes: one, one short of all, all, one more, several
    rounds) and three rows higher than a band, against numpy's int64 sums of the dense windows."""
    import torch
    name = f'moments-{dtype}-w{w}'
    n, H, W = T.NAMED[name][1]
    band = 16384 // w
    hw = band + 3
    assert hw > band and H - hw == 5 and W - w >= 6
    stack = np.random.default_rng(w).integers(0, np.iinfo(dtype).max + 1, (n, H, W)).astype(dtype)
    stack[0, 2:4, 3:3 + w] = np.iinfo(dtype).max
    windows = np.array([(0, 1, 2, 3, 4, 1, hw, w),                  # crosses the band boundary
                        (2, 0, 5, W - w, 0, 0, hw, w),              # against the far edges of its tiles
                        (1, 1, 0, 0, 0, 0, band, w),                # exactly one band, a tile with itself
                        (1, 2, 1, 2, 3, 4, 1, w),                   # one row
                        (2, 1, 1, 1, 2, 2, hw, 1)],                 # one column
                       dtype=np.int32).view(native.OVERLAP_DTYPE).reshape(-1)
    want = []
    for p in windows:
        a = stack[p['ref_tile']][p['ref_y0']:p['ref_y0'] + p['h'], p['ref_x0']:p['ref_x0'] + p['w']].astype(np.int64)
        b = stack[p['mov_tile']][p['mov_y0']:p['mov_y0'] + p['h'], p['mov_x0']:p['mov_x0'] + p['w']].astype(np.int64)
        assert a.shape == b.shape == (p['h'], p['w'])
        want.append([a.sum(), b.sum(), (a * a).sum(), (b * b).sum(), (a * b).sum()])
    want = np.array(want, dtype=np.int64)
    windows_dev = _to_device(windows.view(np.uint8).reshape(-1))
    for src in (base_source(T.named(name, stack)), table_source(T.named_separate(name, stack))):
        out = torch.full((len(windows) + 1, 5), -7, dtype=torch.int64, device=_dev())
        status = native.lib().sq_pair_overlap_moments(src.ptrs, src.base, src.stride, n, H, W, src.pitch, native.sq_dtype_of(dtype),
                                                      windows_dev.data_ptr(), len(windows), out.data_ptr(), native._stream_ptr())
        assert status == 0, native.lib().sq_last_error().decode()
        got = out.cpu().numpy()
        assert (got[len(windows)] == -7).all(), f'{src.label}: wrote behind the sums'
        np.testing.assert_array_equal(got[:len(windows)], want, err_msg=f'{name} {src.label}')
