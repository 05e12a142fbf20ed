"""--pyramid-method mean without a GPU: the definition against the vectors dask's coarsen produced
(tests/golden/make_golden_pyramid_mean.py), the property the one-pass kernel relies on, the store metadata and the
interface."""
import json
import os
import re

import numpy as np
import pytest

from helpers import GOLDEN
from image_stitcher_amd import native, omezarr, stitcher_cli
from image_stitcher_amd.stitcher import Stitcher
from image_stitcher_amd.stitcher_parameters import StitchingParameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mean_level(a):
    """The definition: the truncated 2 x 2 mean over the last two axes, a trailing odd row / column dropped."""
    h, w = a.shape[-2] // 2 * 2, a.shape[-1] // 2 * 2
    s = a[..., 0:h:2, 0:w:2].astype(np.uint32) + a[..., 0:h:2, 1:w:2] + a[..., 1:h:2, 0:w:2] + a[..., 1:h:2, 1:w:2]
    return (s >> 2).astype(a.dtype)


def mean_pyramid(a, n_levels):
    """[a, level 1, ...]: at most n_levels arrays, ending where the next level would be empty."""
    out = [a]
    while len(out) < n_levels and out[-1].shape[-2] >= 2 and out[-1].shape[-1] >= 2:
        out.append(mean_level(out[-1]))
    return out


def one_pass(a, n):
    """Levels 1..n from the 2^n x 2^n blocks of level 0 alone, the way a workgroup that sees only its strip makes them."""
    step = 1 << n
    hb, wb = a.shape[0] // step, a.shape[1] // step
    block = a[:hb * step, :wb * step].reshape(hb, step, wb, step).transpose(0, 2, 1, 3)      # [hb, wb, step, step]
    out = []
    for _ in range(n):
        block = mean_level(block)
        k = block.shape[-1]
        out.append(block.transpose(0, 2, 1, 3).reshape(hb * k, wb * k))
    return out


def _vectors():
    v = np.load(os.path.join(GOLDEN, 'pyramid_mean_vectors.npz'))
    cases = {}
    for key in v.files:
        if key.startswith('in_'):
            name = key[3:]
            levels = [v[key]]
            while f'l{len(levels)}_{name}' in v.files:
                levels.append(v[f'l{len(levels)}_{name}'])
            cases[name] = levels
    return cases


def test_restatement_reproduces_the_coarsen_vectors():
    cases = _vectors()
    assert len(cases) >= 12
    deepest = 0
    for name, levels in cases.items():
        got = mean_pyramid(levels[0], 99)
        assert len(got) == len(levels), name
        for lv, (g, w) in enumerate(zip(got, levels)):
            assert g.dtype == w.dtype and g.shape == w.shape, (name, lv)
            np.testing.assert_array_equal(g, w, err_msg=f'{name} level {lv}')
        deepest = max(deepest, len(levels) - 1)
    assert deepest >= 5
    # the 18-bit sum: four saturated voxels stay saturated
    assert (cases['all_65535'][1] == 65535).all() and (cases['all_255'][1] == 255).all()


def test_levels_depend_only_on_their_block_of_level_0():
    """What the one-pass kernel relies on: level l at (y, x) is a function of the 2^l x 2^l block of level 0 at (y << l, x << l)
    -- the chain over the whole image and the reduction block by block agree wherever the block lies inside level 0, and
    that is every voxel of every level."""
    rng = np.random.default_rng(5)
    for name, levels in _vectors().items():
        a = levels[0]
        for n in range(1, len(levels)):
            got = one_pass(a, n)
            for lv in range(1, n + 1):
                want = levels[lv]
                hb, wb = (a.shape[0] >> n) << (n - lv), (a.shape[1] >> n) << (n - lv)
                np.testing.assert_array_equal(got[lv - 1], want[:hb, :wb], err_msg=f'{name} n={n} level {lv}')
            # the deepest level of the request is covered completely: floor-halving n times = floor(size / 2^n)
            assert got[n - 1].shape == levels[n].shape
    for dtype in ('uint8', 'uint16'):
        a = rng.integers(0, np.iinfo(dtype).max + 1, (203, 330)).astype(dtype)
        chain = mean_pyramid(a, 6)
        for lv in range(1, 6):
            np.testing.assert_array_equal(one_pass(a, lv)[lv - 1], chain[lv])


@pytest.mark.parametrize('shape', [(37, 53), (64, 96), (5, 2), (131, 70), (2, 2), (1, 40), (36428, 29108)])
def test_level_shapes_are_those_of_the_store(shape):
    shapes = omezarr.level_shapes((1, 1, 1) + shape, 8)
    if shape[0] * shape[1] < 1 << 20:
        got = mean_pyramid(np.zeros(shape, np.uint8), 8)
        assert [g.shape for g in got] == [s[3:] for s in shapes]
    for lv, s in enumerate(shapes):
        assert s[3:] == (shape[0] >> lv, shape[1] >> lv)


def test_cli_flag():
    assert stitcher_cli.parse_args(['-i', 'x']).pyramid_method == 'nearest'
    assert stitcher_cli.parse_args(['-i', 'x', '--pyramid-method', 'mean']).pyramid_method == 'mean'
    assert stitcher_cli.parse_args(['-i', 'x', '--pyramid-method', 'nearest']).pyramid_method == 'nearest'
    with pytest.raises(SystemExit):
        stitcher_cli.parse_args(['-i', 'x', '--pyramid-method', 'gaussian'])
    flag = [kw for names, kw in stitcher_cli.FLAGS if names == ('--pyramid-method',)]
    assert len(flag) == 1 and flag[0]['choices'] == ['nearest', 'mean'] and '.ome.tiff' in flag[0]['help']


def test_stitcher_rejects_other_methods(tmp_path):
    params = StitchingParameters(input_folder=str(tmp_path))
    assert Stitcher(params).pyramid_method == 'nearest'
    assert Stitcher(params, pyramid_method='mean').pyramid_method == 'mean'
    for bad in ('gaussian', 'Mean', None, ''):
        with pytest.raises(ValueError, match='pyramid_method'):
            Stitcher(params, pyramid_method=bad)
    with pytest.raises(ValueError, match='pyramid_method'):
        omezarr.create_store(str(tmp_path / 'x.ome.zarr'), (1, 1, 1, 8, 8), np.uint16, pixel_size_um=1.0, pyramid_method='box')
    assert not os.path.exists(str(tmp_path / 'x.ome.zarr'))


def _expected_default_attrs(name, px, dz, n_levels, channel_names, colors, vmax):
    """.zattrs of a store as every commit so far has written it, from the documented keys (NGFF 0.4 multiscales + omero)."""
    return {
        'multiscales': [{
            'version': '0.4', 'name': name,
            'axes': [{'name': 't', 'type': 'time', 'unit': 'second'}, {'name': 'c', 'type': 'channel'},
                     {'name': 'z', 'type': 'space', 'unit': 'micrometer'},
                     {'name': 'y', 'type': 'space', 'unit': 'micrometer'},
                     {'name': 'x', 'type': 'space', 'unit': 'micrometer'}],
            'datasets': [{'path': str(lv), 'coordinateTransformations': [
                {'type': 'scale', 'scale': [1, 1, dz, px * 2 ** lv, px * 2 ** lv]}]} for lv in range(n_levels)]}],
        'omero': {'id': 1, 'name': name, 'version': '0.4', 'channels': [
            {'label': n, 'color': f'{c:06X}', 'window': {'start': 0, 'end': vmax, 'min': 0, 'max': vmax},
             'active': True, 'coefficient': 1, 'family': 'linear'} for n, c in zip(channel_names, colors)]},
    }


def test_default_store_metadata_is_unchanged_and_mean_adds_two_keys(tmp_path):
    kw = dict(pixel_size_um=0.752, dz_um=1.5, channel_names=['405', '561'], channel_colors=[0x3300FF, 0xFFCF00], num_levels=3,
              name='R0_t0', compression='blosc')
    want = _expected_default_attrs('R0_t0', 0.752, 1.5, 3, ['405', '561'], [0x3300FF, 0xFFCF00], 65535)
    paths = {k: str(tmp_path / f'{k}.ome.zarr') for k in ('default', 'nearest', 'mean')}
    shapes = omezarr.create_store(paths['default'], (1, 2, 3, 100, 141), np.uint16, **kw)
    assert omezarr.create_store(paths['nearest'], (1, 2, 3, 100, 141), np.uint16, pyramid_method='nearest', **kw) == shapes
    assert omezarr.create_store(paths['mean'], (1, 2, 3, 100, 141), np.uint16, pyramid_method='mean', **kw) == shapes
    raw = {k: open(os.path.join(p, '.zattrs'), 'rb').read() for k, p in paths.items()}
    assert raw['default'] == json.dumps(want, indent=1).encode()       # the bytes, not only the content
    assert raw['nearest'] == raw['default']
    ms = json.loads(raw['default'])['multiscales'][0]
    assert 'type' not in ms and 'metadata' not in ms
    mean = json.loads(raw['mean'])
    mm = mean['multiscales'][0]
    assert set(mm) - set(ms) == {'type', 'metadata'} and mm['type'] == 'mean'
    assert isinstance(mm['metadata'], dict) and 'method' in mm['metadata'] and '>> 2' in json.dumps(mm['metadata'])
    del mm['type'], mm['metadata']
    assert mean == want
    # layout, chunk grid and array metadata do not depend on the method
    for lv in range(3):
        assert open(os.path.join(paths['mean'], str(lv), '.zarray'), 'rb').read() == \
            open(os.path.join(paths['default'], str(lv), '.zarray'), 'rb').read()


def test_entry_point_is_exported_and_declared():
    assert 'sq_pyramid_mean' in native.EXPORTS
    with open(os.path.join(ROOT, 'include', 'squidstitch.h')) as fh:
        header = fh.read()
    assert re.search(r'\bint\s+sq_pyramid_mean\s*\(', header)
    assert 'zarr_stitcher.py:614-719' in header
    m = re.search(r'#define\s+SQ_PYRAMID_MEAN_MAX_LEVELS\s+(\d+)', header)
    assert m and int(m.group(1)) == native.SQ_PYRAMID_MEAN_MAX_LEVELS >= 5
    assert callable(native.pyramid_mean)
