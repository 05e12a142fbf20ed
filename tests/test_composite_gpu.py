"""--composite on the GPU: sq_block_mean and sq_composite_render against the numpy definition (tests/composite_ref.py), and the
option end to end through stitcher_cli.main on golden acquisitions.  Every comparison is equality."""
import hashlib
import json
import os

import numpy as np
import pytest

import composite_ref as R
from helpers import load_case, spec_of
from image_stitcher_amd import native, omezarr, stitcher_cli, synth

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _random(rng, dtype, shape):
    """Values that exercise the sums: mostly mid-range, with runs of the dtype's extremes."""
    top = int(np.iinfo(dtype).max)
    a = rng.integers(0, top + 1, shape).astype(dtype)
    a[..., : shape[-1] // 3] = top
    a[..., shape[-2] // 2:, shape[-1] // 2:] //= 7
    return a


# ------------------------------------------------------------------------------------------------ sq_block_mean
@pytest.mark.parametrize('dtype', [np.uint8, np.uint16])
@pytest.mark.parametrize('k', range(9))
def test_block_mean_every_level(dtype, k):
    """Several planes, H and W with partial blocks at every k, rows wider than one wave's kilobyte."""
    rng = np.random.default_rng(100 + k)
    src = _random(rng, dtype, (3, 523, 1301))
    got = native.block_mean(_dev(src), k).cpu().numpy()
    np.testing.assert_array_equal(got, R.block_mean(src, k))
    if k == 0:
        np.testing.assert_array_equal(got, src)


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16])
@pytest.mark.parametrize('shape', [(1, 1), (1, 300), (300, 1), (7, 9), (256, 256), (257, 255), (512, 1024), (1025, 2049)])
def test_block_mean_shapes(dtype, shape):
    rng = np.random.default_rng(7)
    src = _random(rng, dtype, (2,) + shape)
    for k in (0, 1, 3, 4, 8):
        np.testing.assert_array_equal(native.block_mean(_dev(src), k).cpu().numpy(), R.block_mean(src, k), err_msg=f'k={k}')


def test_block_mean_saturated_blocks_do_not_overflow():
    """A full 256 x 256 block of 65535 sums to 65535 * 65536 < 2^32."""
    src = np.full((1, 512, 300), 65535, np.uint16)
    np.testing.assert_array_equal(native.block_mean(_dev(src), 8).cpu().numpy(), np.full((1, 2, 2), 65535, np.uint16))


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16])
@pytest.mark.parametrize('k', [0, 1, 2, 4, 5, 8])
def test_block_mean_sliced_views(dtype, k):
    """Odd element offset, padded pitch, strided planes; a padded destination is written only inside the image."""
    import torch
    rng = np.random.default_rng(11 + k)
    big = _random(rng, dtype, (5, 300, 777))
    dbig = _dev(big)
    view = dbig[0:5:2, 3:290, 5:600]                   # every other plane, pitch 777, first element at an odd offset
    want = R.block_mean(big[0:5:2, 3:290, 5:600], k)
    np.testing.assert_array_equal(native.block_mean(view, k).cpu().numpy(), want)
    canvas = torch.full((4, want.shape[1] + 3, want.shape[2] + 5), 77, dtype=dbig.dtype, device='cuda')
    out = canvas[1:4, 1:1 + want.shape[1], 3:3 + want.shape[2]]
    native.block_mean(view, k, out=out)
    got = canvas.cpu().numpy()
    np.testing.assert_array_equal(got[1:4, 1:1 + want.shape[1], 3:3 + want.shape[2]], want)
    got[1:4, 1:1 + want.shape[1], 3:3 + want.shape[2]] = 77
    assert (got == 77).all()


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16])
@pytest.mark.parametrize('k', [0, 2, 4, 6])
def test_block_mean_row_bands(dtype, k):
    """Bands that start on multiples of f (the last one runs to H): stitched into one zeroed output they equal the whole plane,
    whether the band is a view of the whole plane (rows=) or a buffer of its own (out= a row slice)."""
    import torch
    rng = np.random.default_rng(23)
    src = _random(rng, dtype, (2, 1000, 900))
    d = _dev(src)
    want = R.block_mean(src, k)
    f = 1 << k
    cuts = [0, 128, 512, 832, 1000]
    out = torch.zeros(want.shape, dtype=d.dtype, device='cuda')
    for y0, y1 in zip(cuts[:-1], cuts[1:]):
        got = native.block_mean(d, k, out=out, rows=(y0, y1))
        assert got is out
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    out2 = torch.zeros(want.shape, dtype=d.dtype, device='cuda')
    for y0, y1 in zip(cuts[:-1], cuts[1:]):
        band = d[:, y0:y1].contiguous()
        native.block_mean(band, k, out=out2[:, y0 // f:y0 // f + -(-(y1 - y0) // f)])
    np.testing.assert_array_equal(out2.cpu().numpy(), want)
    one = native.block_mean(d, k, rows=(128, 512)).cpu().numpy()      # a fresh output: zero outside the band
    np.testing.assert_array_equal(one[:, 128 // f:512 // f], want[:, 128 // f:512 // f])
    assert not one[:, :128 // f].any() and not one[:, 512 // f:].any()
    with pytest.raises(ValueError):
        native.block_mean(d, 4, rows=(8, 512))
    with pytest.raises(ValueError):
        native.block_mean(d, 4, rows=(0, 500))
    with pytest.raises(ValueError):
        native.block_mean(d, 9)


# ------------------------------------------------------------------------------------------------ sq_composite_render
@pytest.mark.parametrize('dtype', [np.uint8, np.uint16])
def test_composite_render(dtype):
    import torch
    rng = np.random.default_rng(3)
    top = int(np.iinfo(dtype).max)
    means = rng.integers(0, top + 1, (5, 67, 131)).astype(dtype)
    windows = [(0, top), (top // 5, top // 2), (3, 4), (top - 1, top), (top // 3, top // 3 + 97)]
    colors = [0x0000FF, 0x00FF00, 0xFFCF00, 0xFF0000, 0x770000]
    want = R.render(means, windows, colors)
    got = native.composite_render(_dev(means), windows, colors).cpu().numpy()
    np.testing.assert_array_equal(got, want)
    # the additive sum saturates: white on white
    sat = R.render(means[:3], [(0, max(1, top // 4))] * 3, [0xFFFFFF] * 3)
    assert (sat == 255).mean() > 0.5 and (sat < 255).any()
    np.testing.assert_array_equal(native.composite_render(_dev(means[:3]), [(0, max(1, top // 4))] * 3, [0xFFFFFF] * 3).cpu().numpy(), sat)
    # a padded destination and strided planes: nothing outside the image is written
    canvas = torch.full((70, 140, 3), 9, dtype=torch.uint8, device='cuda')
    planes = _dev(rng.integers(0, top + 1, (5, 80, 150)).astype(dtype))
    view = planes[1:5:2, 2:69, 7:138]
    native.composite_render(view, windows[:2], colors[:2], out=canvas[2:69, 5:136])
    g = canvas.cpu().numpy()
    np.testing.assert_array_equal(g[2:69, 5:136], R.render(view.cpu().numpy(), windows[:2], colors[:2]))
    g[2:69, 5:136] = 9
    assert (g == 9).all()
    with pytest.raises(ValueError):
        native.composite_render(_dev(means), windows[:4], colors)
    with pytest.raises(ValueError):
        native.composite_render(_dev(means[:1]), [(5, 5)], [0xFFFFFF])
    with pytest.raises(ValueError):
        native.composite_render(_dev(np.zeros((17, 4, 4), dtype)), [(0, 1)] * 17, [0] * 17)


# ------------------------------------------------------------------------------------------------ end to end
TWO_CHANNELS = ('Fluorescence 488 nm Ex', 'Fluorescence 561 nm Ex')
# (golden acquisition, channels, --composite-max-side): max_side gives k = 2 on every one of these canvases.  reg_uint8 and
# reg_multi have ONE channel (488 nm: pure green), whose picture can vary in one colour component only; the non-degeneracy
# condition below asks for two, so they are written with a second channel (561 nm: 0xFFCF00) -- the condition is kept, the case
# is replaced by its two-channel variant (same grid, tiles, overlaps, regions and timepoints).  Checked on the CPU with the
# numpy definition on the oracle's canvases: at least 58 distinct values in two components, at most 34 % extreme pixels.
CASES = {'reg_3x4_small': (None, 128), 'reg_uint8': (TWO_CHANNELS, 100), 'coord_rgb': (None, 64), 'reg_multi': (TWO_CHANNELS, 100)}


def _acquisition(case, root):
    info, _ = load_case(case)
    channels, max_side = CASES[case]
    sp = dict(info['spec'])
    if channels:
        sp['channels'] = list(channels)
    spec = spec_of(dict(info, spec=sp))
    synth.write_acquisition(spec, root)
    p = info['params']
    base = ['-r'] if p['use_registration'] else []
    if p['registration_channel']:
        base += ['--registration-channel', p['registration_channel']]
    if p['registration_z_level']:
        base += ['--registration-z-level', str(p['registration_z_level'])]
    return spec, base, max_side


def _run(root, *extra):
    stitcher_cli.main(['-i', root, '--normalization', 'none', *extra])
    base = os.path.dirname(root)
    outs = [d for d in os.listdir(base) if d.startswith(os.path.basename(root) + '_stitched_')]
    assert len(outs) == 1
    return os.path.join(base, outs[0])


def _files(folder):
    out = {}
    for d, _, names in os.walk(folder):
        for n in names:
            with open(os.path.join(d, n), 'rb') as fh:
                out[os.path.relpath(os.path.join(d, n), folder)] = hashlib.sha256(fh.read()).hexdigest()
    return out


def _level0(path):
    """Level 0 of a store (TCZYX) as written: .ome.zarr through omezarr.read_array, .ome.tiff through the package's test reader (planes in C, Z order)."""
    if path.endswith('.zarr'):
        return omezarr.read_array(os.path.join(path, '0'))
    import re
    from image_stitcher_amd.ometiff import read_ome_tiff
    planes, xml = read_ome_tiff(path)
    c, z = (int(re.search(f'Size{d}="(\\d+)"', xml).group(1)) for d in 'CZ')
    return np.stack(planes).reshape((1, c, z) + planes[0].shape)


def _check_region(out, t, region, *, kind, z, max_side, fmt='.ome.zarr', names=None, lo=0.1, hi=99.9, demand_contrast=True):
    """One region's PNG and sidecar against the definition applied to level 0 of the store the sidecar names."""
    tag = '' if kind == 'stack' else '_' + kind
    folder = os.path.join(out, f'{t}_stitched')
    stem = os.path.join(folder, f'{region}_stitched{tag}_composite')
    with open(stem + '.json') as fh:
        meta = json.load(fh)
    assert meta['source'] == {'store': f'{region}_stitched{tag}{fmt}', 'kind': kind, 'z': z}
    store = os.path.join(folder, meta['source']['store'])
    a = _level0(store)
    if fmt.endswith('.zarr'):
        with open(os.path.join(store, '.zattrs')) as fh:
            channels = json.load(fh)['omero']['channels']
        labels = [ch['label'] for ch in channels]
        colors = [int(ch['color'], 16) for ch in channels]
    else:
        from image_stitcher_amd.stitcher import Stitcher
        labels = names['all']
        colors = [Stitcher.get_channel_color(None, n) for n in labels]
    use = (names or {}).get('use') or labels
    idx = [labels.index(n) for n in use]
    src = a[0, idx, 0 if z is None else z]
    want, k, windows = R.composite(src, [colors[i] for i in idx], max_side, lo, hi)
    assert k >= 1
    with open(stem + '.png', 'rb') as fh:
        got = R.decode_png(fh.read())
    np.testing.assert_array_equal(got, want)
    assert meta['level'] == k and meta['factor'] == 1 << k and meta['shape'] == list(want.shape[:2])
    assert meta['source_shape'] == list(src.shape[1:]) and meta['percentiles'] == [lo, hi]
    assert meta['channels'] == [{'label': labels[i], 'color': f'{colors[i]:06X}', 'window': {'start': w[0], 'end': w[1]}}
                                for i, w in zip(idx, windows)]
    if demand_contrast:      # the case is not degenerate: a picture with structure in at least two colour components
        assert sum(len(np.unique(want[..., j])) >= 16 for j in range(3)) >= 2
        assert np.all((want == 0) | (want == 255), axis=2).mean() < 0.5
    return meta, a


@pytest.mark.parametrize('case', sorted(CASES))
def test_golden_acquisitions_plain_stack(tmp_path, case):
    """The plain stack, default z: every (timepoint, region) gets its picture; without the flag no _composite file appears and
    every other output file is byte-identical."""
    roots = {k: str(tmp_path / k / 'acq') for k in ('on', 'off')}
    for r in roots.values():
        spec, base, max_side = _acquisition(case, r)
    out = _run(roots['on'], *base, '--composite', '--composite-max-side', str(max_side))
    ref = _run(roots['off'], *base)
    n = 0
    for t in range(spec.nt):
        for region in spec.regions:
            _check_region(out, t, region, kind='stack', z=spec.nz // 2, max_side=max_side)
            n += 1
    on, off = _files(out), _files(ref)
    assert not [f for f in off if '_composite' in f]
    assert sorted(f for f in on if '_composite' in f) == sorted(
        os.path.join(f'{t}_stitched', f'{region}_stitched_composite{ext}')
        for t in range(spec.nt) for region in spec.regions for ext in ('.png', '.json'))
    assert {f: h for f, h in on.items() if '_composite' not in f} == off and len(off) > 4 and n >= 1


def test_explicit_z_and_channel_subset(tmp_path):
    root = str(tmp_path / 'acq')
    spec, base, max_side = _acquisition('reg_3x4_small', root)
    use = [spec.channels[1], spec.channels[0]]      # permuted
    out = _run(root, *base, '--composite', '--composite-max-side', str(max_side), '--composite-z', '0',
               '--composite-channels', *use)
    meta, _ = _check_region(out, 0, 'R0', kind='stack', z=0, max_side=max_side, names={'use': use})
    assert [c['label'] for c in meta['channels']] == use


def test_rgb_channel_subset(tmp_path):
    root = str(tmp_path / 'acq')
    spec, base, max_side = _acquisition('coord_rgb', root)
    use = ['Fluorescence 488 nm Ex', 'BF LED matrix full_B', 'BF LED matrix full_R']
    out = _run(root, *base, '--composite', '--composite-max-side', str(max_side), '--composite-channels', *use)
    _check_region(out, 0, 'R0', kind='stack', z=0, max_side=max_side, names={'use': use})


@pytest.mark.parametrize('extra,kind', [(['--z-projection', 'max'], 'mip'), (['--z-projection', 'max-only'], 'mip'),
                                        (['--z-projection', 'focus-only', '--focus-guide-channel', 'Fluorescence 488 nm Ex'], 'edf')])
def test_projection_is_the_source(tmp_path, extra, kind):
    roots = {k: str(tmp_path / k / 'acq') for k in ('on', 'off')}
    for r in roots.values():
        spec, base, max_side = _acquisition('reg_3x4_small', r)
    out = _run(roots['on'], *base, *extra, '--composite', '--composite-max-side', str(max_side))
    ref = _run(roots['off'], *base, *extra)
    _check_region(out, 0, 'R0', kind=kind, z=None, max_side=max_side)
    on, off = _files(out), _files(ref)
    assert sorted(f for f in on if '_composite' in f) == [os.path.join('0_stitched', f'R0_stitched_{kind}_composite{e}')
                                                          for e in ('.json', '.png')]
    assert {f: h for f, h in on.items() if '_composite' not in f} == off


def test_percentile_windows_of_the_projection_store_are_the_sidecars(tmp_path):
    """--contrast-limits percentile and a projection: the store's own counts serve the composite; the windows agree."""
    roots = {k: str(tmp_path / k / 'acq') for k in ('on', 'off')}
    for r in roots.values():
        spec, base, max_side = _acquisition('reg_3x4_small', r)
    extra = ['--z-projection', 'max', '--contrast-limits', 'percentile', '--contrast-percentiles', '1', '99']
    out = _run(roots['on'], *base, *extra, '--composite', '--composite-max-side', str(max_side))
    ref = _run(roots['off'], *base, *extra)
    meta, _ = _check_region(out, 0, 'R0', kind='mip', z=None, max_side=max_side, lo=1.0, hi=99.0)
    with open(os.path.join(out, '0_stitched', 'R0_stitched_mip.ome.zarr', '.zattrs')) as fh:
        channels = json.load(fh)['omero']['channels']
    assert [c['window'] for c in meta['channels']] == [{'start': ch['window']['start'], 'end': ch['window']['end']} for ch in channels]
    assert all(ch['window']['end'] < 65535 for ch in channels)
    on, off = _files(out), _files(ref)
    assert {f: h for f, h in on.items() if '_composite' not in f} == off


@pytest.mark.parametrize('extra,fmt', [(['--fusion-mode', 'feather'], '.ome.zarr'), (['--output-format', '.ome.tiff'], '.ome.tiff'),
                                       (['--output-format', '.ome.tiff', '--z-projection', 'max'], '.ome.tiff')])
def test_other_modes_and_formats(tmp_path, extra, fmt):
    roots = {k: str(tmp_path / k / 'acq') for k in ('on', 'off')}
    for r in roots.values():
        spec, base, max_side = _acquisition('reg_3x4_small', r)
    out = _run(roots['on'], *base, *extra, '--composite', '--composite-max-side', str(max_side))
    ref = _run(roots['off'], *base, *extra)
    proj = '--z-projection' in extra
    _check_region(out, 0, 'R0', kind='mip' if proj else 'stack', z=None if proj else 1, max_side=max_side, fmt=fmt,
                  names={'all': list(spec.channels)})
    on, off = _files(out), _files(ref)
    assert {f: h for f, h in on.items() if '_composite' not in f} == off and len(off) >= 1


def test_refusals_at_metadata_time(tmp_path):
    from image_stitcher_amd.stitcher import Stitcher
    root = str(tmp_path / 'acq')
    spec, base, _ = _acquisition('reg_3x4_small', root)
    params = lambda: stitcher_cli.create_params(stitcher_cli.parse_args(['-i', root]))
    for kw, word in ((dict(composite_z=2), 'composite_z'), (dict(composite_channels=['nope']), 'composite_channels')):
        st = Stitcher(params(), composite=True, **kw)
        with pytest.raises(ValueError, match=word):
            st.run()
    st = Stitcher(params(), composite=True, composite_max_side=16)      # the smallest side allowed: blocks of 32 or more
    st.run()
    with open(os.path.join(st.output_folder, '0_stitched', 'R0_stitched_composite.json')) as fh:
        meta = json.load(fh)
    assert meta['level'] == R.choose_level(*meta['source_shape'], 16) >= 5 and max(meta['shape']) <= 16
