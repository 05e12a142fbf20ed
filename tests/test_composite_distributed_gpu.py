"""--composite when several ranks share one region (gloo ranks on cuda:0), by (channel, z) planes and by row bands: every rank
reduces what it writes into a zeroed target, means and counts are summed, rank 0 renders -- and the PNG and JSON bytes are those
of a single process."""
import json
import os
import socket
import sys

import numpy as np
import pytest

import composite_ref as R
from helpers import load_case, spec_of
from image_stitcher_amd import omezarr, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker(rank, world, port, root, extra):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), SQ_DIST_BACKEND='gloo')
    from image_stitcher_amd import stitcher_cli
    stitcher_cli.main(['-i', root, '-r', '--normalization', 'none', *extra])
    import torch.distributed as dist
    dist.destroy_process_group()


def _single(root, extra):
    from image_stitcher_amd import stitcher_cli
    stitcher_cli.main(['-i', root, '-r', '--normalization', 'none', *extra])


def _out(root):
    outs = [d for d in os.listdir(os.path.dirname(root)) if d.startswith('acq_stitched_')]
    assert len(outs) == 1
    return os.path.join(os.path.dirname(root), outs[0], '0_stitched')


def _spec(kind):
    """The specs of tests/test_contrast_distributed_gpu.py."""
    if kind == 'planes':
        # 2 channels x 2 z = 4 planes of a 2100-pixel canvas (2 levels): every rank takes whole planes
        info, _ = load_case('reg_3x4_small')
        spec = spec_of(dict(info, spec=dict(info['spec'], rows=2, cols=2, tile_h=1100, tile_w=1100, ov_y=100, ov_x=100)))
        return spec, ['--registration-channel', info['params']['registration_channel'], '--registration-z-level', '1']
    # one plane, a 4343-row canvas with 3 levels: bands of 512 * 4 = 2048 level-0 rows are dealt over the ranks
    info, _ = load_case('reg_2x2_2048')
    return spec_of(info), ['--zarr-compression', 'none']


@pytest.mark.parametrize('projection', [False, True])
@pytest.mark.parametrize('kind,world', [('planes', 2), ('planes', 3), ('bands', 2), ('bands', 3)])
def test_ranks_write_the_picture_of_one_process(tmp_path, kind, world, projection):
    import torch.multiprocessing as mp
    spec, extra = _spec(kind)
    extra = [*extra, '--composite', '--composite-max-side', '300', *(['--z-projection', 'max'] if projection else [])]
    roots = {k: str(tmp_path / k / 'acq') for k in ('one', 'ranks')}
    for r in roots.values():
        synth.write_acquisition(spec, r)
    _single(roots['one'], extra)
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(world, port, roots['ranks'], extra), nprocs=world, join=True)
    one, ranks = _out(roots['one']), _out(roots['ranks'])
    stem = 'R0_stitched_mip' if projection else 'R0_stitched'
    names = sorted(f for f in os.listdir(ranks) if '_composite' in f)
    assert names == [stem + '_composite.json', stem + '_composite.png'] == sorted(f for f in os.listdir(one) if '_composite' in f)
    for name in names:
        with open(os.path.join(one, name), 'rb') as fa, open(os.path.join(ranks, name), 'rb') as fb:
            assert fa.read() == fb.read(), name
    # ... and that picture is the definition applied to level 0 of the store the ranks wrote together
    with open(os.path.join(ranks, stem + '_composite.json')) as fh:
        meta = json.load(fh)
    level0 = omezarr.read_array(os.path.join(ranks, stem + '.ome.zarr', '0'))
    with open(os.path.join(ranks, stem + '.ome.zarr', '.zattrs')) as fh:
        colors = [int(ch['color'], 16) for ch in json.load(fh)['omero']['channels']]
    z = meta['source']['z']
    assert z == (None if projection else level0.shape[2] // 2)
    want, k, windows = R.composite(level0[0, :, 0 if z is None else z], colors, 300)
    assert k >= 3 and meta['level'] == k and [(c['window']['start'], c['window']['end']) for c in meta['channels']] == windows
    with open(os.path.join(ranks, stem + '_composite.png'), 'rb') as fh:
        np.testing.assert_array_equal(R.decode_png(fh.read()), want)
    assert len(np.unique(want)) >= 16
