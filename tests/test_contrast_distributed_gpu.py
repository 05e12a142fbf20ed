"""--contrast-limits percentile when several ranks share one region (gloo ranks on cuda:0): whether the (channel, z) planes are
dealt over the ranks or one plane is cut into row bands, every rank counts what it writes, the counts are summed, and rank 0
writes the sidecars and windows a single process writes."""
import json
import os
import socket
import sys

import numpy as np
import pytest

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
    if kind == 'planes':
        # 2 channels x 2 z = 4 planes of a 2100-pixel canvas (2 levels): every rank takes whole planes
        info, _ = load_case('reg_3x4_small')
        spec = spec_of(dict(info, spec=dict(info['spec'], rows=2, cols=2, tile_h=1100, tile_w=1100, ov_y=100, ov_x=100)))
        return spec, ['--registration-channel', info['params']['registration_channel'], '--registration-z-level', '1']
    # one plane, a 4343-row canvas with 3 levels: bands of 512 * 4 = 2048 level-0 rows are dealt over the ranks
    info, _ = load_case('reg_2x2_2048')
    return spec_of(info), ['--zarr-compression', 'none']


@pytest.mark.parametrize('kind,world', [('planes', 2), ('planes', 3), ('bands', 2), ('bands', 3)])
def test_ranks_write_the_sidecars_of_one_process(tmp_path, kind, world):
    import torch.multiprocessing as mp
    spec, extra = _spec(kind)
    extra = [*extra, '--z-projection', 'max', '--contrast-limits', 'percentile']
    roots = {k: str(tmp_path / k / 'acq') for k in ('one', 'ranks')}
    for r in roots.values():
        synth.write_acquisition(spec, r)
    _single(roots['one'], extra)
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(world, port, roots['ranks'], extra), nprocs=world, join=True)
    one, ranks = _out(roots['one']), _out(roots['ranks'])
    for stem in ('R0_stitched', 'R0_stitched_mip'):
        for tail in ('_histogram.npy', '_stats.json', '.ome.zarr/.zattrs'):
            with open(os.path.join(one, stem + tail), 'rb') as fa, open(os.path.join(ranks, stem + tail), 'rb') as fb:
                assert fa.read() == fb.read(), stem + tail
        level0 = omezarr.read_array(os.path.join(ranks, stem + '.ome.zarr', '0'))
        hist = np.load(os.path.join(ranks, stem + '_histogram.npy'))
        with open(os.path.join(ranks, stem + '.ome.zarr', '.zattrs')) as fh:
            channels = json.load(fh)['omero']['channels']
        for c in range(level0.shape[1]):
            want = np.bincount(level0[:, c].ravel(), minlength=65536)
            assert want[1:].any()
            np.testing.assert_array_equal(hist[c], want, err_msg=f'{stem} channel {c}')
            w = channels[c]['window']
            assert (w['start'], w['end']) == omezarr.contrast_window(want, 0.1, 99.9, 65535) != (0, 65535)
    stack = omezarr.read_array(os.path.join(ranks, 'R0_stitched.ome.zarr', '0'))
    assert (stack.shape[1] * stack.shape[2] >= world) == (kind == 'planes')      # bands: fewer planes than ranks
