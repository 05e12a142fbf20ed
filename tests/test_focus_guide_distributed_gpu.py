"""--focus-guide-channel / --focus-depth-map when several ranks share one region (gloo ranks on cuda:0): the (channel, row band)
units are dealt over the ranks, a follower's rank computes the guide's depth of its band itself, and the stores equal the ones
a single process writes."""
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


def _store(path):
    levels = sorted(int(d) for d in os.listdir(path) if d.isdigit())
    return [omezarr.read_array(os.path.join(path, str(lv))) for lv in levels]


@pytest.mark.parametrize('name,world,guide,extra', [
    # 2 channels x 2 z: each rank projects one whole channel; the follower's rank projects the guide too
    ('reg_3x4_small', 2, 1, ['--registration-z-level', '1', '--z-projection', 'focus']),
    ('reg_3x4_small', 3, 0, ['--registration-z-level', '1', '--z-projection', 'focus-only']),
    # one channel, a 4343-row canvas with 3 pyramid levels: row bands; the guide is the only channel
    ('reg_2x2_2048', 2, 0, ['--zarr-compression', 'none', '--z-projection', 'focus-only', '--focus-radius', '5']),
    ('reg_2x2_2048', 3, 0, ['--zarr-compression', 'none', '--z-projection', 'focus-only', '--focus-radius', '5']),
])
def test_ranks_write_what_one_rank_writes(tmp_path, name, world, guide, extra):
    import torch.multiprocessing as mp
    info, _ = load_case(name)
    if info['params']['registration_channel']:
        extra = ['--registration-channel', info['params']['registration_channel'], *extra]
    spec = spec_of(info)
    extra = [*extra, '--focus-guide-channel', list(spec.channels)[guide], '--focus-depth-map']
    roots = {k: str(tmp_path / k / 'acq') for k in ('one', 'ranks')}
    for r in roots.values():
        synth.write_acquisition(spec, r)
    _single(roots['one'], extra)
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(world, port, roots['ranks'], extra), nprocs=world, join=True)
    one, ranks = _out(roots['one']), _out(roots['ranks'])
    for store in ('R0_stitched_edf.ome.zarr', 'R0_stitched_depth.ome.zarr'):
        want, got = _store(os.path.join(one, store)), _store(os.path.join(ranks, store))
        assert len(want) == len(got) >= 1 and want[0].shape[2] == 1
        for a, b in zip(want, got):
            np.testing.assert_array_equal(a, b)
        assert want[0].any()
        with open(os.path.join(one, store, '.zattrs')) as fa, open(os.path.join(ranks, store, '.zattrs')) as fb:
            assert fa.read() == fb.read()
    assert _store(os.path.join(one, 'R0_stitched_depth.ome.zarr'))[0].shape[1] == 1
