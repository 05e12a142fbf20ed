"""--pyramid-method mean when several ranks share one region (gloo ranks on cuda:0): whether the (channel, z) planes are dealt
over the ranks or one plane is cut into row bands, the store has the same arrays at every level as the one a single process
writes, and every level is the truncated 2 x 2 mean of the one before."""
import os
import socket
import sys

import numpy as np
import pytest

from helpers import load_case, spec_of
from image_stitcher_amd import omezarr, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mean_level(a):
    h, w = a.shape[-2] // 2 * 2, a.shape[-1] // 2 * 2
    s = a[..., 0:h:2, 0:w:2].astype(np.uint32) + a[..., 0:h:2, 1:w:2] + a[..., 1:h:2, 0:w:2] + a[..., 1:h:2, 1:w:2]
    return (s >> 2).astype(a.dtype)


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
def test_ranks_write_what_one_process_writes(tmp_path, kind, world):
    import torch.multiprocessing as mp
    spec, extra = _spec(kind)
    extra = [*extra, '--pyramid-method', 'mean', '--z-projection', 'max']
    roots = {k: str(tmp_path / k / 'acq') for k in ('one', 'ranks')}
    for r in roots.values():
        synth.write_acquisition(spec, r)
    _single(roots['one'], extra)
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(world, port, roots['ranks'], extra), nprocs=world, join=True)
    one, ranks = _out(roots['one']), _out(roots['ranks'])
    for name in ('R0_stitched.ome.zarr', 'R0_stitched_mip.ome.zarr'):
        want = _store(os.path.join(one, name))
        got = _store(os.path.join(ranks, name))
        assert len(want) == len(got) == (2 if kind == 'planes' else 3), name
        assert want[0].any()
        for lv, (a, b) in enumerate(zip(want, got)):
            np.testing.assert_array_equal(a, b, err_msg=f'{name} level {lv}')
            if lv:
                np.testing.assert_array_equal(b, mean_level(got[lv - 1]), err_msg=f'{name} level {lv} is not the mean of {lv - 1}')
        with open(os.path.join(one, name, '.zattrs'), 'rb') as fa, open(os.path.join(ranks, name, '.zattrs'), 'rb') as fb:
            assert fa.read() == fb.read()
    stack = omezarr.read_array(os.path.join(ranks, 'R0_stitched.ome.zarr', '0'))
    planes = stack.shape[1] * stack.shape[2]
    assert (planes >= world) == (kind == 'planes')      # bands: fewer planes than ranks
