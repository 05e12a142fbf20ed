"""--z-projection when several ranks share one region (gloo ranks on cuda:0): the (channel, row band) units of the
projection are dealt over the ranks, and the projection store equals the single-process one."""
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


def _spawn(tmp_path, name, world, extra):
    import torch.multiprocessing as mp
    info, arrays = load_case(name)
    root = str(tmp_path / name / 'acq')
    synth.write_acquisition(spec_of(info), root)
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(world, port, root, extra), nprocs=world, join=True)
    outs = [d for d in os.listdir(os.path.dirname(root)) if d.startswith('acq_stitched_')]
    assert len(outs) == 1
    return info, arrays, os.path.join(os.path.dirname(root), outs[0], '0_stitched')


@pytest.mark.parametrize('world', [2, 3])
def test_ranks_share_one_region_with_its_projection(tmp_path, world):
    """2 channels x 2 z: with two ranks every rank projects one whole channel, with three the channels are fewer than the
    ranks and are dealt by row band (a single band on this canvas: one rank has no unit)."""
    info, arrays, out = _spawn(tmp_path, 'reg_3x4_small', world,
                               ['--registration-channel', info_channel('reg_3x4_small'), '--registration-z-level', '1',
                                '--z-projection', 'max'])
    np.testing.assert_array_equal(omezarr.read_array(os.path.join(out, 'R0_stitched.ome.zarr', '0')), arrays['t0_R0_canvas'])
    np.testing.assert_array_equal(omezarr.read_array(os.path.join(out, 'R0_stitched_mip.ome.zarr', '0')),
                                  arrays['t0_R0_canvas'].max(axis=2, keepdims=True))


def info_channel(name):
    return load_case(name)[0]['params']['registration_channel']


@pytest.mark.parametrize('world', [2, 3])
def test_projection_split_by_row_band(tmp_path, world):
    """One channel, a 4343-row canvas with 3 pyramid levels: the channel is cut into bands of 2048 rows that the ranks
    project and write on their own; every level equals what one process writes (max over z of the stack, its pyramid)."""
    from oracle import stitch_oracle as O
    info, arrays, out = _spawn(tmp_path, 'reg_2x2_2048', world, ['--zarr-compression', 'none', '--z-projection', 'max'])
    stack = omezarr.read_array(os.path.join(out, 'R0_stitched.ome.zarr', '0'))
    store = os.path.join(out, 'R0_stitched_mip.ome.zarr')
    level0 = omezarr.read_array(os.path.join(store, '0'))
    np.testing.assert_array_equal(level0, stack.max(axis=2, keepdims=True))
    levels = O.pyramid_nearest(level0, info['canvases']['t0_R0']['num_pyramid_levels'])
    assert len(levels) == 3
    for lv in range(1, 3):
        np.testing.assert_array_equal(omezarr.read_array(os.path.join(store, str(lv))), levels[lv])
