"""--tile-binning when two ranks share one region (gloo ranks on cuda:0), by (channel, z) planes and by row bands: every rank
bins the tiles it stages, and the ranks write together the output tree of a single process."""
import hashlib
import os
import socket
import sys

import pytest

from helpers import load_case, spec_of
from image_stitcher_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOTE = 'R0_stitched_binning.json'


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
    return os.path.join(os.path.dirname(root), outs[0])


def _tree(out):
    found = {}
    for folder, _, names in os.walk(out):
        for name in names:
            with open(os.path.join(folder, name), 'rb') as fh:
                found[os.path.relpath(os.path.join(folder, name), out)] = hashlib.sha256(fh.read()).hexdigest()
    return found


def _spec(kind):
    info, _ = load_case('reg_3x4_small')
    if kind == 'planes':
        # 2 channels x 2 z = 4 planes: every rank takes whole planes
        return spec_of(info), ['--registration-channel', info['params']['registration_channel'], '--registration-z-level', '1']
    # one plane of 2 x 2 tiles of 1100 x 1100, binned to 550 x 550: a canvas of about 1000 rows with one level, so bands of 512
    # rows are dealt over the ranks
    spec = spec_of(dict(info, spec=dict(info['spec'], rows=2, cols=2, tile_h=1100, tile_w=1100, ov_y=100, ov_x=100, nz=1,
                                        channels=info['spec']['channels'][:1])))
    return spec, ['--zarr-compression', 'none']


@pytest.mark.parametrize('kind', ['planes', 'bands'])
def test_two_ranks_write_the_tree_of_one_process(tmp_path, kind, capfd):
    import torch.multiprocessing as mp
    spec, extra = _spec(kind)
    extra = [*extra, '--tile-binning', '2', '--tile-qc']
    roots = {k: str(tmp_path / k / 'acq') for k in ('one', 'ranks')}
    for r in roots.values():
        synth.write_acquisition(spec, r)
    _single(roots['one'], extra)
    capfd.readouterr()
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(2, port, roots['ranks'], extra), nprocs=2, join=True)
    printed = capfd.readouterr().out
    one, ranks = _tree(_out(roots['one'])), _tree(_out(roots['ranks']))
    assert one and sorted(one) == sorted(ranks)
    assert [k for k in one if one[k] != ranks[k]] == []
    assert os.path.join('0_stitched', NOTE) in one
    assert any('.ome.zarr' in k and not os.path.basename(k).startswith('.') for k in one)
    # the units the ranks were dealt: whole planes (band -1), or row bands of the one plane
    assert '(plane, band) units' in printed and ('(0, -1)' in printed) == (kind == 'planes')
