"""--seam-qc when two ranks share one region by (channel, z) planes (gloo ranks on cuda:0): every rank's words go into the region's
dense table, one element-wise MAX all-reduce combines them, rank 0 writes -- and the CSV and JSON bytes are those of a single
process."""
import os
import socket
import sys

import pytest

from image_stitcher_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC = synth.GridSpec(rows=3, cols=4, tile_h=64, tile_w=96, ov_y=8, ov_x=12, nz=3, channels=tuple(synth.DEFAULT_CHANNELS[:2]),
                      seed=5, blank_fovs=(7,))
EXTRA = ['--seam-qc', '--z-projection', 'max']


def _worker(rank, world, port, root, extra):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), SQ_DIST_BACKEND='gloo')
    from image_stitcher_amd import stitcher_cli
    stitcher_cli.main(['-i', root, '--normalization', 'none', *extra])
    import torch.distributed as dist
    dist.destroy_process_group()


def _out(root):
    outs = [d for d in os.listdir(os.path.dirname(root)) if d.startswith('acq_stitched_')]
    assert len(outs) == 1
    return os.path.join(os.path.dirname(root), outs[0], '0_stitched')


def test_two_ranks_write_the_report_of_one_process(tmp_path):
    import torch.multiprocessing as mp
    from image_stitcher_amd import stitcher_cli
    roots = {k: str(tmp_path / k / 'acq') for k in ('one', 'ranks')}
    for r in roots.values():
        synth.write_acquisition(SPEC, r)
    stitcher_cli.main(['-i', roots['one'], '--normalization', 'none', *EXTRA])
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(2, port, roots['ranks'], EXTRA), nprocs=2, join=True)
    one, ranks = _out(roots['one']), _out(roots['ranks'])
    names = sorted(f for f in os.listdir(ranks) if '_seam_qc.' in f)
    assert names == ['R0_stitched_seam_qc.csv', 'R0_stitched_seam_qc.json'] == sorted(f for f in os.listdir(one) if '_seam_qc.' in f)
    for name in names:
        with open(os.path.join(one, name), 'rb') as fa, open(os.path.join(ranks, name), 'rb') as fb:
            a, b = fa.read(), fb.read()
        assert a == b and len(a) > 500, name
    with open(os.path.join(ranks, names[0])) as fh:
        assert len(fh.read().splitlines()) == 1 + 17 * 6      # every seam of every plane once, whichever rank measured it
