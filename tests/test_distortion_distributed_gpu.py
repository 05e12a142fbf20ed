"""--distortion-correction when two ranks share one region (gloo ranks on cuda:0), by (channel, z) planes: every rank corrects the
tiles it stages, and the ranks write together the output tree of a single process -- which is the tree of a run without the flag
on a folder of files corrected beforehand."""
import hashlib
import os
import socket
import sys

import pytest

import warp_ref
from helpers import load_case, spec_of
from image_stitcher_amd import synth, tiffio

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOTE = 'R0_stitched_distortion.json'
D = 20000


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


def _tree(out, skip=()):
    found = {}
    for folder, _, names in os.walk(out):
        for name in names:
            if name not in skip:
                with open(os.path.join(folder, name), 'rb') as fh:
                    found[os.path.relpath(os.path.join(folder, name), out)] = hashlib.sha256(fh.read()).hexdigest()
    return found


def test_two_ranks_write_the_tree_of_one_process(tmp_path, capfd):
    import torch.multiprocessing as mp
    info, _ = load_case('reg_3x4_small')
    spec = spec_of(info)      # 2 channels x 2 z = 4 planes: every rank takes whole planes
    extra = ['--registration-channel', info['params']['registration_channel'], '--registration-z-level', '1', '--tile-qc',
             '--seam-qc']
    flag = ['--distortion-correction', str(D)]
    roots = {k: str(tmp_path / k / 'acq') for k in ('one', 'ranks', 'prewarped')}
    for r in roots.values():
        synth.write_acquisition(spec, r)
    n = 0
    for folder, _, names in os.walk(roots['prewarped']):      # F -> F'
        for name in names:
            if name.lower().endswith(('.tif', '.tiff')):
                path = os.path.join(folder, name)
                tiffio.write_tiff(path, warp_ref.warp_file_image(tiffio.read_image(path), D))
                n += 1
    assert n == 12 * 4
    _single(roots['one'], extra + flag)
    _single(roots['prewarped'], extra)
    capfd.readouterr()
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(2, port, roots['ranks'], extra + flag), nprocs=2, join=True)
    printed = capfd.readouterr().out
    one, ranks = _tree(_out(roots['one'])), _tree(_out(roots['ranks']))
    assert one and sorted(one) == sorted(ranks)
    assert [k for k in one if one[k] != ranks[k]] == []
    assert os.path.join('0_stitched', NOTE) in one
    assert any('.ome.zarr' in k and not os.path.basename(k).startswith('.') for k in one)
    assert any(k.endswith('_tile_qc.csv') for k in one) and any(k.endswith('_seam_qc.csv') for k in one)
    # the units the ranks were dealt: whole planes (band -1)
    assert '(plane, band) units' in printed and '(0, -1)' in printed
    # ... and both are the tree of the run without the flag on the corrected files, but for the note
    pre = _tree(_out(roots['prewarped']))
    without_note = _tree(_out(roots['ranks']), skip=(NOTE,))
    assert sorted(pre) == sorted(without_note) and [k for k in pre if pre[k] != without_note[k]] == []
