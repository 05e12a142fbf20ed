"""--dark-frame when two ranks share one region (gloo ranks on cuda:0), by (channel, z) planes and by row bands: every rank
subtracts from the tiles it stages, and the ranks write together the output tree of a single process -- which is the tree of a run
without the flag on a folder whose every tile file was subtracted beforehand."""
import hashlib
import os
import socket
import sys

import numpy as np
import pytest

import dark_ref
from helpers import load_case, spec_of
from image_stitcher_amd import synth, tiffio

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOTE = 'R0_stitched_dark_frame.json'
PEDESTAL = 40


def _worker(rank, world, port, root, extra):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), SQ_DIST_BACKEND='gloo')
    from image_stitcher_amd import stitcher_cli
    stitcher_cli.main(['-i', root, '--normalization', 'none', *extra])
    import torch.distributed as dist
    dist.destroy_process_group()


def _single(root, extra):
    from image_stitcher_amd import stitcher_cli
    stitcher_cli.main(['-i', root, '--normalization', 'none', *extra])


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


def _spec(kind):
    info, _ = load_case('reg_3x4_small')
    channels = info['spec']['channels']
    if kind == 'planes':
        # 2 channels x 2 z = 4 planes: every rank takes whole planes; the registration channel takes its frame like the other
        reg = info['params']['registration_channel']
        assert len(channels) == 2
        return spec_of(info), ['-r', '--registration-channel', reg, '--registration-z-level', '1', '--tile-qc', '--seam-qc']
    # one plane of 2 x 2 tiles of 600 x 600 placed by their coordinates: a canvas of about 1100 rows with one level, so bands of
    # 512 rows are dealt over the ranks, and both ranks subtract from tiles of the one channel
    spec = spec_of(dict(info, spec=dict(info['spec'], rows=2, cols=2, tile_h=600, tile_w=600, ov_y=100, ov_x=100, nz=1,
                                        channels=channels[:1])))
    return spec, ['--zarr-compression', 'none', '--tile-qc']


@pytest.mark.parametrize('kind', ['planes', 'bands'])
def test_two_ranks_write_the_tree_of_one_process(tmp_path, kind, capfd):
    import torch.multiprocessing as mp
    spec, extra = _spec(kind)
    rng = np.random.default_rng(77)
    frame = rng.integers(8000, 16000, (spec.tile_h, spec.tile_w)).astype(spec.dtype)      # the tiles lie around 21000
    frame_path = str(tmp_path / 'dark.npy')
    np.save(frame_path, frame)
    flag = ['--dark-frame', '*', frame_path, '--dark-pedestal', str(PEDESTAL)]
    roots = {k: str(tmp_path / k / 'acq') for k in ('one', 'ranks', 'premade')}
    for r in roots.values():
        synth.write_acquisition(spec, r)
    n = total = changed = clipped = 0
    for folder, _, names in os.walk(roots['premade']):      # F -> F'
        for name in names:
            if name.lower().endswith(('.tif', '.tiff')):
                path = os.path.join(folder, name)
                img = tiffio.read_image(path)
                new = dark_ref.dark_file_image(img, frame, PEDESTAL)
                total, changed, clipped = total + img.size, changed + int((new != img).sum()), clipped + int(((new == 0) & (img != 0)).sum())
                tiffio.write_tiff(path, new)
                n += 1
    assert n == (12 * 2 * 2 if kind == 'planes' else 4)
    assert changed > total // 2 and 0.001 * total < clipped < 0.5 * total, (changed, clipped, total)
    _single(roots['one'], extra + flag)
    _single(roots['premade'], extra)
    capfd.readouterr()
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(2, port, roots['ranks'], extra + flag), nprocs=2, join=True)
    printed = capfd.readouterr().out
    one, ranks = _tree(_out(roots['one'])), _tree(_out(roots['ranks']))
    assert one and sorted(one) == sorted(ranks)
    assert [k for k in one if one[k] != ranks[k]] == []
    assert os.path.join('0_stitched', NOTE) in one
    assert any('.ome.zarr' in k and not os.path.basename(k).startswith('.') for k in one)
    assert any(k.endswith('_tile_qc.csv') for k in one)
    # the units the ranks were dealt: whole planes (band -1), or row bands of the one plane
    assert '(plane, band) units' in printed and ('(0, -1)' in printed) == (kind == 'planes')
    # ... and both are the tree of the run without the flag on the subtracted files, but for the note
    pre = _tree(_out(roots['premade']))
    without_note = _tree(_out(roots['ranks']), skip=(NOTE,))
    assert sorted(pre) == sorted(without_note) and [k for k in pre if pre[k] != without_note[k]] == []
