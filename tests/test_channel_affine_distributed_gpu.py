"""--channel-affine when two ranks share one region (gloo ranks on cuda:0), by (channel, z) planes and by row bands: every rank
maps the tiles it stages, and the ranks write together the output tree of a single process -- which is the tree of a run without
the flags on a folder whose files of the mapped channel were transformed beforehand (tests/affine_ref.py)."""
import hashlib
import os
import socket
import sys

import pytest

import affine_ref
from helpers import load_case, spec_of
from image_stitcher_amd import synth, tiffio

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOTES = ('R0_stitched_channel_affine.json', 'R0_stitched_channel_shift.json')
SHIFT, AFFINE = (77, -200), (2994, -3501, 3501, 2994)      # rotation by -0.2 degree with +0.3 %, and a shift
PIXELS = ['0.30078125', '-0.78125']      # the same pair as the command line gives it


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
        # 2 channels x 2 z = 4 planes: every rank takes whole planes; one channel is registered on, the other mapped
        reg = info['params']['registration_channel']
        other = [c for c in channels if c != reg]
        assert len(channels) == 2 and len(other) == 1
        return spec_of(info), other[0], ['-r', '--registration-channel', reg, '--registration-z-level', '1', '--tile-qc',
                                         '--seam-qc']
    # one plane of 2 x 2 tiles of 600 x 600 placed by their coordinates: a canvas of about 1100 rows with one level, so bands of
    # 512 rows are dealt over the ranks, and both ranks map tiles of the one channel
    spec = spec_of(dict(info, spec=dict(info['spec'], rows=2, cols=2, tile_h=600, tile_w=600, ov_y=100, ov_x=100, nz=1,
                                        channels=channels[:1])))
    return spec, channels[0], ['--zarr-compression', 'none', '--tile-qc']


@pytest.mark.parametrize('kind', ['planes', 'bands'])
def test_two_ranks_write_the_tree_of_one_process(tmp_path, kind, capfd):
    import torch.multiprocessing as mp
    spec, shifted, extra = _spec(kind)
    flag = ['--channel-shift', shifted, *PIXELS, '--channel-affine', shifted, *(str(c) for c in AFFINE)]
    roots = {k: str(tmp_path / k / 'acq') for k in ('one', 'ranks', 'premade')}
    for r in roots.values():
        synth.write_acquisition(spec, r)
    n = 0
    token = shifted.replace(' ', '_')
    for folder, _, names in os.walk(roots['premade']):      # F -> F'
        for name in names:
            if name.lower().endswith(('.tif', '.tiff')) and token in name:
                path = os.path.join(folder, name)
                tiffio.write_tiff(path, affine_ref.affine_file_image(tiffio.read_image(path), SHIFT, AFFINE))
                n += 1
    assert n == (12 * 2 if kind == 'planes' else 4)
    _single(roots['one'], extra + flag)
    _single(roots['premade'], extra)
    capfd.readouterr()
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(2, port, roots['ranks'], extra + flag), nprocs=2, join=True)
    printed = capfd.readouterr().out
    one, ranks = _tree(_out(roots['one'])), _tree(_out(roots['ranks']))
    assert one and sorted(one) == sorted(ranks)
    assert [k for k in one if one[k] != ranks[k]] == []
    assert all(os.path.join('0_stitched', note) in one for note in NOTES)
    assert any('.ome.zarr' in k and not os.path.basename(k).startswith('.') for k in one)
    assert any(k.endswith('_tile_qc.csv') for k in one)
    # the units the ranks were dealt: whole planes (band -1), or row bands of the one plane
    assert '(plane, band) units' in printed and ('(0, -1)' in printed) == (kind == 'planes')
    # ... and both are the tree of the run without the flag on the transformed files, but for the notes
    pre = _tree(_out(roots['premade']))
    without_note = _tree(_out(roots['ranks']), skip=NOTES)
    assert sorted(pre) == sorted(without_note) and [k for k in pre if pre[k] != without_note[k]] == []
