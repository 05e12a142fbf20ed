"""Time sq_tile_stats on the staged tiles of one config-3 plane (256 tiles of 2048 x 2048 uint16 from the device generator; HIP
events after warm-up, one process, a time limit of its own) against

    (a) sq_tile_stats                          one launch for the batch (plus the 16 KiB identity fill), eight words per tile
    (b) torch.amax over the same bytes         a plain reduction read: the roof of anything that reads the batch once
    (c) sq_despeckle_tiles on the same batch   the launch the report sits in front of (one read and one write of every byte)
    (d) the same words with torch              on the first B_TILES tiles (its time is per tile), equality with (a) checked there

The launches alternate (a, b, c, a, b, c, ...) so that whatever else the box does lands on all of them; the medians are quoted.

    python tools/tile_stats_probe.py [tiles [reps]]      -> profiles/tile_stats_probe_kernel.json
"""
import json
import os
import signal
import sys

import numpy as np
import torch

sys.path.insert(0, '.')
from image_stitcher_amd import native

OUT = os.environ.get('SQ_PROBE_OUT', 'profiles')
n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 15
H = W = 2048
B_TILES = min(n, 8)
signal.alarm(int(os.environ.get('SQ_PROBE_LIMIT_S', 300)))      # the probe ends itself: nothing here should take minutes
dev = torch.device('cuda:0')

desc = np.zeros(n, dtype=native.SYNTH_DTYPE)      # a 16 x 16 grid of overlapping views of one scene, a noise seed per tile
for i in range(n):
    desc[i] = (4242, 977 + i, (i // 16) * 1804, (i % 16) * 1804)
src = native.synth_tiles(desc, H, W, 300, np.uint16, dev)
dst = torch.empty_like(src)
words = torch.empty((n, native.SQ_TILE_STATS_WORDS), dtype=torch.int64, device=dev)
nbytes = src.numel() * 2


def torch_words(x):
    f = x.to(torch.int64)
    dx = f[:, :, 2:] - f[:, :, :-2]
    dy = f[:, 2:, :] - f[:, :-2, :]
    return torch.stack([f.amin(dim=(1, 2)), f.amax(dim=(1, 2)), f.sum(dim=(1, 2)), (f * f).sum(dim=(1, 2)),
                        (f == 65535).sum(dim=(1, 2)), (f == 0).sum(dim=(1, 2)), (dx * dx).sum(dim=(1, 2)),
                        (dy * dy).sum(dim=(1, 2))], dim=1)


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(times):
    return {'ms': round(sorted(times)[len(times) // 2], 4), 'ms_min': round(min(times), 4), 'ms_max': round(max(times), 4)}


launches = {'a_tile_stats': lambda: native.tile_stats(src, out=words),
            'b_amax_read': lambda: src.view(torch.int16).amax(),
            'c_despeckle_hot': lambda: native.despeckle_tiles(src, 1000, 'hot', out=dst)}
times = {k: [] for k in launches}
for i in range(reps + 3):      # three warm-up rounds
    for k, fn in launches.items():
        t = once(fn)
        if i >= 3:
            times[k].append(t)
result = {'tiles': n, 'shape': [H, W], 'dtype': 'uint16', 'reps': reps, 'bytes': nbytes, 'torch_tiles': B_TILES,
          'rows_per_thread': native.SQ_TILE_STATS_ROWS_PER_THREAD}
for k in launches:
    result[k] = stats(times[k])
    result[k]['gb_per_s_read'] = round(nbytes / result[k]['ms'] / 1e6, 1)
keep = {}
result['d_torch'] = stats([once(lambda: keep.__setitem__('w', torch_words(src[:B_TILES]))) for _ in range(3)])
result['equal'] = bool(torch.equal(keep['w'], words[:B_TILES]))
a, b, c = (result[k]['ms'] for k in launches)
result['a_over_read'] = round(a / b, 3)
result['a_over_despeckle'] = round(a / c, 3)
result['a_ms_per_tile'] = round(a / n, 5)
result['d_ms_per_tile'] = round(result['d_torch']['ms'] / B_TILES, 4)
result['d_over_a'] = round(result['d_ms_per_tile'] / (a / n), 1)
print(f"tile_stats {a:.3f} ms = {result['a_tile_stats']['gb_per_s_read']:.0f} GB/s read; amax {b:.3f} ms; despeckle {c:.3f} ms; "
      f"a / read = {result['a_over_read']:.2f}, a / despeckle = {result['a_over_despeckle']:.2f}; torch {result['d_ms_per_tile']:.3f} "
      f"ms/tile = {result['d_over_a']:.0f} x; equal {result['equal']}", flush=True)
print(json.dumps(result))
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, 'tile_stats_probe_kernel.json'), 'w') as fh:
    json.dump(result, fh, indent=1)
