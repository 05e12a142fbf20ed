"""Time sq_bin_tiles on the staged tiles of one config-3 plane (256 tiles of 2048 x 2048 uint16 from the device generator; HIP
events after warm-up, one process, a time limit of its own) with K = 2 and 4 in both methods, against

    (a) sq_bin_tiles                           one launch for the batch, out of place: it writes 1 / K^2 of what it reads
    (b) torch.amax over the same bytes         a plain reduction read: the roof of anything that reads the batch once (the
                                               yardstick of tools/tile_stats_probe.py)
    (c) the same binning with torch            reshape to [n, hb, K, wb, K], integer sum over the two K axes, divide or clamp,
                                               back to uint16; on the first B_TILES tiles (its time is per tile), equality with
                                               (a) checked there

    python tools/bin_probe.py [tiles [reps]]      -> profiles/bin_probe_kernel.json
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
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
H = W = 2048
B_TILES = min(n, 8)
signal.alarm(int(os.environ.get('SQ_PROBE_LIMIT_S', 300)))      # the probe ends itself: nothing here should take minutes
dev = torch.device('cuda:0')

desc = np.zeros(n, dtype=native.SYNTH_DTYPE)      # a 16 x 16 grid of overlapping views of one scene, a noise seed per tile
for i in range(n):
    desc[i] = (4242, 977 + i, (i // 16) * 1804, (i % 16) * 1804)
src = native.synth_tiles(desc, H, W, 300, np.uint16, dev)
nbytes = src.numel() * 2


def timed(fn, reps):
    times = []
    for i in range(reps + 3):      # three warm-up rounds
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= 3:
            times.append(e0.elapsed_time(e1))
    return {'ms': round(sorted(times)[len(times) // 2], 3), 'ms_min': round(min(times), 3), 'ms_max': round(max(times), 3)}


def torch_bin(x, k, method):
    hb, wb = H // k, W // k
    s = x[:, :hb * k, :wb * k].to(torch.int32).view(-1, hb, k, wb, k).sum(dim=(2, 4))
    s = s // (k * k) if method == 'mean' else s.clamp(max=65535)
    return s.to(torch.int16).view(torch.uint16)


result = {'tiles': n, 'shape': [H, W], 'dtype': 'uint16', 'reps': reps, 'bytes': nbytes, 'torch_tiles': B_TILES}
result['b_amax_read'] = timed(lambda: src.view(torch.int16).amax(), reps)
result['b_amax_read']['gb_per_s'] = round(nbytes / result['b_amax_read']['ms'] / 1e6, 1)
print(f"amax {result['b_amax_read']['ms']:.3f} ms = {result['b_amax_read']['gb_per_s']:.0f} GB/s read", flush=True)
cases = [(2, 'mean'), (2, 'sum'), (4, 'mean'), (4, 'sum')]
for k, method in cases:
    dst = torch.empty((n, H // k, W // k), dtype=torch.uint16, device=dev)
    row = {}
    row['a_bin_tiles'] = timed(lambda: native.bin_tiles(src, k, method, out=dst), reps)
    row['a_gb_per_s_read'] = round(nbytes / row['a_bin_tiles']['ms'] / 1e6, 1)
    got = dst[:B_TILES].clone()
    keep = {}
    row['c_torch'] = timed(lambda: keep.__setitem__('out', torch_bin(src[:B_TILES], k, method)), 2)
    row['equal'] = bool(torch.equal(keep['out'].view(torch.int16), got.view(torch.int16)))
    keep.clear()
    a_tile = row['a_bin_tiles']['ms'] / n
    c_tile = row['c_torch']['ms'] / B_TILES
    row['a_ms_per_tile'], row['c_ms_per_tile'] = round(a_tile, 4), round(c_tile, 4)
    row['a_over_read'] = round(row['a_bin_tiles']['ms'] / result['b_amax_read']['ms'], 2)
    row['c_over_a'] = round(c_tile / a_tile, 2)
    if method == 'sum':
        row['saturated_fraction'] = round(float((got.view(torch.int16) == -1).float().mean()), 4)
    result[f'K{k}_{method}'] = row
    print(f"K={k} {method:4s} equal {row['equal']}  (a) {row['a_bin_tiles']['ms']:8.3f} ms = {a_tile:.4f} ms/tile = "
          f"{row['a_over_read']:.2f} x read   (c) {c_tile:.4f} ms/tile = {row['c_over_a']:.1f} x (a)", flush=True)
    del dst
result['all_equal'] = all(result[f'K{k}_{m}']['equal'] for k, m in cases)
print(json.dumps(result))
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, 'bin_probe_kernel.json'), 'w') as fh:
    json.dump(result, fh, indent=1)
