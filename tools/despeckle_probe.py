"""Time sq_despeckle_tiles on the staged tiles of one config-3 plane (256 tiles of 2048 x 2048 uint16 from the device generator;
HIP events after warm-up, one process, a time limit of its own) in both modes at T = 1000 and at T = 0, against

    (a) sq_despeckle_tiles                     one launch for the batch, out of place, counts included
    (b) the same result with torch             float32 copies (they hold uint16 exactly), replicate padding, the nine shifted
                                               views stacked, torch.median over them, compare and select, back to uint16; on the
                                               first B_TILES tiles (its time is per tile), equality with (a) checked there
    (c) dst.copy_(src) of the same batch       one read and one write of every byte: the floor of anything out of place

    python tools/despeckle_probe.py [tiles [reps]]      -> profiles/despeckle_probe_kernel.json
"""
import json
import os
import signal
import sys

import numpy as np
import torch
import torch.nn.functional as F

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
dst = torch.empty_like(src)
counts = torch.zeros(n, dtype=torch.int64, device=dev)
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


def torch_despeckle(x, threshold, mode):
    f = x.to(torch.float32)
    p = F.pad(f.unsqueeze(1), (1, 1, 1, 1), mode='replicate').squeeze(1)
    m = torch.stack([p[:, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)]).median(dim=0).values
    d = f - m
    fire = (d if mode == 'hot' else d.abs()) > threshold
    return torch.where(fire, m, f).to(torch.int32).to(torch.int16).view(torch.uint16)


result = {'tiles': n, 'shape': [H, W], 'dtype': 'uint16', 'reps': reps, 'bytes': nbytes, 'torch_tiles': B_TILES}
result['c_copy'] = timed(lambda: dst.copy_(src), reps)
result['c_copy']['gb_per_s'] = round(2 * nbytes / result['c_copy']['ms'] / 1e6, 1)
print(f"copy {result['c_copy']['ms']:.3f} ms = {result['c_copy']['gb_per_s']:.0f} GB/s read + write", flush=True)
cases = [('hot', 1000), ('both', 1000), ('both', 0)]
for mode, threshold in cases:
    row = {}
    row['a_despeckle_tiles'] = timed(lambda: native.despeckle_tiles(src, threshold, mode, out=dst, counts=counts), reps)
    row['a_gb_per_s'] = round(2 * nbytes / row['a_despeckle_tiles']['ms'] / 1e6, 1)
    got = dst[:B_TILES].clone()
    keep = {}
    row['b_torch'] = timed(lambda: keep.__setitem__('out', torch_despeckle(src[:B_TILES], threshold, mode)), 2)
    row['equal'] = bool(torch.equal(keep['out'].view(torch.int16), got.view(torch.int16)))
    keep.clear()
    a_tile = row['a_despeckle_tiles']['ms'] / n
    b_tile = row['b_torch']['ms'] / B_TILES
    row['a_ms_per_tile'], row['b_ms_per_tile'] = round(a_tile, 4), round(b_tile, 4)
    row['a_over_copy'] = round(row['a_despeckle_tiles']['ms'] / result['c_copy']['ms'], 2)
    row['b_over_a'] = round(b_tile / a_tile, 2)
    row['replaced_fraction'] = round(float((got.view(torch.int16) != src[:B_TILES].view(torch.int16)).float().mean()), 4)
    result[f'{mode}_T{threshold}'] = row
    print(f"{mode:4s} T={threshold:4d} equal {row['equal']}  (a) {row['a_despeckle_tiles']['ms']:8.3f} ms = {a_tile:.4f} ms/tile = "
          f"{row['a_over_copy']:.2f} x copy   (b) {b_tile:.4f} ms/tile = {row['b_over_a']:.1f} x (a)", flush=True)
result['all_equal'] = all(result[f'{m}_T{t}']['equal'] for m, t in cases)
print(json.dumps(result))
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, 'despeckle_probe_kernel.json'), 'w') as fh:
    json.dump(result, fh, indent=1)
