"""Time sq_tophat_tiles on the staged tiles of one config-3 plane (256 tiles of 2048 x 2048 uint16 from the device generator;
HIP events after warm-up, one process) at R = 8, 50 and 127, against

    (a) sq_tophat_tiles                       two launches for the batch, in place
    (b) the same result with torch            float32 copies (uint16 does not fit half precision), -max_pool2d(-x) along the rows
                                              and the columns for the erosion, max_pool2d both ways for the dilation (the pooling's
                                              implicit -inf padding is the clipped window), subtract, back to uint16; on the
                                              first B_TILES tiles (its time is per tile), equality with (a) checked there
    (c) a device-to-device copy of the tensor  one read and one write of every byte: the floor of anything in place

    python tools/tophat_probe.py [tiles [reps]]      -> profiles/tophat_probe_kernel.json
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, '.')
from image_stitcher_amd import native

OUT = os.environ.get('SQ_PROBE_OUT', 'profiles')
n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
H = W = 2048
B_TILES = min(n, 16)
dev = torch.device('cuda:0')

desc = np.zeros(n, dtype=native.SYNTH_DTYPE)      # a 16 x 16 grid of overlapping views of one scene, a noise seed per tile
for i in range(n):
    desc[i] = (4242, 977 + i, (i // 16) * 1804, (i % 16) * 1804)
src = native.synth_tiles(desc, H, W, 300, np.uint16, dev)
work = torch.empty_like(src)
scratch = torch.empty(native.tophat_scratch_bytes(n, H, W, np.uint16), dtype=torch.uint8, device=dev)
nbytes = src.numel() * 2


def timed(prepare, fn, reps):
    times = []
    for i in range(reps + 2):      # two warm-up rounds
        prepare()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= 2:
            times.append(e0.elapsed_time(e1))
    return {'ms': round(sorted(times)[len(times) // 2], 3), 'ms_min': round(min(times), 3), 'ms_max': round(max(times), 3)}


def torch_tophat(x, radius):
    k = 2 * radius + 1
    f = x.to(torch.float32).unsqueeze(1)
    e = -F.max_pool2d(-f, (1, k), 1, (0, radius))
    e = -F.max_pool2d(-e, (k, 1), 1, (radius, 0))
    o = F.max_pool2d(e, (1, k), 1, (0, radius))
    o = F.max_pool2d(o, (k, 1), 1, (radius, 0))
    return (f - o).squeeze(1).to(torch.int32).to(torch.int16).view(torch.uint16)


result = {'tiles': n, 'shape': [H, W], 'dtype': 'uint16', 'reps': reps, 'bytes': nbytes, 'torch_tiles': B_TILES}
result['c_copy'] = timed(lambda: None, lambda: work.copy_(src), reps)
result['c_copy']['gb_per_s'] = round(2 * nbytes / result['c_copy']['ms'] / 1e6, 1)
print(f"copy {result['c_copy']['ms']:.3f} ms = {result['c_copy']['gb_per_s']:.0f} GB/s read + write", flush=True)
for radius in (8, 50, 127):
    row = {}
    row['a_tophat_tiles'] = timed(lambda: work.copy_(src), lambda: native.tophat_tiles(work, radius, scratch), reps)
    got = work[:B_TILES].clone()
    keep = {}
    row['b_torch'] = timed(lambda: None, lambda: keep.__setitem__('out', torch_tophat(src[:B_TILES], radius)), max(2, reps // 3))
    row['equal'] = bool(torch.equal(keep['out'].view(torch.int16), got.view(torch.int16)))
    keep.clear()
    a_tile = row['a_tophat_tiles']['ms'] / n
    b_tile = row['b_torch']['ms'] / B_TILES
    row['a_ms_per_tile'], row['b_ms_per_tile'] = round(a_tile, 4), round(b_tile, 4)
    row['a_over_copy'] = round(row['a_tophat_tiles']['ms'] / result['c_copy']['ms'], 2)
    row['b_over_a'] = round(b_tile / a_tile, 2)
    row['nonzero_fraction'] = round(float((got.view(torch.int16) != 0).float().mean()), 4)
    result[f'R{radius}'] = row
    print(f"R={radius:3d} equal {row['equal']}  (a) {row['a_tophat_tiles']['ms']:9.3f} ms = {a_tile:.4f} ms/tile = "
          f"{row['a_over_copy']:.2f} x copy   (b) {b_tile:.4f} ms/tile = {row['b_over_a']:.1f} x (a)", flush=True)
result['a_faster_than_b_everywhere'] = all(result[f'R{r}']['b_over_a'] > 1 for r in (8, 50, 127))
result['all_equal'] = all(result[f'R{r}']['equal'] for r in (8, 50, 127))
print(json.dumps(result))
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, 'tophat_probe_kernel.json'), 'w') as fh:
    json.dump(result, fh, indent=1)
