"""Time sq_dpc_tiles on the staged tiles of one config-3 plane (256 tiles of 2048 x 2048 uint16 from the device generator, once
as the left and once, with other noise, as the right halves; HIP events after warm-up, one process, a time limit of its own)
against

    (a) sq_dpc_tiles, in place over left          one launch for the batch: 2 + 2 bytes read and 2 written per pixel
    (b) torch.add(left, right, out=left)          an elementwise op that moves the same 6 bytes per pixel: the yardstick
                                                  (on int16 views of the same buffers: the add wraps, the bytes are the same)
    (c) the same formula with torch ops           int64 copies, floor division, clamp and select, back to uint16; on the first
                                                  B_TILES tiles (its time is per tile), equality with (a) checked there

(a) and (b) alternate in one loop, so both see the same neighbours on the box.

    python tools/dpc_probe.py [tiles [reps]]      -> profiles/dpc_probe_kernel.json
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
M = 65535
B_TILES = min(n, 8)
signal.alarm(int(os.environ.get('SQ_PROBE_LIMIT_S', 300)))      # the probe ends itself: nothing here should take minutes
dev = torch.device('cuda:0')


def tiles(scene, noise):      # a 16 x 16 grid of overlapping views of one scene, a noise seed per tile
    desc = np.zeros(n, dtype=native.SYNTH_DTYPE)
    for i in range(n):
        desc[i] = (scene, noise + i, (i // 16) * 1804, (i % 16) * 1804)
    return native.synth_tiles(desc, H, W, 300, np.uint16, dev)


left0, right = tiles(4242, 977), tiles(5151, 40977)
left = left0.clone()
left_i16, right_i16 = left.view(torch.int16), right.view(torch.int16)
nbytes = left.numel() * 2


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(times):
    return {'ms': round(sorted(times)[len(times) // 2], 3), 'ms_min': round(min(times), 3), 'ms_max': round(max(times), 3)}


def torch_dpc(l, r, gain):
    l, r = l.to(torch.int64), r.to(torch.int64)
    s = l + r
    q = torch.div(M * (s + 2 * gain * (l - r)), (2 * s).clamp(min=1), rounding_mode='floor').clamp(0, M)
    return torch.where(s == 0, torch.zeros_like(q), q).to(torch.int32).to(torch.int16).view(torch.uint16)


result = {'tiles': n, 'shape': [H, W], 'dtype': 'uint16', 'reps': reps, 'bytes_per_plane_set': 3 * nbytes, 'torch_tiles': B_TILES}
for gain in (1, 4):
    a_times, b_times = [], []
    for i in range(reps + 3):      # three warm-up rounds; the values of left drift, the bytes moved do not
        a = event_ms(lambda: native.dpc_tiles(left, right, gain))
        b = event_ms(lambda: torch.add(left_i16, right_i16, out=left_i16))
        if i >= 3:
            a_times.append(a)
            b_times.append(b)
    row = {'a_dpc_tiles': stats(a_times), 'b_torch_add': stats(b_times)}
    row['a_gb_per_s'] = round(3 * nbytes / row['a_dpc_tiles']['ms'] / 1e6, 1)
    row['b_gb_per_s'] = round(3 * nbytes / row['b_torch_add']['ms'] / 1e6, 1)
    row['a_over_b'] = round(row['a_dpc_tiles']['ms'] / row['b_torch_add']['ms'], 2)
    left.copy_(left0)
    got = native.dpc_tiles(left[:B_TILES].clone(), right[:B_TILES], gain)
    keep = {}
    c_times = [event_ms(lambda: keep.__setitem__('out', torch_dpc(left0[:B_TILES], right[:B_TILES], gain))) for _ in range(3)][1:]
    row['c_torch_formula'] = stats(c_times)
    row['equal'] = bool(torch.equal(keep['out'].view(torch.int16), got.view(torch.int16)))
    keep.clear()
    a_tile, c_tile = row['a_dpc_tiles']['ms'] / n, row['c_torch_formula']['ms'] / B_TILES
    row['a_ms_per_tile'], row['c_ms_per_tile'], row['c_over_a'] = round(a_tile, 4), round(c_tile, 4), round(c_tile / a_tile, 1)
    g16 = got.view(torch.int16)
    row['clamped_fraction'] = round(float(((g16 == 0) | (g16 == -1)).float().mean()), 4)
    result[f'gain_{gain}'] = row
    print(f"gain {gain}: equal {row['equal']}  (a) {row['a_dpc_tiles']['ms']:.3f} ms = {row['a_gb_per_s']:.0f} GB/s   (b) add "
          f"{row['b_torch_add']['ms']:.3f} ms = {row['b_gb_per_s']:.0f} GB/s   (a) / (b) = {row['a_over_b']:.2f}   (c) "
          f"{c_tile:.4f} ms/tile = {row['c_over_a']:.0f} x (a)", flush=True)
result['all_equal'] = all(result[f'gain_{g}']['equal'] for g in (1, 4))
print(json.dumps(result))
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, 'dpc_probe_kernel.json'), 'w') as fh:
    json.dump(result, fh, indent=1)
