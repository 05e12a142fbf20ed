"""Time sq_shift_tiles on the staged tiles of one config-3 plane (256 tiles of 2048 x 2048 uint16 from the device generator; HIP
events after warm-up, one process, a time limit of its own) at S = (0, 0) (the copy a chunk's unshifted planes get), (256, -512)
(whole pixels: the source span at dst's phase) and (77, -200) (a fraction on both axes: the span one element off dst's phase),
against

    (a) sq_shift_tiles                         one launch for the batch, out of place: every source row read once per run of 32
                                               rows plus one halo row, dst written once
    (b) a device copy of the same batch        dst.copy_(src): one read and one write of the same bytes, the floor
    (w) sq_warp_tiles at D = 1500              the gather a constant shift does not fit: the kernel (a) has to beat
    (c) the same definition with torch         clamped index tensors, four gathers, the blend in int64, back to uint16; on the
                                               first B_TILES tiles (its time is per tile), equality with (a) checked there

    python tools/shift_probe.py [tiles [reps]]      -> profiles/shift_probe_kernel.json
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
dst = torch.empty_like(src)
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


def torch_shift(x, sy, sx):
    U, V = W - 1, H - 1
    X = (256 * torch.arange(W, dtype=torch.int64, device=dev)[None, :] + sx).clamp(0, 256 * U)
    Y = (256 * torch.arange(H, dtype=torch.int64, device=dev)[:, None] + sy).clamp(0, 256 * V)
    x0, fx, y0, fy = X >> 8, X & 255, Y >> 8, Y & 255
    x1, y1 = (x0 + 1).clamp(max=U), (y0 + 1).clamp(max=V)
    flat = x.to(torch.int32).view(x.shape[0], -1)
    tap = lambda yy, xx: flat[:, (yy * W + xx).view(-1)].view(x.shape).to(torch.int64)
    acc = tap(y0, x0) * ((256 - fx) * (256 - fy)) + tap(y0, x1) * (fx * (256 - fy)) + tap(y1, x0) * ((256 - fx) * fy) + \
        tap(y1, x1) * (fx * fy) + 32768
    return (acc >> 16).to(torch.int16).view(torch.uint16)


result = {'tiles': n, 'shape': [H, W], 'dtype': 'uint16', 'reps': reps, 'bytes': nbytes, 'torch_tiles': B_TILES, 'warp_ppm': 1500}
cases = ((0, 0), (256, -512), (77, -200))
copies, warps = [], []
for sy, sx in cases:      # the copy and the gather before every case: the three alternate
    copy = timed(lambda: dst.copy_(src), reps)
    warp = timed(lambda: native.warp_tiles(src, 1500, out=dst), reps)
    copies.append(copy['ms'])
    warps.append(warp['ms'])
    row = {'b_device_copy': copy, 'w_warp_tiles': warp}
    row['a_shift_tiles'] = timed(lambda: native.shift_tiles(src, (sy, sx), out=dst), reps)
    row['a_gb_per_s_read_and_written'] = round(2 * nbytes / row['a_shift_tiles']['ms'] / 1e6, 1)
    got = dst[:B_TILES].clone()
    keep = {}
    row['c_torch'] = timed(lambda: keep.__setitem__('out', torch_shift(src[:B_TILES], sy, sx)), 2)
    out = keep['out']
    row['equal'] = bool(torch.equal(out.view(torch.int16), got.view(torch.int16)))
    row['changed_fraction'] = round(float((got.view(torch.int16) != src[:B_TILES].view(torch.int16)).float().mean()), 4)
    keep.clear()
    del out
    a_tile = row['a_shift_tiles']['ms'] / n
    c_tile = row['c_torch']['ms'] / B_TILES
    row['a_ms_per_tile'], row['c_ms_per_tile'] = round(a_tile, 4), round(c_tile, 4)
    row['a_over_copy'] = round(row['a_shift_tiles']['ms'] / copy['ms'], 2)
    row['a_over_warp'] = round(row['a_shift_tiles']['ms'] / warp['ms'], 2)
    row['c_over_a'] = round(c_tile / a_tile, 2)
    result[f'S{sy}_{sx}'] = row
    print(f"S=({sy:4d},{sx:5d}) equal {row['equal']}  copy {copy['ms']:.3f} ms  warp {warp['ms']:.3f} ms  (a) "
          f"{row['a_shift_tiles']['ms']:8.3f} ms = {row['a_over_copy']:.2f} x copy = {row['a_over_warp']:.2f} x warp   (c) "
          f"{c_tile:.4f} ms/tile = {row['c_over_a']:.1f} x (a)", flush=True)
result['copy_gb_per_s'] = round(2 * nbytes / min(copies) / 1e6, 1)
result['all_equal'] = all(result[f'S{sy}_{sx}']['equal'] for sy, sx in cases)
result['faster_than_warp'] = all(result[f'S{sy}_{sx}']['a_shift_tiles']['ms'] < result[f'S{sy}_{sx}']['w_warp_tiles']['ms']
                                 for sy, sx in cases)
print(json.dumps(result))
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, 'shift_probe_kernel.json'), 'w') as fh:
    json.dump(result, fh, indent=1)
