"""Time sq_affine_tiles on the staged tiles of one config-3 plane (256 tiles of 2048 x 2048 uint16 from the device generator; HIP
events after warm-up, one process, a time limit of its own) at four parameter sets -- A = 0, S = 0 (the copy a chunk's unmapped
planes get); a rotation by 0.2 degree; a rotation by 1 degree with +1 %; every coefficient at 50000 (the range's end: the largest
clamped border, three source rows in most vectors) -- against

    (a) sq_affine_tiles                        one launch for the batch, out of place
    (b) a device copy of the same batch        dst.copy_(src): one read and one write of the same bytes, the floor
    (s) sq_shift_tiles at (77, -200)           the streaming kernel of the constant map
    (w) sq_warp_tiles at D = 1500              the general gather with the same blend: the yardstick
    (c) the same definition with torch         index tensors from integer ops, four gathers, the blend in int64, back to uint16; on
                                               the first B_TILES tiles (its time is per tile), equality with (a) checked there

    python tools/affine_probe.py [tiles [reps]]      -> profiles/affine_probe_kernel.json
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


def torch_affine(x, s, a):
    U, V = W - 1, H - 1
    v = (2 * torch.arange(H, dtype=torch.int64, device=dev) - V)[:, None]
    u = (2 * torch.arange(W, dtype=torch.int64, device=dev) - U)[None, :]
    dv = s[0] + torch.div(16 * (a[0] * v + a[1] * u) + 62500, 125000, rounding_mode='floor')
    du = s[1] + torch.div(16 * (a[2] * v + a[3] * u) + 62500, 125000, rounding_mode='floor')
    Y = (256 * torch.arange(H, dtype=torch.int64, device=dev)[:, None] + dv).clamp(0, 256 * V)
    X = (256 * torch.arange(W, dtype=torch.int64, device=dev)[None, :] + du).clamp(0, 256 * U)
    x0, fx, y0, fy = X >> 8, X & 255, Y >> 8, Y & 255
    x1, y1 = (x0 + 1).clamp(max=U), (y0 + 1).clamp(max=V)
    flat = x.to(torch.int32).view(x.shape[0], -1)
    tap = lambda yy, xx: flat[:, (yy * W + xx).view(-1)].view(x.shape).to(torch.int64)
    acc = tap(y0, x0) * ((256 - fx) * (256 - fy)) + tap(y0, x1) * (fx * (256 - fy)) + tap(y1, x0) * ((256 - fx) * fy) + \
        tap(y1, x1) * (fx * fy) + 32768
    return (acc >> 16).to(torch.int16).view(torch.uint16)


CASES = (('zero', (0, 0), (0, 0, 0, 0)),
         ('rot0.2', (0, 0), (-6, 3491, -3491, -6)),                     # (cos 0.2 - 1, sin 0.2) 10^6
         ('rot1_plus1pct', (0, 0), (9846, 17627, -17627, 9846)),        # 1.01 (cos 1, sin 1) - (1, 0), 10^6
         ('all50000', (0, 0), (50000, 50000, 50000, 50000)))
REALISTIC = ('rot0.2', 'rot1_plus1pct')
result = {'tiles': n, 'shape': [H, W], 'dtype': 'uint16', 'reps': reps, 'bytes': nbytes, 'torch_tiles': B_TILES, 'warp_ppm': 1500,
          'shift': [77, -200]}
copies = []
for name, s, a in CASES:      # the copy, the shift and the gather before every case: the four alternate
    six = tuple(s) + tuple(a)
    copy = timed(lambda: dst.copy_(src), reps)
    shift = timed(lambda: native.shift_tiles(src, (77, -200), out=dst), reps)
    warp = timed(lambda: native.warp_tiles(src, 1500, out=dst), reps)
    copies.append(copy['ms'])
    row = {'params': list(six), 'b_device_copy': copy, 's_shift_tiles': shift, 'w_warp_tiles': warp}
    row['a_affine_tiles'] = timed(lambda: native.affine_tiles(src, six, out=dst), reps)
    row['a_gb_per_s_read_and_written'] = round(2 * nbytes / row['a_affine_tiles']['ms'] / 1e6, 1)
    got = dst[:B_TILES].clone()
    keep = {}
    row['c_torch'] = timed(lambda: keep.__setitem__('out', torch_affine(src[:B_TILES], s, a)), 2)
    out = keep['out']
    row['equal'] = bool(torch.equal(out.view(torch.int16), got.view(torch.int16)))
    row['changed_fraction'] = round(float((got.view(torch.int16) != src[:B_TILES].view(torch.int16)).float().mean()), 4)
    keep.clear()
    del out
    a_tile = row['a_affine_tiles']['ms'] / n
    c_tile = row['c_torch']['ms'] / B_TILES
    row['a_ms_per_tile'], row['c_ms_per_tile'] = round(a_tile, 4), round(c_tile, 4)
    row['a_over_copy'] = round(row['a_affine_tiles']['ms'] / copy['ms'], 2)
    row['a_over_shift'] = round(row['a_affine_tiles']['ms'] / shift['ms'], 2)
    row['a_over_warp'] = round(row['a_affine_tiles']['ms'] / warp['ms'], 2)
    row['c_over_a'] = round(c_tile / a_tile, 2)
    result[name] = row
    print(f"{name:14s} equal {row['equal']}  copy {copy['ms']:.3f} ms  shift {shift['ms']:.3f} ms  warp {warp['ms']:.3f} ms  (a) "
          f"{row['a_affine_tiles']['ms']:8.3f} ms = {row['a_over_copy']:.2f} x copy = {row['a_over_shift']:.2f} x shift = "
          f"{row['a_over_warp']:.2f} x warp   (c) {c_tile:.4f} ms/tile = {row['c_over_a']:.1f} x (a)", flush=True)
result['copy_gb_per_s'] = round(2 * nbytes / min(copies) / 1e6, 1)
result['all_equal'] = all(result[name]['equal'] for name, _, _ in CASES)
result['no_slower_than_warp_at_realistic_parameters'] = all(
    result[name]['a_affine_tiles']['ms'] <= result[name]['w_warp_tiles']['ms'] for name in REALISTIC)
print(json.dumps(result))
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, 'affine_probe_kernel.json'), 'w') as fh:
    json.dump(result, fh, indent=1)
