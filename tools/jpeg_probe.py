"""What the device JPEG tile encoder (csrc/jpeg.hip) costs and what it saves, on an MI355X.

    python tools/jpeg_probe.py               the step below as a child process under a time limit of its own; at most 16 CPU threads
    python tools/jpeg_probe.py kernel [planes [reps]]
        4 config-3 planes (36 428 x 29 108 uint8, smooth + 2 counts of noise, a quarter of every plane uncovered = zero), tiles of
        512 x 512, HIP events, best of `reps`, all in one run on the same planes:
          sq_jpeg_encode_planes at quality 75 and 90  against  sq_deflate_encode_planes (predictor 2; the yardstick)  and  torch.amax
          over the same bytes (the plain read the other probes use);
        sizes of both; 16 sampled tile streams compared with jpegtile.encode_tile byte for byte
        -> profiles/jpeg_probe_kernel.json
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get('SQ_PROBE_OUT', os.path.join(ROOT, 'profiles'))
LIMITS = {'kernel': 420}      # seconds

if len(sys.argv) < 2:
    for step in ('kernel',):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), step], timeout=LIMITS[step]).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f'step {step} ended with {rc}: nothing more is started')
            sys.exit(rc)
    sys.exit(0)

import numpy as np
import torch

sys.path.insert(0, ROOT)
from image_stitcher_amd import jpegtile, native

torch.set_num_threads(min(16, torch.get_num_threads()))


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return best


def kernel_probe(n=4, reps=3):
    dev = torch.device('cuda:0')
    h, w, t = 36428, 29108, 512
    yy = torch.linspace(-1, 1, h, device=dev)[:, None]
    xx = torch.linspace(-1, 1, w, device=dev)[None, :]
    planes = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    for p in range(n):
        img = 40 + 150 * (1 - 0.3 * (yy * yy + xx * xx)) + 2 * torch.randn((h, w), device=dev)
        img[: h // 2, : w // 2] = 0      # no tile reaches here
        planes[p].copy_(img.clamp_(0, 255).to(torch.uint8))
        del img
    raw = planes.numel()
    result = {'planes': n, 'shape': [h, w], 'dtype': 'uint8', 'tile': t, 'raw_bytes': raw, 'reps': reps}
    ms = timed(lambda: planes.amax(), reps)
    result['plain_read_ms'] = round(ms, 3)
    print(f'torch.amax: {ms:.2f} ms = {raw / ms / 1e6:.0f} GB/s', flush=True)
    dbuf = native.DeflateBuffers(n, h, w, np.uint8, t, t, dev)
    ms = timed(lambda: native.deflate_encode_planes(planes, t, t, 2, dbuf), reps)
    assert int(dbuf.status.item()) == 0
    result['deflate_ms'], result['deflate_bytes'] = round(ms, 3), int(dbuf.offsets[-1].item())
    print(f'deflate encode: {ms:.2f} ms = {raw / ms / 1e6:.0f} GB/s in, {result["deflate_bytes"]} bytes = '
          f'{result["deflate_bytes"] / raw:.4f} of raw', flush=True)
    del dbuf
    gy, gx = -(-h // t), -(-w // t)
    sample = [int(i) for i in np.linspace(0, gy * gx - 1, 16).astype(int)]
    host = planes[0].cpu().numpy()
    jbuf = native.JpegBuffers(n, h, w, t, t, dev)
    for q in (75, 90):
        ms = timed(lambda: native.jpeg_encode_planes(planes, t, t, q, jbuf), reps)
        assert int(jbuf.status.item()) == 0
        off = jbuf.offsets.cpu().numpy()
        checked = 0
        for i in sample:      # the sampled streams are the host definition's
            iy, ix = divmod(i, gx)
            tile = np.zeros((t, t), np.uint8)
            part = host[iy * t:(iy + 1) * t, ix * t:(ix + 1) * t]
            tile[:part.shape[0], :part.shape[1]] = part
            got = jbuf.out[int(off[i]):int(off[i + 1])].cpu().numpy().tobytes()
            assert got == (jpegtile.encode_tile(tile, q) if tile.any() else b''), f'tile {i} at quality {q} differs from the host'
            checked += 1
        result[f'jpeg_q{q}_ms'], result[f'jpeg_q{q}_bytes'] = round(ms, 3), int(off[-1])
        result[f'jpeg_q{q}_over_deflate_time'] = round(ms / result['deflate_ms'], 3)
        result[f'jpeg_q{q}_over_plain_read'] = round(ms / result['plain_read_ms'], 3)
        result[f'jpeg_q{q}_over_deflate_bytes'] = round(int(off[-1]) / result['deflate_bytes'], 4)
        result[f'jpeg_q{q}_tiles_compared'] = checked
        print(f'jpeg q{q} encode: {ms:.2f} ms = {raw / ms / 1e6:.0f} GB/s in, {int(off[-1])} bytes = {off[-1] / raw:.4f} of raw, '
              f'{ms / result["deflate_ms"]:.3f} of the deflate encoder\'s time', flush=True)
    print(json.dumps(result), flush=True)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, 'jpeg_probe_kernel.json'), 'w') as fh:
        json.dump(result, fh, indent=1)


if sys.argv[1] == 'kernel':
    kernel_probe(*(int(v) for v in sys.argv[2:4]))
else:
    sys.exit(__doc__)
