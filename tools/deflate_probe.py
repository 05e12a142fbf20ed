"""What the device tile encoder (csrc/deflate.hip) costs and what it saves, on an MI355X.

    python tools/deflate_probe.py            both steps below, each a child process under a time limit of its own; the second
                                             starts only when the first ended well; at most 16 CPU threads
    python tools/deflate_probe.py kernel [planes [reps]]
        4 config-3 planes (36 428 x 29 108 uint16, smooth + 8 counts of noise, a quarter of every plane uncovered = zero), tiles of
        512 x 512, HIP events, best of `reps`:
          sq_deflate_encode_planes (predictor 2)  against  sq_blosc_encode_planes on the same planes and chunk shape  and  torch.amax
          over the same bytes (the plain read the other probes use);
        sizes: deflate against Blosc, and both against host zlib level 1 of the same predicted bytes on a sample of 64 tiles
        -> profiles/deflate_probe_kernel.json
    python tools/deflate_probe.py run
        files -> pyramid OME-TIFF against files -> Blosc OME-Zarr store, both on /dev/shm, Stitcher.run on one region of 16 x 16
        tiles of 2048^2 (a config-3 canvas: six levels), 1 channel x 2 z, three repetitions alternating: wall time per region
        -> profiles/deflate_probe_run.json
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get('SQ_PROBE_OUT', os.path.join(ROOT, 'profiles'))
LIMITS = {'kernel': 420, 'run': 540}      # seconds

if len(sys.argv) < 2:
    for step in ('kernel', 'run'):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), step], timeout=LIMITS[step]).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f'step {step} ended with {rc}: nothing more is started')
            sys.exit(rc)
    sys.exit(0)

import zlib

import numpy as np
import torch

sys.path.insert(0, ROOT)
from image_stitcher_amd import native

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
    planes = torch.empty((n, h, w), dtype=torch.uint16, device=dev)
    for p in range(n):
        img = 2000 + 3000 * (1 - 0.3 * (yy * yy + xx * xx)) + 8 * torch.randn((h, w), device=dev)
        img[: h // 2, : w // 2] = 0      # no tile reaches here
        planes[p].view(torch.int16).copy_(img.clamp_(0, 32767).to(torch.int16))
        del img
    raw = planes.numel() * 2
    result = {'planes': n, 'shape': [h, w], 'dtype': 'uint16', 'tile': t, 'raw_bytes': raw, 'reps': reps}
    ms = timed(lambda: planes.view(torch.int16).amax(), reps)
    result['plain_read_ms'] = round(ms, 3)
    print(f'torch.amax: {ms:.2f} ms = {raw / ms / 1e6:.0f} GB/s', flush=True)
    dbuf = native.DeflateBuffers(n, h, w, np.uint16, t, t, dev)
    ms = timed(lambda: native.deflate_encode_planes(planes, t, t, 2, dbuf), reps)
    doff = dbuf.offsets.cpu().numpy()
    result['deflate_ms'], result['deflate_bytes'] = round(ms, 3), int(doff[-1])
    print(f'deflate encode: {ms:.2f} ms = {raw / ms / 1e6:.0f} GB/s in, {int(doff[-1])} bytes = {doff[-1] / raw:.4f} of raw', flush=True)
    gy, gx = -(-h // t), -(-w // t)
    sample = [int(i) for i in np.linspace(0, gy * gx - 1, 64).astype(int)]
    dsize = {i: int(doff[i + 1] - doff[i]) for i in sample}
    # the sampled streams inflate to the predicted tiles (what the sizes are compared on)
    host = planes[0].cpu().numpy()
    zsize, checked = {}, 0
    for i in sample:
        iy, ix = divmod(i, gx)
        tile = np.zeros((t, t), np.uint16)
        part = host[iy * t:(iy + 1) * t, ix * t:(ix + 1) * t]
        tile[:part.shape[0], :part.shape[1]] = part
        pred = tile.copy()
        pred[:, 1:] = tile[:, 1:] - tile[:, :-1]
        zsize[i] = len(zlib.compress(pred.tobytes(), 1)) if tile.any() else 0
        if dsize[i]:
            got = zlib.decompress(dbuf.out[int(doff[i]):int(doff[i + 1])].cpu().numpy().tobytes())
            assert got == pred.tobytes(), f'tile {i}: the stream does not inflate to the tile'
            checked += 1
    del dbuf
    bbuf = native.BloscBuffers(n, h, w, np.uint16, t, t, dev)
    ms = timed(lambda: native.blosc_encode_planes(planes, t, t, bbuf), reps)
    boff = bbuf.offsets.cpu().numpy()
    result['blosc_ms'], result['blosc_bytes'] = round(ms, 3), int(boff[-1])
    print(f'blosc encode: {ms:.2f} ms = {raw / ms / 1e6:.0f} GB/s in, {int(boff[-1])} bytes = {boff[-1] / raw:.4f} of raw', flush=True)
    bsize = {i: int(boff[i + 1] - boff[i]) for i in sample}
    nz = [i for i in sample if zsize[i]]
    result['sample'] = {'tiles': len(sample), 'non_zero': len(nz), 'inflated_and_compared': checked,
                        'deflate_bytes': sum(dsize[i] for i in nz), 'blosc_bytes': sum(bsize[i] for i in nz),
                        'host_zlib1_bytes': sum(zsize[i] for i in nz), 'raw_bytes': len(nz) * t * t * 2}
    result['deflate_over_blosc_time'] = round(result['deflate_ms'] / result['blosc_ms'], 3)
    result['deflate_over_plain_read'] = round(result['deflate_ms'] / result['plain_read_ms'], 3)
    print(json.dumps(result), flush=True)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, 'deflate_probe_kernel.json'), 'w') as fh:
        json.dump(result, fh, indent=1)


def run_probe():
    import contextlib
    import io
    import shutil
    import tempfile
    from image_stitcher_amd import synth
    from image_stitcher_amd.stitcher import Stitcher
    from image_stitcher_amd.stitcher_parameters import StitchingParameters
    spec = synth.GridSpec(rows=16, cols=16, tile_h=2048, tile_w=2048, ov_y=244, ov_x=244, seed=5300,
                          channels=synth.DEFAULT_CHANNELS[:1], nz=2, nt=1)
    tmp = tempfile.mkdtemp(prefix='deflate_', dir='/dev/shm')
    result = {'grid': '16x16 of 2048^2', 'planes_per_region': 2}
    try:
        root = os.path.join(tmp, 'acq')
        synth.write_acquisition_device(spec, root, torch.device('cuda:0'))
        for rep in range(3):
            for name, fmt, kw in (('pyramid_tiff_deflate', '.ome.tiff', dict(ome_tiff_layout='pyramid')),
                                  ('blosc_store', '.ome.zarr', {})):
                st = Stitcher(StitchingParameters(input_folder=root, output_format=fmt, use_registration=True), **kw)
                t0 = time.time()
                with contextlib.redirect_stdout(io.StringIO()):
                    st.run()
                dt = time.time() - t0
                size = sum(os.path.getsize(os.path.join(dp, f)) for dp, _, fs in os.walk(st.output_folder) for f in fs)
                w, h = st.calculate_output_dimensions(0, st.regions[0])
                result.setdefault(name, {'seconds': [], 'bytes': size, 'levels': st.num_pyramid_levels, 'canvas': [h, w]})['seconds'].append(round(dt, 2))
                print(f'run {rep} {name}: {h} x {w} x 2 planes, {st.num_pyramid_levels} levels: {dt:.2f} s, {size} bytes', flush=True)
                shutil.rmtree(st.output_folder, ignore_errors=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(result), flush=True)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, 'deflate_probe_run.json'), 'w') as fh:
        json.dump(result, fh, indent=1)


if sys.argv[1] == 'kernel':
    kernel_probe(*(int(v) for v in sys.argv[2:4]))
elif sys.argv[1] == 'run':
    run_probe()
else:
    sys.exit(__doc__)
