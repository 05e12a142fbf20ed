"""Time sq_block_mean on a config-3-sized plane batch (4 planes of 36 428 x 29 108 uint16, k = 4 at the default
--composite-max-side of 4096; HIP events, one process, median of 5) three ways:

    (a) sq_block_mean                               one launch for the batch
    (b) the same means with torch                   what a user has without it: int32 copies of row blocks, zero padding to whole
                                                    blocks, reshape / sum, an integer divide by the blocks' pixel counts
    (c) torch.amax over the same bytes              a plain reduction read: the roof (the yardstick of DESIGN.md 5.4b)

    python tools/composite_probe.py [planes [reps]]      -> profiles/composite_probe_kernel.json
    python tools/composite_probe.py run                  what the option costs end to end: the plate workload of
                                                         tools/histogram_probe.py run (4 wells of 4 x 4 tiles of 2048^2, 2 channels
                                                         x 2 z, on /dev/shm), --composite off against on, three alternating
                                                         repetitions -> profiles/composite_probe_run.json
"""
import json
import os
import sys

import torch

sys.path.insert(0, '.')
from image_stitcher_amd import native

OUT = os.environ.get('SQ_PROBE_OUT', 'profiles')


def run_probe():
    import contextlib, io, shutil, tempfile, time
    from image_stitcher_amd import synth
    from image_stitcher_amd.stitcher import Stitcher
    from image_stitcher_amd.stitcher_parameters import StitchingParameters
    wells = ('A1', 'A2', 'A3', 'A4')
    spec = synth.GridSpec(rows=4, cols=4, tile_h=2048, tile_w=2048, ov_y=244, ov_x=244, seed=5100,
                          channels=synth.DEFAULT_CHANNELS[:2], nz=2, nt=1, regions=wells)
    tmp = tempfile.mkdtemp(prefix='compprobe_', dir='/dev/shm')
    result = {'wells': len(wells), 'grid': '4x4 of 2048^2', 'planes_per_region': 4}
    try:
        root = os.path.join(tmp, 'acq')
        synth.write_acquisition_device(spec, root, torch.device('cuda:0'))
        for rep in range(3):
            for mode in ('off', 'on'):
                st = Stitcher(StitchingParameters(input_folder=root, use_registration=True), composite=mode == 'on')
                t0 = time.time()
                with contextlib.redirect_stdout(io.StringIO()):
                    st.run()
                dt = time.time() - t0
                result.setdefault(mode, []).append(round(dt / len(wells) * 1e3, 1))
                print(f'run {rep} composite {mode:3s}: {dt:.2f} s = {dt / len(wells) * 1e3:.0f} ms per region', flush=True)
                shutil.rmtree(st.output_folder, ignore_errors=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps({'stitcher_run_ms_per_region': result}))
    with open(os.path.join(OUT, 'composite_probe_run.json'), 'w') as fh:
        json.dump({'stitcher_run_ms_per_region': result}, fh, indent=1)


if len(sys.argv) > 1 and sys.argv[1] == 'run':
    run_probe()
    sys.exit(0)

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
K = 4
F = 1 << K
h, w = 36428, 29108
ho, wo = -(-h // F), -(-w // F)
a = torch.empty((n, h, w), dtype=torch.uint16, device='cuda')
out = torch.empty((n, ho, wo), dtype=torch.uint16, device='cuda')
ROWS = 2048      # a multiple of F

g = torch.Generator(device='cuda').manual_seed(9)
for p in range(n):      # background 100 +- 8, one voxel in 50 a bright signal up to 4000, a zero border, one saturated patch
    for y in range(0, h, ROWS):
        rows = min(ROWS, h - y)
        bg = (torch.randn((rows, w), generator=g, device='cuda') * 8 + 100).clamp_(1, 65535)
        sig = torch.rand((rows, w), generator=g, device='cuda')
        bg = torch.where(sig < 0.02, 200 + sig * 50 * 3800, bg)
        a[p, y:y + rows] = bg.to(torch.int32).to(torch.uint16)
    a[p, :1500] = 0
    a[p, :, :1200] = 0
    a[p, 20000:20400, 8000:9000] = 65535

ones = torch.zeros((ho * F, wo * F), dtype=torch.int32, device='cuda')
ones[:h, :w] = 1
counts = ones.view(ho, F, wo, F).sum(dim=(1, 3))
del ones


def ours():
    native.block_mean(a, K, out=out)
    return out


def with_torch():
    res = torch.empty((n, ho, wo), dtype=torch.int32, device='cuda')
    for p in range(n):
        for y in range(0, h, ROWS):
            rows = min(ROWS, h - y)
            ro = -(-rows // F)
            x = torch.nn.functional.pad(a[p, y:y + rows].to(torch.int32), (0, wo * F - w, 0, ro * F - rows))
            res[p, y // F:y // F + ro] = x.view(ro, F, wo, F).sum(dim=(1, 3))      # 65535 * 256 < 2^31
    return torch.div(res, counts, rounding_mode='floor')


def amax():
    return a.view(torch.int16).amax()


def timed(fn, reps):
    for _ in range(2):
        fn()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return sorted(times)[len(times) // 2], min(times), max(times)


nbytes = a.numel() * 2
equal = bool(torch.equal(ours().to(torch.int32), with_torch()))
result = {'planes': n, 'shape': [h, w], 'dtype': 'uint16', 'k': K, 'reps': reps, 'bytes': nbytes, 'equal': equal}
for key, fn in (('a_block_mean', ours), ('b_torch', with_torch), ('c_amax_read', amax)):
    ms, lo, hi = timed(fn, reps)
    result[key] = {'ms': round(ms, 3), 'ms_min': round(lo, 3), 'ms_max': round(hi, 3), 'gb_per_s': round(nbytes / ms / 1e6, 1)}
result['a_fraction_of_read_roof'] = round(result['c_amax_read']['ms'] / result['a_block_mean']['ms'], 3)
result['b_over_a'] = round(result['b_torch']['ms'] / result['a_block_mean']['ms'], 2)
result['a_faster_than_b'] = result['b_over_a'] > 1
print(json.dumps(result))
with open(os.path.join(OUT, 'composite_probe_kernel.json'), 'w') as fh:
    json.dump(result, fh, indent=1)
if not equal or not result['a_faster_than_b']:
    sys.exit(1)
