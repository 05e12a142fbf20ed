"""Time sq_histogram_planes on a config-3-sized canvas plane batch (4 planes of 36 428 x 29 108 uint16; HIP events, one process)
with three contents -- a synthetic fused canvas (zero border, a clustered background, sparse bright signal, a saturated patch),
a constant plane (worst contention), uniform random values (worst spread) -- three ways:

    (a) sq_histogram_planes                         one launch for the batch
    (b) torch.bincount on the device                what a user has without it (int32 copies of row blocks, as bincount requires)
    (c) torch.amax over the same bytes              a plain reduction read: the roof

    python tools/histogram_probe.py [planes [reps]]      -> profiles/histogram_probe_kernel.json
    python tools/histogram_probe.py run                  what the option costs end to end: Stitcher.run on 4 wells of 4 x 4 tiles
                                                         of 2048^2, 2 channels x 2 z, on /dev/shm, --contrast-limits dtype against
                                                         percentile, three repetitions each -> profiles/histogram_probe_run.json
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
    tmp = tempfile.mkdtemp(prefix='histprobe_', dir='/dev/shm')
    result = {'wells': len(wells), 'grid': '4x4 of 2048^2', 'planes_per_region': 4}
    try:
        root = os.path.join(tmp, 'acq')
        synth.write_acquisition_device(spec, root, torch.device('cuda:0'))
        for rep in range(3):
            for mode in ('dtype', 'percentile'):
                kw = {'contrast_limits': mode} if mode != 'dtype' or 'contrast_limits' in Stitcher.__init__.__code__.co_varnames else {}
                st = Stitcher(StitchingParameters(input_folder=root, use_registration=True), **kw)
                t0 = time.time()
                with contextlib.redirect_stdout(io.StringIO()):
                    st.run()
                dt = time.time() - t0
                result.setdefault(mode, []).append(round(dt / len(wells) * 1e3, 1))
                print(f'run {rep} {mode:10s}: {dt:.2f} s = {dt / len(wells) * 1e3:.0f} ms per region', flush=True)
                shutil.rmtree(st.output_folder, ignore_errors=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps({'stitcher_run_ms_per_region': result}))
    with open(os.path.join(OUT, 'histogram_probe_run.json'), 'w') as fh:
        json.dump({'stitcher_run_ms_per_region': result}, fh, indent=1)


if len(sys.argv) > 1 and sys.argv[1] == 'run':
    run_probe()
    sys.exit(0)

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
h, w = 36428, 29108
a = torch.empty((n, h, w), dtype=torch.uint16, device='cuda')
hist = torch.zeros((1, 65536), dtype=torch.int64, device='cuda')
ROWS = 2048


def fill(kind):
    g = torch.Generator(device='cuda').manual_seed(9)
    for p in range(n):
        for y in range(0, h, ROWS):
            rows = min(ROWS, h - y)
            if kind == 'constant':
                a[p, y:y + rows] = 1000
            elif kind == 'uniform':
                a[p, y:y + rows] = torch.randint(0, 65536, (rows, w), generator=g, device='cuda', dtype=torch.int32).to(torch.uint16)
            else:       # background 100 +- 8, one voxel in 50 a bright signal up to 4000
                bg = (torch.randn((rows, w), generator=g, device='cuda') * 8 + 100).clamp_(1, 65535)
                sig = torch.rand((rows, w), generator=g, device='cuda')
                bg = torch.where(sig < 0.02, 200 + sig * 50 * 3800, bg)
                a[p, y:y + rows] = bg.to(torch.int32).to(torch.uint16)
        if kind == 'canvas':   # the canvas is larger than the tiles' union; one saturated patch
            a[p, :1500] = 0
            a[p, :, :1200] = 0
            a[p, 20000:20400, 8000:9000] = 65535


def ours():
    native.histogram_planes(a, [0] * n, hist=hist)


def bincount():
    out = torch.zeros(65536, dtype=torch.int64, device='cuda')
    for p in range(n):
        for y in range(0, h, ROWS):
            out += torch.bincount(a[p, y:y + ROWS].to(torch.int32).flatten(), minlength=65536)
    return out


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
result = {'planes': n, 'shape': [h, w], 'dtype': 'uint16', 'reps': reps, 'bytes': nbytes}
for kind in ('canvas', 'constant', 'uniform'):
    fill(kind)
    hist.zero_()
    ours()
    exact = bool(torch.equal(hist[0], bincount()))
    row = {'exact': exact}
    for key, fn, r in (('a_histogram_planes', ours, reps), ('b_torch_bincount', bincount, max(2, reps // 3)), ('c_amax_read', amax, reps)):
        ms, lo, hi = timed(fn, r)
        row[key] = {'ms': round(ms, 3), 'ms_min': round(lo, 3), 'ms_max': round(hi, 3), 'gb_per_s': round(nbytes / ms / 1e6, 1)}
    row['a_fraction_of_read_roof'] = round(row['c_amax_read']['ms'] / row['a_histogram_planes']['ms'], 3)
    row['b_over_a'] = round(row['b_torch_bincount']['ms'] / row['a_histogram_planes']['ms'], 2)
    result[kind] = row
    print(f"{kind:9s} exact {exact}  (a) {row['a_histogram_planes']['ms']:8.3f} ms {row['a_histogram_planes']['gb_per_s']:7.0f} GB/s   "
          f"(b) {row['b_torch_bincount']['ms']:9.3f} ms   (c) {row['c_amax_read']['ms']:7.3f} ms {row['c_amax_read']['gb_per_s']:7.0f} GB/s   "
          f"a = {row['a_fraction_of_read_roof']:.3f} of the read roof, bincount / a = {row['b_over_a']:.1f}", flush=True)
result['a_faster_than_b_everywhere'] = all(result[k]['b_over_a'] > 1 for k in ('canvas', 'constant', 'uniform'))
print(json.dumps(result))
with open(os.path.join(OUT, 'histogram_probe_kernel.json'), 'w') as fh:
    json.dump(result, fh, indent=1)
