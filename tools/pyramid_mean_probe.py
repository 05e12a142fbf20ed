"""Time the pyramid levels 1..5 of a config-3-sized canvas plane batch (4 planes of 36 428 x 29 108 uint16; HIP events, one
process) three ways and report the HBM rate of each:

    (a) nearest chain   five sq_downsample2 launches (the default method)          algorithmic bytes 1.00 x level 0
    (b) mean one-pass   ONE sq_pyramid_mean launch for all five levels                               1.33 x
    (c) mean per level  five sq_pyramid_mean launches with n = 1 (for information)                   1.67 x

Algorithmic bytes: (a) per level the odd source rows read whole + the level written = 3/4 of the level before, summed over the
levels 3/4 * 4/3; (b) level 0 read once + every level written 1 + 1/3; (c) every level read whole + written 5/4 * 4/3.

    python tools/pyramid_mean_probe.py [planes [reps]]
    python tools/pyramid_mean_probe.py run      what the option costs end to end: Stitcher.run (files -> registration -> fusion ->
                                                levels -> Blosc chunks -> store, all on /dev/shm) on 4 wells of 4 x 4 tiles of
                                                2048^2, 2 channels x 2 z, with either method: wall time per region
"""
import json
import sys

import torch

sys.path.insert(0, '.')
from image_stitcher_amd import native


def run_probe():
    import contextlib, io, os, shutil, tempfile, time
    from image_stitcher_amd import synth
    from image_stitcher_amd.stitcher import Stitcher
    from image_stitcher_amd.stitcher_parameters import StitchingParameters
    wells = ('A1', 'A2', 'A3', 'A4')
    spec = synth.GridSpec(rows=4, cols=4, tile_h=2048, tile_w=2048, ov_y=244, ov_x=244, seed=5100,
                          channels=synth.DEFAULT_CHANNELS[:2], nz=2, nt=1, regions=wells)
    tmp = tempfile.mkdtemp(prefix='pyrmean_', dir='/dev/shm')
    result = {'wells': len(wells), 'grid': '4x4 of 2048^2', 'planes_per_region': 4}
    try:
        root = os.path.join(tmp, 'acq')
        synth.write_acquisition_device(spec, root, torch.device('cuda:0'))
        for rep in range(3):
            for method in ('nearest', 'mean'):
                st = Stitcher(StitchingParameters(input_folder=root, use_registration=True), pyramid_method=method)
                t0 = time.time()
                with contextlib.redirect_stdout(io.StringIO()):
                    st.run()
                dt = time.time() - t0
                w, h = st.calculate_output_dimensions(0, st.regions[0])
                result.setdefault(method, []).append(round(dt / len(wells) * 1e3, 1))
                print(f'run {rep} {method:8s}: {len(wells)} regions of {h} x {w} x 4 planes, {st.num_pyramid_levels} levels: {dt:.2f} s = '
                      f'{dt / len(wells) * 1e3:.0f} ms per region', flush=True)
                shutil.rmtree(st.output_folder, ignore_errors=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps({'stitcher_run_ms_per_region': result}))


if len(sys.argv) > 1 and sys.argv[1] == 'run':
    run_probe()
    sys.exit(0)

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
h, w, levels = 36428, 29108, 5
a = torch.empty((n, h, w), dtype=torch.uint16, device='cuda')
a.view(torch.int16).random_(-30000, 30000)
outs = [torch.empty((n, h >> k, w >> k), dtype=torch.uint16, device='cuda') for k in range(1, levels + 1)]
level0_bytes = a.numel() * 2


def nearest_chain():
    src = a
    for o in outs:
        native.downsample2(src, out=o)
        src = o


def mean_one_pass():
    native.pyramid_mean(a, levels, out=outs)


def mean_per_level():
    src = a
    for o in outs:
        native.pyramid_mean(src, 1, out=[o])
        src = o


def timed(fn):
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


result = {'planes': n, 'shape': [h, w], 'dtype': 'uint16', 'levels': levels, 'reps': reps, 'level0_bytes': level0_bytes}
geo = sum(0.25 ** k for k in range(levels))          # 1 + 1/4 + ... over the five source levels
for key, fn, factor in (('a_nearest_chain', nearest_chain, 0.75 * geo),
                        ('b_mean_one_pass', mean_one_pass, 1 + 0.25 * geo),
                        ('c_mean_per_level', mean_per_level, 1.25 * geo)):
    ms, lo, hi = timed(fn)
    alg = level0_bytes * factor
    result[key] = {'ms': round(ms, 3), 'ms_min': round(lo, 3), 'ms_max': round(hi, 3), 'algorithmic_bytes': int(alg),
                   'bytes_x_level0': round(factor, 3), 'gb_per_s': round(alg / ms / 1e6, 1),
                   'of_8_tb_per_s': round(alg / ms / 1e6 / 8000, 3)}
    print(f"{key:17s} {ms:7.3f} ms (min {lo:.3f}, max {hi:.3f})  {factor:.2f} x level 0 = {alg / 1e9:.2f} GB  "
          f"{alg / ms / 1e6:6.0f} GB/s algorithmic ({alg / ms / 1e6 / 8000:.3f} of 8 TB/s)", flush=True)
# the one-pass levels against the per-level ones (the definition composes)
mean_one_pass()
one = [o.clone() for o in outs]
mean_per_level()
result['one_pass_equals_per_level'] = all(torch.equal(x, y) for x, y in zip(one, outs))
ra, rb, rc = (result[k]['ms'] for k in ('a_nearest_chain', 'b_mean_one_pass', 'c_mean_per_level'))
result['b_over_a'] = round(rb / ra, 3)
result['target_b_over_a'] = round(1.33 * 1.10, 3)
result['b_over_c'] = round(rb / rc, 3)
print(f"one-pass / nearest chain = {rb / ra:.3f} (target <= {1.33 * 1.10:.3f}); one-pass / per-level mean = {rb / rc:.3f}; "
      f"one-pass levels equal the per-level ones: {result['one_pass_equals_per_level']}")
print(json.dumps(result))
