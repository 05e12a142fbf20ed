"""Time sq_dark_tiles on the staged tiles of one config-3 plane (256 tiles of 2048 x 2048 uint16 from the device generator; HIP
events after warm-up, one process, a time limit of its own), in place over the batch:

    (a) the frame path         one frame for all tiles: 2 bytes read and 2 written per pixel, plus the frame
    (b) the constant path      no frame
    (c) the frame path of a build with the other SQ_DARK_IMAGES_PER_THREAD -- 4 where the library has 1, 1 where it has another
        value -- a second library made from csrc/dark.hip alone: what the walk over the images of a run buys

against two yardsticks measured in the same loop, so all see the same neighbours on the box:

    (d) a device copy of the same batch        the same bytes read and written
    (e) sq_dpc_tiles in place                  2 + 2 bytes read and 2 written per pixel

    python tools/dark_probe.py --build            compiles the library of (c) for gfx950 (no device needed)
    python tools/dark_probe.py [tiles [reps]]     -> profiles/dark_probe_kernel.json
"""
import ctypes
import json
import os
import signal
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'image-stitcher_amd', 'csrc')
ONE_DIR = os.path.join(CSRC, 'build_dark_alt')
ONE_LIB = os.path.join(ONE_DIR, 'libdark_alt.so')
SHIM = '#include <string>\nnamespace sq { std::string &last_error_ref() { static thread_local std::string e; return e; } }\n'


def alt_images_per_thread():
    with open(os.path.join(ROOT, 'include', 'squidstitch.h')) as fh:
        return 4 if '#define SQ_DARK_IMAGES_PER_THREAD 1\n' in fh.read() else 1


def build_one():
    """csrc/dark.hip with the other number of images per thread, and the error string it reports into, as a library of its own."""
    os.makedirs(ONE_DIR, exist_ok=True)
    shim = os.path.join(ONE_DIR, 'shim.cpp')
    with open(shim, 'w') as fh:
        fh.write(SHIM)
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    subprocess.run([hipcc, '-O3', '-std=c++17', '-fPIC', '-shared', '--offload-arch=gfx950', '-ffp-contract=off',
                    f'-DSQ_DARK_IMAGES_PER_THREAD={alt_images_per_thread()}', '-x', 'hip', os.path.join(CSRC, 'dark.hip'), shim, '-o', ONE_LIB], check=True)
    return ONE_LIB


if __name__ == '__main__' and '--build' in sys.argv:
    print(build_one())
    sys.exit(0)

import numpy as np
import torch

sys.path.insert(0, ROOT)
from image_stitcher_amd import native

OUT = os.environ.get('SQ_PROBE_OUT', 'profiles')
n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 15
H = W = 2048
PEDESTAL, CONSTANT = 100, 1100
signal.alarm(int(os.environ.get('SQ_PROBE_LIMIT_S', 300)))      # the probe ends itself: nothing here should take minutes
dev = torch.device('cuda:0')


def tiles(scene, noise):      # a 16 x 16 grid of overlapping views of one scene, a noise seed per tile
    desc = np.zeros(n, dtype=native.SYNTH_DTYPE)
    for i in range(n):
        desc[i] = (scene, noise + i, (i // 16) * 1804, (i % 16) * 1804)
    return native.synth_tiles(desc, H, W, 300, np.uint16, dev)


src, right = tiles(4242, 977), tiles(5151, 40977)
work, spare = src.clone(), torch.empty_like(src)
rng = np.random.default_rng(3)
frame_np = (1000 + rng.integers(0, 200, (1, H, W))).astype(np.uint16)      # a pedestal of a thousand counts with noise
frame = torch.from_numpy(frame_np).to(dev)
nbytes = src.numel() * 2

one = None
if os.path.exists(ONE_LIB):
    one = ctypes.CDLL(ONE_LIB)
    one.sq_dark_tiles.restype = ctypes.c_int
    one.sq_dark_tiles.argtypes = native.EXPORTS['sq_dark_tiles'][1]


def dark_one():
    table = (ctypes.c_int32 * 2)(0, 0)
    status = one.sq_dark_tiles(work.data_ptr(), n, H, W, H * W, W, native.SQ_U16, frame.data_ptr(), 1, H * W, W, table, n, PEDESTAL,
                               int(torch.cuda.current_stream().cuda_stream))
    assert status == 0, status


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(times):
    return {'ms': round(sorted(times)[len(times) // 2], 3), 'ms_min': round(min(times), 3), 'ms_max': round(max(times), 3)}


# equality first, on eight tiles: both builds against the definition in torch
want = (src[:8].to(torch.int32) - frame.to(torch.int32) + PEDESTAL).clamp(0, 65535)
got = native.dark_tiles(src[:8].clone(), (0, 0), frames=frame, pedestal=PEDESTAL)
equal = {'frame': bool(torch.equal(got.to(torch.int32), want))}
got = native.dark_tiles(src[:8].clone(), (-1, CONSTANT), pedestal=PEDESTAL)
equal['constant'] = bool(torch.equal(got.to(torch.int32), (src[:8].to(torch.int32) - CONSTANT + PEDESTAL).clamp(0, 65535)))
if one is not None:
    work.copy_(src)
    dark_one()
    equal['frame_other_build'] = bool(torch.equal(work[:8].to(torch.int32), want))
    work.copy_(src)

legs = {'a_frame': lambda: native.dark_tiles(work, (0, 0), frames=frame, pedestal=PEDESTAL),
        'b_constant': lambda: native.dark_tiles(work, (-1, CONSTANT), pedestal=PEDESTAL),
        'd_device_copy': lambda: spare.copy_(work),
        'e_dpc_in_place': lambda: native.dpc_tiles(work, right, 1)}
if one is not None:
    legs['c_frame_other_build'] = dark_one
times = {name: [] for name in legs}
for i in range(reps + 3):      # three warm-up rounds; the values of work drift, the bytes moved do not
    for name, fn in legs.items():
        t = event_ms(fn)
        if i >= 3:
            times[name].append(t)
result = {'tiles': n, 'shape': [H, W], 'dtype': 'uint16', 'reps': reps, 'bytes_read_and_written': 2 * nbytes,
          'images_per_thread': native.SQ_DARK_IMAGES_PER_THREAD,
          'images_per_thread_other_build': alt_images_per_thread() if one is not None else None, 'equal': equal}
for name in legs:
    result[name] = stats(times[name])
    moved = (3 if name == 'e_dpc_in_place' else 2) * nbytes
    result[name]['gb_per_s'] = round(moved / result[name]['ms'] / 1e6, 1)
copy_ms, dpc_ms = result['d_device_copy']['ms'], result['e_dpc_in_place']['ms']
result['ratios'] = {name + '_over_copy': round(result[name]['ms'] / copy_ms, 3) for name in legs if name[0] in 'abc'}
result['ratios'].update({name + '_over_dpc': round(result[name]['ms'] / dpc_ms, 3) for name in legs if name[0] in 'abc'})
if one is not None:
    result['ratios']['a_frame_over_c_other_build'] = round(result['a_frame']['ms'] / result['c_frame_other_build']['ms'], 3)
result['all_equal'] = all(equal.values())
for name in legs:
    print(f"{name}: {result[name]['ms']:.3f} ms = {result[name]['gb_per_s']:.0f} GB/s", flush=True)
print(json.dumps(result))
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, 'dark_probe_kernel.json'), 'w') as fh:
    json.dump(result, fh, indent=1)
