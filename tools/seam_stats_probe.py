"""Time sq_seam_stats on the staged tiles of one config-3 plane (16 x 16 tiles of 2048 x 2048 uint16 with 10 % overlap from the
device generator; HIP events after warm-up, one process, a time limit of its own) against

    (a) sq_seam_stats at R = 0, 2 and 3        one launch (plus the zero-fill of the words) over every seam of the plane
    (b) sq_pair_overlap_moments                the existing kernel over the R = 0 core windows: the same five sums per seam, the
                                               baseline of (a) at R = 0 (equality of the shared sums is checked); it reads its
                                               table back, so its time includes a synchronise
    (c) torch.amax over as many bytes          a plain reduction read of as many bytes of the staged tiles as the R = 0 windows hold

The launches alternate so that whatever else the box does lands on all of them; the medians are quoted.

    python tools/seam_stats_probe.py [reps]      -> profiles/seam_stats_probe_kernel.json
"""
import json
import os
import signal
import sys

import numpy as np
import torch

sys.path.insert(0, '.')
from image_stitcher_amd import native, seamqc

OUT = os.environ.get('SQ_PROBE_OUT', 'profiles')
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
H = W = 2048
GRID, STEP = 16, 2048 - 205
signal.alarm(int(os.environ.get('SQ_PROBE_LIMIT_S', 300)))      # the probe ends itself: nothing here should take minutes
dev = torch.device('cuda:0')

n = GRID * GRID
desc = np.zeros(n, dtype=native.SYNTH_DTYPE)      # overlapping views of one scene, a noise seed per tile
for i in range(n):
    desc[i] = (4242, 977 + i, (i // GRID) * STEP, (i % GRID) * STEP)
src = native.synth_tiles(desc, H, W, 300, np.uint16, dev).view(1, n, H, W)
rects = {i: (0, 0, H, W, (i // GRID) * STEP, (i % GRID) * STEP) for i in range(n)}


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(times):
    return {'ms': round(sorted(times)[len(times) // 2], 4), 'ms_min': round(min(times), 4), 'ms_max': round(max(times), 4)}


launches, tables, words = {}, {}, {}
for radius in (0, 2, 3):
    seams = seamqc.region_seams(rects, H, W, radius, 256)
    table = native.as_overlaps(seamqc.pair_table(seams, {i: i for i in range(n)}))
    tables[radius] = (seams, table, native.seam_pairs_to_device(table, dev))
    words[radius] = torch.empty((1, len(table), native.seam_words(radius)), dtype=torch.int64, device=dev)
    launches[f'a_seam_stats_r{radius}'] = (lambda r=radius: native.seam_stats(src, tables[r][1], r, out=words[r], pairs_dev=tables[r][2]))
table0 = tables[0][1]
moments = torch.empty((len(table0), 5), dtype=torch.int64, device=dev)
window_bytes = int(2 * 2 * (table0['h'].astype(np.int64) * table0['w']).sum())      # two windows per seam, 2 bytes a pixel
flat = src.view(-1).view(torch.int16)[:window_bytes // 2]
launches['b_overlap_moments'] = lambda: native.pair_overlap_moments(src[0], table0, out=moments)
launches['c_amax_read'] = lambda: flat.amax()

times = {k: [] for k in launches}
for i in range(reps + 3):      # three warm-up rounds
    for k, fn in launches.items():
        t = once(fn)
        if i >= 3:
            times[k].append(t)
result = {'tiles': n, 'shape': [H, W], 'dtype': 'uint16', 'overlap_px': H - STEP, 'reps': reps, 'window_bytes_r0': window_bytes,
          'seams': {str(r): len(tables[r][1]) for r in tables},
          'core_pixels': {str(r): int((tables[r][1]['h'].astype(np.int64) * tables[r][1]['w']).sum()) for r in tables}}
for k in launches:
    result[k] = stats(times[k])
w0, m = words[0][0].cpu().numpy(), moments.cpu().numpy()      # Sa, Saa, Sad, Sb, Sbb, Sab against Sa, Sb, Saa, Sbb, Sab
result['equal_to_overlap_moments'] = bool((w0[:, [0, 3, 1, 4, 5]] == m).all())
a0, a2, a3 = (result[f'a_seam_stats_r{r}']['ms'] for r in (0, 2, 3))
b, c = result['b_overlap_moments']['ms'], result['c_amax_read']['ms']
result['r0_over_overlap_moments'] = round(a0 / b, 3)
result['r0_over_read'] = round(a0 / c, 3)
result['r2_over_r0'] = round(a2 / a0, 3)
result['r3_over_r0'] = round(a3 / a0, 3)
result['r3_ns_per_pixel_offset'] = round(a3 * 1e6 / (result['core_pixels']['3'] * 49), 5)
print(f"seam_stats R=0 {a0:.3f} ms, R=2 {a2:.3f} ms, R=3 {a3:.3f} ms over {result['seams']['3']} seams; overlap_moments {b:.3f} ms; "
      f"amax over {window_bytes / 1e6:.0f} MB {c:.3f} ms; R=0 / moments = {result['r0_over_overlap_moments']:.2f}; equal "
      f"{result['equal_to_overlap_moments']}", flush=True)
print(json.dumps(result))
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, 'seam_stats_probe_kernel.json'), 'w') as fh:
    json.dump(result, fh, indent=1)
