"""Device probe of the z projection (sq_fuse_project_max) on one config-3-shaped channel: 16 x 16 tiles of 2048^2 uint16 from
sq_synth_tiles at config-3 placement, 10 z planes, one float32 gain image.  ~45 GB of device memory: 21 GB of tiles, the
projection and the baseline's 10-plane stack.

Times, by HIP events after warm-up and alternating in this process on the same buffers:
  * the projection launch (algorithmic bytes: Z x 2 B read per covered voxel + 2 B written per canvas voxel);
  * the baseline a host-side MIP would need on the device: sq_fuse_planes over the 10 planes, then torch.amax over z (of the
    stack's int16 view: the same bytes; torch has no uint16 max reduction on the device);
and checks that both give identical outputs.  Prints one JSON line (--json writes it to a file too)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from image_stitcher_amd import native, placement, synth  # noqa: E402

PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--grid', type=int, default=16)
    ap.add_argument('--tile', type=int, default=2048)
    ap.add_argument('--ov', type=int, default=244)
    ap.add_argument('--nz', type=int, default=10)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--flags', type=int, default=0, help='sq_fuse_flags of the projection launch (1 queues, 2 static walk)')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    g, T, Z = a.grid, a.tile, a.nz
    shifts = placement.Shifts((3, -a.ov), (-a.ov, -2))
    rects = placement.grid_rects(g, g, T, T, shifts, crop=True)
    wc, hc = placement.canvas_size(g, g, T, T, use_registration=True, shifts=shifts)
    plan = native.FusePlan(rects, T, T, hc, wc, expand_on_device=True)
    spec = synth.GridSpec(rows=g, cols=g, tile_h=T, tile_w=T, ov_y=a.ov, ov_x=a.ov, seed=1)
    tiles = torch.empty((Z, g * g, T, T), dtype=torch.uint16, device=dev)
    for z in range(Z):
        desc = np.zeros(g * g, dtype=native.SYNTH_DTYPE)
        for r in range(g):
            for c in range(g):
                oy, ox = spec.origin(r, c)
                desc[r * g + c] = (spec.scene_seed(0, 0, z, 0) % 2**64, spec.noise_seed(0, 0, z, 0, r * g + c) % 2**64, oy, ox)
        native.synth_tiles(desc, T, T, spec.noise, 'uint16', dev, out=tiles[z])
    gain = torch.from_numpy(synth.synthetic_flatfield(T, T, np.float32)).to(dev)
    flats = [gain] * Z
    flat_ptrs = native.pointer_table(flats, dev)
    stack = native.empty_canvas(Z, hc, wc, torch.uint16, dev)
    proj = torch.empty((hc, wc), dtype=torch.uint16, device=dev)
    base = torch.empty((hc, wc), dtype=torch.uint16, device=dev)

    def project():
        native.fuse_project_max(plan, tiles, proj, flats, flat_ptrs=flat_ptrs, flags=a.flags)

    def fuse_only():
        native.fuse_planes(plan, tiles, stack, flats, flat_ptrs=flat_ptrs)

    def amax():      # the reduction's traffic (torch has no uint16 max on the device: its int16 view moves the same bytes)
        torch.amax(stack.view(torch.int16), dim=0, out=base.view(torch.int16))

    for _ in range(a.warmup):
        project(), fuse_only(), amax()
    torch.cuda.synchronize()
    times = {'project': [], 'fuse': [], 'amax': []}
    for _ in range(a.steps):      # alternating: the three share the box's state
        for name, fn in (('project', project), ('fuse', fuse_only), ('amax', amax)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            times[name].append((e0, e1))
    torch.cuda.synchronize()
    ms = {k: np.array([e0.elapsed_time(e1) for e0, e1 in v]) for k, v in times.items()}
    flip = stack.view(torch.int16) ^ -32768      # the exact unsigned maximum for the check
    base = (flip.amax(0) ^ -32768).view(torch.uint16)
    del flip
    mismatched = int((proj != base).sum())
    cov = plan.covered_voxels
    proj_bytes = Z * cov * 2 + hc * wc * 2
    fuse_bytes = Z * (cov * 2 + hc * wc * 2)
    amax_bytes = Z * hc * wc * 2 + hc * wc * 2
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out = {
        'workload': f'{g}x{g} x {T}^2 uint16, {Z} z, float32 gains (one channel of config 3)', 'canvas': [hc, wc],
        'covered_voxels': int(cov), 'steps': a.steps, 'flags': a.flags,
        'project_ms': med['project'], 'project_ms_min': float(ms['project'].min()),
        'project_algorithmic_gb': proj_bytes / 1e9, 'project_gbs': proj_bytes / med['project'] / 1e6,
        'project_fraction_of_peak': proj_bytes / med['project'] / 1e6 / PEAK_GBS,
        'fuse_planes_ms': med['fuse'], 'fuse_planes_fraction_of_peak': fuse_bytes / med['fuse'] / 1e6 / PEAK_GBS,
        'amax_ms': med['amax'], 'amax_fraction_of_peak': amax_bytes / med['amax'] / 1e6 / PEAK_GBS,
        'baseline_ms': med['fuse'] + med['amax'], 'speedup_vs_baseline': (med['fuse'] + med['amax']) / med['project'],
        'mismatched_voxels': mismatched,
    }
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, 'w') as fh:
            fh.write(line + '\n')
    if mismatched:
        sys.exit(1)


if __name__ == '__main__':
    main()
