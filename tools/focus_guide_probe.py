"""Device probe of the best-focus projection with a guide channel (sq_focus_depth_plane, sq_fuse_select_depth) on the four
channels of config 3: per channel 16 x 16 tiles of 2048^2 uint16 from sq_synth_tiles at config-3 placement, 10 z planes, one
float32 gain image, R = 3, focus-only.  ~110 GB of device memory (4 x 21 GB of tiles, the focus scratch, outputs and keys, and
one channel's 10-plane stack for the check).

Times, by HIP events after warm-up, alternating in this process on the same buffers:
  * baseline: four independent fuse_project_focus channel projections (what a run without a guide does);
  * guided:   one fuse_project_focus (the guide, channel 0) + focus_depth_plane + three fuse_select_depth channels;
  * the select kernel of one channel alone (algorithmic bytes: 1 B of depth read and 2 B written per canvas voxel, 2 B of
    pixel + 4 B of gain read per covered voxel) and its fraction of the HBM peak;
  * focus_depth_plane against the torch expression of native.depth_of_keys on one plane.
Checks one follower voxel by voxel against the fused stack (sq_fuse_planes) gathered at the guide's depth.  Prints one JSON
line (--json writes it to a file too).  Under a kernel trace the per-kernel times of focus_canvas_kernel and
select_depth_kernel can be read side by side."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from image_stitcher_amd import native, placement, synth  # noqa: E402

PEAK_GBS = 8000.0


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--grid', type=int, default=16)
    ap.add_argument('--tile', type=int, default=2048)
    ap.add_argument('--ov', type=int, default=244)
    ap.add_argument('--nz', type=int, default=10)
    ap.add_argument('--channels', type=int, default=4)
    ap.add_argument('--radius', type=int, default=3)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--flags', type=int, default=0, help='sq_fuse_flags of the canvas kernels (1 queues, 2 static walk)')
    ap.add_argument('--no-check', action='store_true', help='skip the voxel-by-voxel check (and its 10-plane stack)')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    g, T, Z, R, C = a.grid, a.tile, a.nz, a.radius, a.channels
    shifts = placement.Shifts((3, -a.ov), (-a.ov, -2))
    rects = placement.grid_rects(g, g, T, T, shifts, crop=True)
    wc, hc = placement.canvas_size(g, g, T, T, use_registration=True, shifts=shifts)
    plan = native.FusePlan(rects, T, T, hc, wc, expand_on_device=True)
    spec = synth.GridSpec(rows=g, cols=g, tile_h=T, tile_w=T, ov_y=a.ov, ov_x=a.ov, seed=1)
    tiles = [torch.empty((Z, g * g, T, T), dtype=torch.uint16, device=dev) for _ in range(C)]
    for c in range(C):
        for z in range(Z):
            desc = np.zeros(g * g, dtype=native.SYNTH_DTYPE)
            for r in range(g):
                for k in range(g):
                    oy, ox = spec.origin(r, k)
                    desc[r * g + k] = (spec.scene_seed(0, 0, z, c) % 2**64, spec.noise_seed(0, 0, z, c, r * g + k) % 2**64, oy, ox)
            native.synth_tiles(desc, T, T, spec.noise, 'uint16', dev, out=tiles[c][z])
    gains = [torch.from_numpy(synth.synthetic_flatfield(T, T, np.float32) * np.float32(1 + 0.01 * c)).to(dev) for c in range(C)]
    flats = [[gains[c]] * Z for c in range(C)]
    flat_ptrs = [native.pointer_table(flats[c], dev) for c in range(C)]
    zl = torch.arange(Z, dtype=torch.int32, device=dev)
    scratch = torch.empty(native.focus_scratch_bytes(g * g, T, T), dtype=torch.uint8, device=dev)
    out = torch.empty((C, hc, wc), dtype=torch.uint16, device=dev)
    key = torch.empty((C, hc, wc), dtype=torch.int64, device=dev)
    guided = torch.empty((C, hc, wc), dtype=torch.uint16, device=dev)
    depth = torch.empty((hc, wc), dtype=torch.uint8, device=dev)

    def focus(c, dst):
        native.fuse_project_focus(plan, tiles[c], dst[c], key[c], zl, R, flats[c], scratch=scratch, flat_ptrs=flat_ptrs[c],
                                  flags=a.flags)

    def select(c):
        native.fuse_select_depth(plan, tiles[c], guided[c], depth, zl, flats[c], flat_ptrs=flat_ptrs[c], flags=a.flags)

    def baseline():
        for c in range(C):
            focus(c, out)

    def with_guide():
        focus(0, guided)
        native.focus_depth_plane(key[0], out=depth)
        for c in range(1, C):
            select(c)

    torch_depth = [None]

    def depth_torch():
        torch_depth[0] = native.depth_of_keys(key[0])

    for _ in range(a.warmup):
        baseline()
        with_guide()
        depth_torch()
    torch.cuda.synchronize()
    ev = {'baseline': [], 'guided': [], 'select': [], 'depth_kernel': [], 'depth_torch': []}
    for _ in range(a.steps):      # alternating: they share the card's state
        ev['baseline'].append(timed(baseline))
        ev['guided'].append(timed(with_guide))
        ev['select'].append(timed(lambda: select(1)))
        ev['depth_kernel'].append(timed(lambda: native.focus_depth_plane(key[0], out=depth)))
        ev['depth_torch'].append(timed(depth_torch))
    torch.cuda.synchronize()
    ms = {k: np.array([e0.elapsed_time(e1) for e0, e1 in v]) for k, v in ev.items()}
    med = {k: float(np.median(v)) for k, v in ms.items()}
    depth_ok = bool(torch.equal(depth.to(torch.int64), torch_depth[0] + 1))
    mismatch = None
    if not a.no_check:
        stack = native.empty_canvas(Z, hc, wc, torch.uint16, dev)
        native.fuse_planes(plan, tiles[1], stack, flats[1], flat_ptrs=flat_ptrs[1])
        d = torch_depth[0]
        want = torch.gather(stack.view(torch.int16), 0, d.clamp(min=0)[None])[0]
        want = torch.where(d < 0, torch.zeros_like(want), want)
        mismatch = int((want != guided[1].view(torch.int16)).sum())
        del stack, want
    cov = plan.covered_voxels
    select_bytes = hc * wc * (1 + 2) + cov * (2 + 4)
    depth_bytes = hc * wc * (8 + 1)
    res = {
        'workload': f'{C} channels of {g}x{g} x {T}^2 uint16, {Z} z, float32 gains, R = {R} (config 3), focus-only',
        'canvas': [hc, wc], 'covered_voxels': int(cov), 'steps': a.steps, 'flags': a.flags,
        'baseline': f'{C} independent fuse_project_focus channel projections',
        'baseline_ms': med['baseline'], 'baseline_ms_min': float(ms['baseline'].min()),
        'guided': f'1 fuse_project_focus + focus_depth_plane + {C - 1} fuse_select_depth',
        'guided_ms': med['guided'], 'guided_ms_min': float(ms['guided'].min()),
        'speedup': med['baseline'] / med['guided'],
        'select_ms_per_channel': med['select'], 'select_ms_min': float(ms['select'].min()),
        'select_algorithmic_gb': select_bytes / 1e9, 'select_gbs': select_bytes / med['select'] / 1e6,
        'select_fraction_of_peak': select_bytes / med['select'] / 1e6 / PEAK_GBS,
        'depth_kernel_ms': med['depth_kernel'], 'depth_kernel_gbs': depth_bytes / med['depth_kernel'] / 1e6,
        'depth_torch_ms': med['depth_torch'], 'depth_kernel_equals_torch': depth_ok,
        'follower_vs_stack_at_depth_mismatches': mismatch,
    }
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, 'w') as fh:
            fh.write(line + '\n')
    if mismatch or not depth_ok:
        sys.exit(1)


if __name__ == '__main__':
    main()
