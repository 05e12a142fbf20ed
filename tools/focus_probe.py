"""Device probe of the best-focus projection (sq_fuse_project_focus) on one config-3-shaped channel: 16 x 16 tiles of 2048^2
uint16 from sq_synth_tiles at config-3 placement, 10 z planes, one float32 gain image, R = 3.  ~80 GB of device memory: 21 GB
of tiles, 5.4 GB of focus scratch, the output and its 8-byte key plane, and the baseline's 10-plane stack with its work planes.

Times, by HIP events after warm-up and alternating in this process on the same buffers:
  * the focus projection (both stages; algorithmic bytes: Z x 2 B read per tile pixel + 5 B written per tile pixel (the
    winners), then per covered voxel 5 B of winners + 2 B of the winning plane + 4 B of gain read, per canvas voxel 2 B of
    output + 8 B of key written);
  * the baseline without this kernel: sq_fuse_planes over the 10 planes, then a torch EDF of the fused STACK (int32 torch
    ops, plane by plane: the modified Laplacian and the (2R+1)^2 box sum on the canvas with its edges clamped, a running
    argmax over z, the gather).  The baseline's windows are canvas windows, not tile windows -- a different (the usual
    post-hoc) definition -- so the two agree except near tile seams, at canvas edges and where scores tie;
and compares them voxel by voxel.  Prints one JSON line (--json writes it to a file too)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from image_stitcher_amd import native, placement, synth  # noqa: E402

PEAK_GBS = 8000.0


def u16_to_i32(t):
    return t.view(torch.int16).to(torch.int32) & 0xFFFF


def box_sum(x, r):
    """(2r+1)^2 box sum of a [H, W] int32 tensor, reads clamped to its edges: separable, 2r + 1 shifted adds per axis."""
    if r == 0:
        return x.clone()
    p = torch.cat([x[:1].expand(r, -1), x, x[-1:].expand(r, -1)], 0)
    h = x.shape[0]
    col = p[0:h].clone()
    for d in range(1, 2 * r + 1):
        col += p[d:d + h]
    p = torch.cat([col[:, :1].expand(-1, r), col, col[:, -1:].expand(-1, r)], 1)
    w = x.shape[1]
    out = p[:, 0:w].clone()
    for d in range(1, 2 * r + 1):
        out += p[:, d:d + w]
    return out


def modified_laplacian(i):
    p = torch.cat([i[:, :1], i, i[:, -1:]], 1)
    ml = (2 * i - p[:, :-2] - p[:, 2:]).abs_()
    p = torch.cat([i[:1], i, i[-1:]], 0)
    return ml.add_((2 * i - p[:-2] - p[2:]).abs_())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--grid', type=int, default=16)
    ap.add_argument('--tile', type=int, default=2048)
    ap.add_argument('--ov', type=int, default=244)
    ap.add_argument('--nz', type=int, default=10)
    ap.add_argument('--radius', type=int, default=3)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--baseline-steps', type=int, default=2)
    ap.add_argument('--flags', type=int, default=0, help='sq_fuse_flags of the canvas stage (1 queues, 2 static walk)')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    g, T, Z, R = a.grid, a.tile, a.nz, a.radius
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
    zl = torch.arange(Z, dtype=torch.int32, device=dev)
    scratch = torch.empty(native.focus_scratch_bytes(g * g, T, T), dtype=torch.uint8, device=dev)
    out = torch.empty((hc, wc), dtype=torch.uint16, device=dev)
    key = torch.empty((hc, wc), dtype=torch.int64, device=dev)
    stack = native.empty_canvas(Z, hc, wc, torch.uint16, dev)
    base = torch.empty((hc, wc), dtype=torch.uint16, device=dev)
    base_z = torch.empty((hc, wc), dtype=torch.uint8, device=dev)

    def focus():
        native.fuse_project_focus(plan, tiles, out, key, zl, R, flats, scratch=scratch, flat_ptrs=flat_ptrs, flags=a.flags)

    def fuse_only():
        native.fuse_planes(plan, tiles, stack, flats, flat_ptrs=flat_ptrs)

    def torch_edf():      # on the fused stack: running best score (a strictly greater score wins: the lowest z on a tie)
        best = None
        for z in range(Z):
            f = box_sum(modified_laplacian(u16_to_i32(stack[z])), R)
            if best is None:
                best = f
                base_z.zero_()
            else:
                take = f > best
                best = torch.where(take, f, best)
                base_z.masked_fill_(take, z)
            del f
        torch.gather(stack.view(torch.int16), 0, base_z.long()[None], out=base.view(torch.int16)[None])

    for _ in range(a.warmup):
        focus()
    fuse_only(), torch_edf()
    torch.cuda.synchronize()
    times = {'focus': [], 'fuse': [], 'edf': []}
    for s in range(a.steps):      # alternating: they share the box's state
        plan_of = [('focus', focus)] + ([('fuse', fuse_only), ('edf', torch_edf)] if s < a.baseline_steps else [])
        for name, fn in plan_of:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            times[name].append((e0, e1))
    torch.cuda.synchronize()
    ms = {k: np.array([e0.elapsed_time(e1) for e0, e1 in v]) for k, v in times.items()}
    depth = native.depth_of_keys(key)
    covered = key != 0
    n_cov = int(covered.sum())
    same_depth = int(((depth == base_z.long()) & covered).sum())
    same_value = int(((out.view(torch.int16) == base.view(torch.int16)) & covered).sum())
    # the projection's output must be the fused stack's voxel at the depth it reports
    at_depth = torch.gather(stack.view(torch.int16), 0, depth.clamp(min=0)[None].to(torch.int64))[0]
    self_mismatch = int(((at_depth != out.view(torch.int16)) & covered).sum())
    cov = plan.covered_voxels
    px = g * g * T * T
    focus_bytes = Z * px * 2 + px * 5 + cov * (5 + 2 + 4) + hc * wc * (2 + 8)
    fuse_bytes = Z * (cov * 2 + hc * wc * 2)
    med = {k: float(np.median(v)) if len(v) else None for k, v in ms.items()}
    base_ms = med['fuse'] + med['edf'] if med['fuse'] is not None else None
    res = {
        'workload': f'{g}x{g} x {T}^2 uint16, {Z} z, float32 gains, R = {R} (one channel of config 3)', 'canvas': [hc, wc],
        'covered_voxels': int(cov), 'steps': a.steps, 'flags': a.flags,
        'focus_ms': med['focus'], 'focus_ms_min': float(ms['focus'].min()),
        'focus_algorithmic_gb': focus_bytes / 1e9, 'focus_gbs': focus_bytes / med['focus'] / 1e6,
        'focus_fraction_of_peak': focus_bytes / med['focus'] / 1e6 / PEAK_GBS,
        'baseline': 'sq_fuse_planes over the stack + torch EDF of the fused stack (canvas windows, int32)',
        'fuse_planes_ms': med['fuse'],
        'fuse_planes_fraction_of_peak': None if base_ms is None else fuse_bytes / med['fuse'] / 1e6 / PEAK_GBS,
        'torch_edf_ms': med['edf'], 'baseline_ms': base_ms,
        'speedup_vs_baseline': None if base_ms is None else base_ms / med['focus'],
        'output_is_stack_at_depth_mismatches': self_mismatch,
        'covered_canvas_voxels': n_cov, 'same_depth_as_baseline': same_depth / max(1, n_cov),
        'same_value_as_baseline': same_value / max(1, n_cov),
    }
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, 'w') as fh:
            fh.write(line + '\n')
    if self_mismatch:
        sys.exit(1)


if __name__ == '__main__':
    main()
