"""Timing of the point-cloud export (switch_nerf_amd/points.py).

    python scripts/points_export_timing.py [--image-rays 248832]

1. swn_points_pack on a 65536-ray x 256-sample batch (16.8 M points), RGBA records with the per-expert partition (E = 8), skip 1
   and skip 4: device time per call (hipEvent, median of 20) and the effective bandwidth over ~36 B read + 32 B written per kept
   point (the issue's 0.5 ms target at skip 1).
2. One render_image_points call (coarse points, skip 4) at 576 x 432 rays x (256 coarse + 512 fine) samples (val_scale_factor = 8
   image) against render_image_rays on the same rays: wall time of each, and the bytes written.
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import tempfile
import time
from argparse import Namespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def time_pack(R, S, skip, E, reps=20):
    from switch_nerf_amd import ops, points
    g = torch.Generator(device="cuda").manual_seed(1)
    pts = torch.randn(R, S, 3, device="cuda", generator=g)
    raw = torch.rand(R * S, 4, device="cuda", generator=g)
    alpha = torch.rand(R, S, device="cuda", generator=g)
    idx = torch.randint(0, E, (R * S,), device="cuda", generator=g, dtype=torch.int32)
    palette = torch.from_numpy(points.VOC_PALETTE[:E].copy()).cuda()
    rgb = raw[:, :3].view(R, S, 3)
    for _ in range(3):
        ops.points_pack(pts, alpha, ops.PLY_RGBA, skip, idx, E, rgb, None, palette)
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.points_pack(pts, alpha, ops.PLY_RGBA, skip, idx, E, rgb, None, palette)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    ms = sorted(times)[len(times) // 2]
    kept = R * ((S + skip - 1) // skip)
    moved = kept * (36 + 32)
    return dict(rays=R, samples=S, skip=skip, experts=E, points=kept, ms=round(ms, 4), tb_per_s=round(moved / ms / 1e9, 3))


def time_image(n_rays, S, F, batch):
    import synth
    from switch_nerf_amd.model import SwitchNeRF
    from switch_nerf_amd import points, rendering
    m = SwitchNeRF(synth.BUILDING, dtype=torch.bfloat16)
    m.load_state_dict(synth.make_weights(7, synth.BUILDING, gate_scale=0.02))
    m.eval()
    rays, img, _ = synth.make_rays(8, n_rays)
    rays, img = torch.from_numpy(rays).cuda(), torch.from_numpy(img).cuda()
    h = Namespace(coarse_samples=S, fine_samples=F, model_chunk_size=131072, perturb=0.0, use_sigma_noise=False, sigma_noise_std=1.0,
                  use_cascade=False, moe_return_gates=True, return_sigma=False, moe_expert_num=synth.BUILDING["num_experts"],
                  appearance_dim=48, image_pixel_batch_size=batch, render_test_points_typ=["coarse"],
                  render_test_points_sample_skip=4, return_pts_class_seg=False)
    with torch.no_grad():
        rendering.render_image_rays(m, None, rays[:batch], 0, h)          # warm-up (allocations)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rendering.render_image_rays(m, None, rays, 0, h)
        torch.cuda.synchronize()
        t_render = time.perf_counter() - t0
        with tempfile.TemporaryDirectory() as d:
            t0 = time.perf_counter()
            counts = points.render_image_points(m, None, rays, 0, h, d, 0)
            torch.cuda.synchronize()
            t_points = time.perf_counter() - t0
            nbytes = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))
    return dict(rays=n_rays, coarse=S, fine=F, pixel_batch=batch, render_image_rays_s=round(t_render, 3),
                render_image_points_s=round(t_points, 3), files=len(counts), points_written=int(sum(counts.values())),
                bytes_written=nbytes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--image-rays", type=int, default=576 * 432)
    ap.add_argument("--pixel-batch", type=int, default=8192)
    a = ap.parse_args()
    out = dict(pack=[time_pack(65536, 256, 1, 8), time_pack(65536, 256, 4, 8)])
    out["image"] = time_image(a.image_rays, 256, 512, a.pixel_batch)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
