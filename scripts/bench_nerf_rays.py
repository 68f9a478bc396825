"""Time the NeRF-dataset ray kernels (switch_nerf_amd/nerf_rays.py) beside the same arithmetic written as eager torch ops on the device,
in one run: one 800 x 800 image's rays per mode (raw, normalized, ndc, bungee sphere, bungee flat) and an 8192-pixel gather.

    python scripts/bench_nerf_rays.py [--iters 200] [--warmup 20]

Each figure is the median of `iters` event-timed calls after `warmup` untimed ones, in microseconds; the eager forms follow the
reference's statements (ray_utils.get_rays / ndc_rays, load_bungee.get_bungee_nearfar_radii) with tensors that already live on the GPU.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from switch_nerf_amd import nerf_rays as nr  # noqa: E402

W = H = 800
SCALE, ORIGIN = 2e-4, [30.0, -20.0, -6371011.0]
NEAR, FAR = 2.0, 6.0


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def eager_get_rays(K, c2w):
    i, j = torch.meshgrid(torch.linspace(0, W - 1, W, device=c2w.device), torch.linspace(0, H - 1, H, device=c2w.device), indexing="ij")
    i, j = i.t(), j.t()
    dirs = torch.stack([(i - K[0][2]) / K[0][0], -(j - K[1][2]) / K[1][1], -torch.ones_like(i)], -1)
    rays_d = torch.sum(dirs[..., None, :] * c2w[:3, :3], -1)
    return c2w[:3, -1].expand(rays_d.shape), rays_d


def eager_ndc(focal, near, o, d):
    t = -(near + o[..., 2]) / d[..., 2]
    o = o + t[..., None] * d
    o0 = -1. / (W / (2. * focal)) * o[..., 0] / o[..., 2]
    o1 = -1. / (H / (2. * focal)) * o[..., 1] / o[..., 2]
    o2 = 1. + 2. * near / o[..., 2]
    d0 = -1. / (W / (2. * focal)) * (d[..., 0] / d[..., 2] - o[..., 0] / o[..., 2])
    d1 = -1. / (H / (2. * focal)) * (d[..., 1] / d[..., 2] - o[..., 1] / o[..., 2])
    d2 = -2. * near / o[..., 2]
    return torch.stack([o0, o1, o2], -1), torch.stack([d0, d1, d2], -1)


def eager_mode(K, c2w, mode, focal):
    o, d = eager_get_rays(K, c2w)
    if mode == "normalized":
        d = d / torch.norm(d, dim=-1, keepdim=True)
    elif mode == "ndc":
        o, d = eager_ndc(focal, 1.0, o, d)
    return torch.cat([o, d, NEAR * torch.ones_like(d[..., :1]), FAR * torch.ones_like(d[..., :1])], -1).view(-1, 8)


def eager_bungee(K, c2w, kind, globe):
    o, d = eager_get_rays(K, c2w)
    d = d / torch.norm(d, dim=-1, keepdim=True)
    if kind == "sphere":
        oc = o - globe
        b = 2 * torch.sum(oc * d, dim=-1)
        n2 = torch.norm(d, dim=-1) ** 2
        c2 = torch.norm(oc, dim=-1) ** 2
        nf = []
        for radius, k in (((6371011 + 250) * SCALE, 0.9), (6371011 * SCALE, 1.1)):
            delta = b ** 2 - 4 * n2 * (c2 - radius ** 2)
            dist = (-b - delta ** 0.5) / (2 * n2)
            nf.append(torch.norm(o - (o + dist[..., None] * d), dim=-1, keepdim=True) * k)
        near, far = nf
    else:
        normal = torch.tensor([0, 0, 1]).to(o) * SCALE
        p_far = torch.tensor([0, 0, 0]).to(o) * SCALE
        p_near = torch.tensor([0, 0, 250]).to(o) * SCALE
        near = ((p_near - o * normal).sum(-1) / (d * normal).sum(-1)).clamp(min=1e-6).unsqueeze(-1)
        far = ((p_far - o * normal).sum(-1) / (d * normal).sum(-1)).unsqueeze(-1)
    dx = torch.sqrt(torch.sum((d[:-1] - d[1:]) ** 2, -1))
    dx = torch.cat([dx, dx[-2:-1]], 0)
    return torch.cat([o, d, near, far], -1).view(-1, 8), (dx[..., None] * 2 / np.sqrt(12)).view(-1, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    K = torch.tensor([[1111.0, 0, 400.5], [0, 1109.0, 399.25], [0, 0, 1]])
    c2w = torch.tensor([[0.68, 0.70, -0.19, 0.1], [-0.72, 0.68, -0.10, -0.2], [0.06, 0.21, 0.97, 0.5]])
    cam = nr.PinholeCamera(W, H, K, c2w)
    Kd, pose = K.cuda(), c2w.cuda()
    globe = torch.tensor(np.array(ORIGIN) * SCALE).float().cuda()
    out, rad = torch.empty(W * H, 8, device="cuda"), torch.empty(W * H, 1, device="cuda")
    res = {}
    for mode in ("raw", "normalized", "ndc"):
        res[f"image_{mode}_kernel_us"] = timed(lambda: nr.camera_rays(cam, mode, NEAR, FAR, focal=1111.0, out=out), a.iters, a.warmup)
        res[f"image_{mode}_eager_us"] = timed(lambda: eager_mode(Kd, pose, mode, 1111.0), a.iters, a.warmup)
    for kind in ("sphere", "flat"):
        res[f"image_{kind}_kernel_us"] = timed(lambda: nr.bungee_rays(cam, SCALE, ORIGIN, kind, out=out, radii_out=rad), a.iters, a.warmup)
        res[f"image_{kind}_eager_us"] = timed(lambda: eager_bungee(Kd, pose, kind, globe), a.iters, a.warmup)
    # the 8192-pixel gather of a training batch from 64 cameras; eager: index the precomputed [M, H * W, 8] rays the loader keeps
    M, N = 64, 8192
    table = nr.camera_table([cam] * M)
    gen = torch.Generator(device="cuda").manual_seed(3)
    ci = torch.randint(0, M, (N,), device="cuda", generator=gen)
    pi = torch.randint(0, W * H, (N,), device="cuda", generator=gen)
    g_out, g_rad = torch.empty(N, 8, device="cuda"), torch.empty(N, 1, device="cuda")
    res["gather_normalized_kernel_us"] = timed(lambda: nr.pixel_rays(table, ci, pi, W, H, "normalized", NEAR, FAR, out=g_out), a.iters, a.warmup)
    res["gather_sphere_kernel_us"] = timed(lambda: nr.pixel_rays(table, ci, pi, W, H, "sphere", scene_scaling_factor=SCALE, scene_origin=ORIGIN,
                                                                 out=g_out, radii_out=g_rad), a.iters, a.warmup)
    stored = eager_mode(Kd, pose, "normalized", 1111.0).unsqueeze(0).expand(M, -1, -1).contiguous()          # 64 x 640000 x 8 fp32: 1.3 GB
    res["gather_stored_rays_index_us"] = timed(lambda: stored[ci, pi], a.iters, a.warmup)
    res["stored_rays_bytes"] = stored.numel() * 4
    res["table_bytes"] = table.numel() * 4
    print(json.dumps({k: round(v, 2) if isinstance(v, float) else v for k, v in res.items()}))


if __name__ == "__main__":
    main()
