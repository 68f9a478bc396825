"""Errors and timings of the ray generation (switch_nerf_amd/rays.py, csrc/raygen.hip) for profiles/r24_raygen.md.

    python scripts/bench_raygen.py [--out FILE]

Needs a GPU (no fallback).  One process; prints markdown and, with --out, writes it to FILE as well.
  1. the device's error against the fp64 restatement (tests/raygen_restate.py) on the fixture's cases, next to the reference's own;
  2. the rays of one 65 536-pixel batch of a 1152 x 1536 validation image and of one 8192-ray training gather: the fused launch against
     what a user of the library had to write before it - ray_utils restated in framework ops on the device (directions of the whole
     image once per image, then per batch a slice, the rotation, the planes and a copy_ into a static buffer); medians of 5 windows of
     200 calls after a warm-up, device events, both paths alternating in the same process;
  3. one whole render_image at the benchmark model's shape (SwitchNeRF of synth.BUILDING, bf16, 64 coarse samples, batches of 8192
     pixels of a 256 x 192 image) with and without graph_eval, against the hand-written loop over framework-op rays.
"""
import argparse
import os
import sys
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import raygen_restate as restate  # noqa: E402
import synth  # noqa: E402
from switch_nerf_amd import rays, rendering  # noqa: E402

WINDOWS, CALLS = 5, 200
NEAR, FAR, ALT = 0.05, 1.5, [-0.3, 0.45]


def torch_directions(W, H, fx, fy, cx, cy, center, dev):
    i, j = torch.meshgrid(torch.arange(W, dtype=torch.float32, device=dev), torch.arange(H, dtype=torch.float32, device=dev), indexing="xy")
    if center:
        i, j = i + 0.5, j + 0.5
    d = torch.stack([(i - cx) / fx, -(j - cy) / fy, -torch.ones_like(i)], -1)
    return d / torch.linalg.norm(d, dim=-1, keepdim=True)


def torch_plane(o, d, alt, bound):
    """The plane truncation without a data-dependent shape (a boolean-mask index is a host read): computed for every ray, selected."""
    hit = (o[..., 0] < alt) & (d[..., 0] > 0)
    w = o - torch.tensor([alt, 0.0, 0.0], device=o.device)
    si = w[..., :1] / -d[..., :1]
    p = w + si * d + torch.tensor([alt, 0.0, 0.0], device=o.device)
    return torch.where(hit[..., None], (o - p).norm(dim=-1, keepdim=True), bound)


def torch_rays(dirs, c2w, near, far, alt):
    """get_rays in framework ops: dirs [n, 3], c2w [3, 4] or [n, 3, 4] on the device -> [n, 8]."""
    if c2w.dim() == 2:
        d = dirs @ c2w[:, :3].T
        o = c2w[:, 3].expand(d.shape)
    else:
        d = torch.bmm(c2w[:, :, :3], dirs[:, :, None])[:, :, 0]
        o = c2w[:, :, 3]
    d = d / torch.norm(d, dim=-1, keepdim=True)
    nb, fb = near * torch.ones_like(o[..., :1]), far * torch.ones_like(o[..., :1])
    if alt is not None:
        nb = torch.clamp(torch_plane(o, d, alt[0], nb), min=near)
        fb = torch.clamp(torch_plane(o, d, alt[1], fb), max=far)
        fb = torch.maximum(nb, fb)
    return torch.cat([o, d, nb, fb], -1)


def timed(fn):
    """Median over WINDOWS windows of CALLS calls, microseconds per call, and (min, max)."""
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        torch.cuda.synchronize()
        per.append(a.elapsed_time(b) * 1e3 / CALLS)
    return float(np.median(per)), min(per), max(per)


def timed_pair(fa, fb):
    """Two paths alternating window by window."""
    ra, rb = [], []
    for _ in range(2):
        ra.append(timed(fa))
        rb.append(timed(fb))
    best = lambda r: (float(np.median([x[0] for x in r])), min(x[1] for x in r), max(x[2] for x in r))
    return best(ra), best(rb)


def look(origin, forward):
    f = np.asarray(forward, np.float64)
    f = f / np.linalg.norm(f)
    r = np.cross(f, np.array([-1.0, 0.0, 0.0]))
    r = r / np.linalg.norm(r)
    return torch.from_numpy(np.concatenate([np.stack([r, np.cross(r, f), -f], 1), np.asarray(origin, np.float64)[:, None]], 1)).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_raygen.py needs a GPU"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    # 1. errors on the fixture
    g = np.load(os.path.join(ROOT, "tests", "golden", "raygen.npz"))
    W, H = int(g["W"]), int(g["H"])
    say("## Error against the fp64 restatement (37 x 29 fixture)\n")
    say("| case | reference dir | device dir | reference near | device near | reference far | device far |")
    say("|---|---|---|---|---|---|---|")
    worst = dict(dir=0.0, near=0.0, far=0.0)
    for name in restate.CASES:
        (want, _, _), alt = restate.want_case(g, name)
        cam = rays.Camera(W, H, g["intrinsics"].tolist(), torch.from_numpy(g[f"{name}_c2w"]))
        got = rays.camera_rays(cam, float(g[f"{name}_near"]), float(g[f"{name}_far"]), None if alt is None else alt.tolist(),
                               bool(g[f"{name}_center"])).view(H, W, 8).cpu().numpy()
        e, r = restate.errors(got, want), restate.errors(g[f"{name}_rays"], want)
        for k in worst:
            worst[k] = max(worst[k], e[k])
        say(f"| {name} | {r['dir']:.3e} | {e['dir']:.3e} | {r['near']:.3e} | {e['near']:.3e} | {r['far']:.3e} | {e['far']:.3e} |")
    say(f"\nMaxima: reference dir {float(g['ref_err_dir']):.3e} near {float(g['ref_err_near']):.3e} far {float(g['ref_err_far']):.3e}; "
        f"device dir {worst['dir']:.3e} near {worst['near']:.3e} far {worst['far']:.3e}; the tests' bound is 4 x the reference's.\n")

    # 2. the rays of one batch, and of one training gather
    W, H, B = 1536, 1152, 65536
    K = [1400.0, 1410.0, 760.5, 580.25]
    cam = rays.Camera(W, H, K, look([-0.6, 0.02, 0.03], [1.0, 0.2, -0.3]), 3)
    c2w = cam.c2w.cuda()
    dirs = torch_directions(W, H, *K, True, "cuda").view(-1, 3)
    static = torch.empty(B, 8, device="cuda")
    begin = 5 * B

    def framework_batch():
        static.copy_(torch_rays(dirs[begin:begin + B], c2w, NEAR, FAR, ALT))

    def fused_batch():
        rays.camera_rays(cam, NEAR, FAR, ALT, True, begin, B, out=static)

    framework_batch()
    ref = static.clone()
    fused_batch()
    say("## One 65 536-pixel batch of a 1536 x 1152 image, into a static buffer\n")
    say(f"max |fused - framework ops| over the batch: {float((static - ref).abs().max()):.3e}\n")
    (fa, fb) = timed_pair(framework_batch, fused_batch)
    say("| path | median us | min | max |")
    say("|---|---|---|---|")
    say(f"| framework ops (slice, matmul, norm, planes, cat, copy_) | {fa[0]:.1f} | {fa[1]:.1f} | {fa[2]:.1f} |")
    say(f"| camera_rays(out=) - one launch | {fb[0]:.1f} | {fb[1]:.1f} | {fb[2]:.1f} |")
    say(f"\nThe launch writes {B * 32 / 1e6:.1f} MB: {B * 32 / 8e12 * 1e6:.2f} us at the 8 TB/s HBM peak.\n")

    N, M = 8192, 64
    cams = [rays.Camera(W, H, K, look([-0.6, 0.01 * k, 0.03], [1.0, 0.2 - 0.005 * k, -0.3]), k) for k in range(M)]
    table = rays.camera_table(cams)
    rng = np.random.default_rng(0)
    ci = torch.from_numpy(rng.integers(0, M, N)).cuda()
    pi = torch.from_numpy(rng.integers(0, W * H, N)).cuda()
    poses = table[:, :12].view(M, 3, 4)

    def framework_gather():
        static[:N].copy_(torch_rays(dirs[pi], poses[ci], NEAR, FAR, ALT))

    def fused_gather():
        rays.pixel_rays(table, ci, pi, W, H, NEAR, FAR, ALT, True, out=static[:N])

    framework_gather()
    ref = static[:N].clone()
    fused_gather()
    say("## One 8192-ray training gather (64 cameras, int64 indices)\n")
    say(f"max |fused - framework ops|: {float((static[:N] - ref).abs().max()):.3e}\n")
    (fa, fb) = timed_pair(framework_gather, fused_gather)
    say("| path | median us | min | max |")
    say("|---|---|---|---|")
    say(f"| framework ops (two gathers, bmm, norm, planes, cat, copy_) | {fa[0]:.1f} | {fa[1]:.1f} | {fa[2]:.1f} |")
    say(f"| pixel_rays(out=) - one launch | {fb[0]:.1f} | {fb[1]:.1f} | {fb[2]:.1f} |\n")

    # 3. a whole render_image
    from switch_nerf_amd.model import SwitchNeRF
    W, H = 256, 192
    cam = rays.Camera(W, H, [280.0, 282.0, 127.5, 97.25], look([-0.6, 0.02, 0.03], [1.0, 0.2, -0.3]), 3)
    c2w = cam.c2w.cuda()
    hp = Namespace(coarse_samples=64, fine_samples=0, model_chunk_size=8192 * 64, perturb=1.0, use_sigma_noise=True, sigma_noise_std=1.0,
                   image_pixel_batch_size=8192, appearance_dim=48, center_pixels=True)
    m = SwitchNeRF(synth.BUILDING, dtype=torch.bfloat16)
    m.load_state_dict(synth.make_weights(41, synth.BUILDING))
    m.eval()
    P = W * H

    def by_hand():
        d = torch_directions(W, H, 280.0, 282.0, 127.5, 97.25, True, "cuda").view(-1, 3)
        r = torch_rays(d, c2w, NEAR, FAR, ALT)
        idx = torch.full((P,), cam.image_index, dtype=torch.long, device="cuda")
        out = {}
        for b in range(0, P, hp.image_pixel_batch_size):
            res, _ = rendering.render_rays(m, None, r[b:b + 8192].contiguous(), idx[b:b + 8192].contiguous(), hp, None, None, True, False, True)
            for k, v in res.items():
                out.setdefault(k, []).append(v)
        return {k: torch.stack(v) if v[0].dim() == 0 else torch.cat(v) for k, v in out.items()}

    def image():
        return rendering.render_image(m, None, cam, hp, NEAR, FAR, ALT)

    say(f"## One render_image, {W} x {H}, SwitchNeRF (synth.BUILDING, bf16), 64 samples, {P // 8192} batches of 8192 pixels\n")
    say("| graph_eval | path | median ms | min | max |")
    say("|---|---|---|---|---|")
    global CALLS
    CALLS = 10
    for ge in (False, True):
        m.graph_eval = ge
        (fa, fb) = timed_pair(by_hand, image)
        say(f"| {ge} | framework-op rays, sliced, render_rays per batch, cat | {fa[0] / 1e3:.3f} | {fa[1] / 1e3:.3f} | {fa[2] / 1e3:.3f} |")
        say(f"| {ge} | render_image | {fb[0] / 1e3:.3f} | {fb[1] / 1e3:.3f} | {fb[2] / 1e3:.3f} |")


if __name__ == "__main__":
    main()
