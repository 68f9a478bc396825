"""Error tables and timings of the image metrics (switch_nerf_amd/metrics.py, csrc/ssim.hip) for profiles/r23_metrics.md.

    python scripts/bench_metrics.py [--out FILE] [--no-torch]

Needs a GPU (no fallback).  One process; prints markdown and, with --out, appends every section to FILE as soon as it is measured.
  1. the reference's own error: its fp32 CPU floats and map (tests/golden/metrics.npz) against the fp64 restatement
     (tests/metrics_restate.py), per case - the figures the test bounds are derived from;
  2. the kernel's error against the same restatement on the same cases, and at the validation-image size against the formula in fp64
     torch ops on the GPU;
  3. timings at 1152 x 1536 x 3 (a Mega-NeRF validation image at val_scale_factor 4) and 256 x 256 x 3: device events, the median of 5
     windows of 200 calls after a warm-up, of (a) the fused pair of launches (ops.ssim_fwd), (b) image_metrics around it, (c) the same
     formula in torch ops on the same GPU - what a user has without this module -, next to (d) the time the bytes the operation must
     move (both images once, four floats out) take at the 8 TB/s HBM peak.
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import metrics_restate as restate  # noqa: E402
from switch_nerf_amd import metrics, ops  # noqa: E402

HBM_PEAK = 8.0e12
WINDOWS, CALLS = 5, 200


def torch_formula(x, y, taps, dtype=torch.float32):
    """The metric in torch ops on x, y [A, B, C]: ten grouped convolutions and the elementwise formula -> (ssim, mse) 0-dim tensors."""
    C = x.shape[-1]
    w, hw = taps.to(x.device, dtype), taps.numel() // 2
    wb, wa = w.view(1, 1, 1, -1).repeat(C, 1, 1, 1), w.view(1, 1, -1, 1).repeat(C, 1, 1, 1)
    blur = lambda z: F.conv2d(F.conv2d(z, wb, padding=[0, hw], groups=C), wa, padding=[hw, 0], groups=C)
    x, y = x.to(dtype).permute(2, 0, 1)[None], y.to(dtype).permute(2, 0, 1)[None]
    mu0, mu1 = blur(x), blur(y)
    s00 = torch.clamp(blur(x * x) - mu0 * mu0, min=0.0)
    s11 = torch.clamp(blur(y * y) - mu1 * mu1, min=0.0)
    r = blur(x * y) - mu0 * mu1
    s01 = torch.sign(r) * torch.min(torch.sqrt(s00 * s11), torch.abs(r))
    m = (2 * mu0 * mu1 + 1e-4) * (2 * s01 + 9e-4) / ((mu0 * mu0 + mu1 * mu1 + 1e-4) * (s00 + s11 + 9e-4))
    return m.mean(), ((x - y) ** 2).mean()


def timed(fn):
    """Median over WINDOWS windows of CALLS calls, in microseconds per call, and the spread (min, max)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch-ops baseline")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_metrics.py needs a GPU"

    def emit(text):
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")

    g = np.load(os.path.join(ROOT, "tests", "golden", "metrics.npz"))
    emit("### Error against the fp64 restatement, per golden case\n")
    emit("| case | shape | filter | reference scalar | reference map | kernel scalar | kernel map |")
    emit("|---|---|---|---|---|---|---|")
    worst = {"rs": 0.0, "rm": 0.0, "ks": 0.0, "km": 0.0}
    for name in map(str, g["cases"]):
        base = str(g[f"{name}_of"]) if f"{name}_of" in g.files else name
        x, y, fs = g[f"{base}_pred"], g[f"{base}_target"], int(g[f"{name}_fs"])
        mask = g[f"{name}_mask"] if base != name else None
        want = restate.metrics(x, y, g[f"taps_{fs}"], mask=mask)
        p, t = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        raw = torch.empty(1, 4, device="cuda")
        res = metrics.image_metrics(p, t, valid_mask=None if mask is None else torch.from_numpy(mask).cuda(), out=raw, want_map=True,
                                    filter_size=fs)
        raw = raw.cpu().double().numpy()[0]
        err = lambda a, b: 0.0 if (a != a and b != b) else abs(a - b)
        if mask is None:
            rs = max(err(float(g[f"{name}_ssim"]), want["ssim"]), err(float(g[f"{name}_mse"]), want["mse"]))
            rm = float(np.abs(g[f"{name}_map"].astype(np.float64) - want["map"]).max())
            ks = max(err(raw[0], want["ssim"]), err(raw[1], want["mse"]))
            km = float(np.abs(res["ssim_map"][0].cpu().double().numpy() - want["map"]).max())
            worst["rm"], worst["km"] = max(worst["rm"], rm), max(worst["km"], km)
            rm, km = f"{rm:.3e}", f"{km:.3e}"
        else:
            rs = max(err(float(g[f"{name}_ssim_mask"]), want["ssim_mask"]), err(float(g[f"{name}_mse_mask"]), want["mse_mask"]))
            ks = max(err(raw[2], want["ssim_mask"]), err(raw[3], want["mse_mask"]))
            rm = km = "(of tails)"
        worst["rs"], worst["ks"] = max(worst["rs"], rs), max(worst["ks"], ks)
        emit(f"| {name} | {'x'.join(map(str, x.shape))} | {fs} | {rs:.3e} | {rm} | {ks:.3e} | {km} |")
    emit(f"| **largest** | | | {worst['rs']:.3e} | {worst['rm']:.3e} | {worst['ks']:.3e} | {worst['km']:.3e} |")
    emit(f"\nBounds (4 x the reference's largest, rounded up, + 2^-23): scalar {restate.BOUND_SCALAR:.3e}, map {restate.BOUND_MAP:.3e}.\n")

    gen = torch.Generator(device="cuda").manual_seed(23)
    taps = metrics._taps(11, 1.5)
    emit("### Timings and the error at the sizes timed\n")
    emit("| shape | tiles | fused pair (us) | min..max | image_metrics (us) | torch ops fp32 (us) | bytes | at 8 TB/s (us) | fused / HBM bound "
         "| ssim err vs fp64 torch | mse err vs fp64 torch |")
    emit("|---|---|---|---|---|---|---|---|---|---|---|")
    for A, B in ((1152, 1536), (256, 256)):
        smooth = lambda z: F.avg_pool2d(z.permute(2, 0, 1)[None], 3, stride=1, padding=1)[0].permute(1, 2, 0).contiguous()
        x = smooth(torch.rand(A, B, 3, device="cuda", generator=gen))
        y = (x + 0.25 * (smooth(torch.rand(A, B, 3, device="cuda", generator=gen)) - 0.5)).clamp(0, 1)
        out = torch.empty(1, 4, device="cuda")
        fused = timed(lambda: ops.ssim_fwd(x[None], y[None], taps, 1e-4, 9e-4, out=out))
        whole = timed(lambda: metrics.image_metrics(x, y, out=out))
        s64, m64 = torch_formula(x, y, taps, torch.float64)
        torch.cuda.synchronize()
        e_ssim, e_mse = abs(out[0, 0].item() - s64.item()), abs(out[0, 1].item() - m64.item())
        base = "not measured" if args.no_torch else f"{timed(lambda: torch_formula(x, y, taps))[0]:.1f}"
        nbytes = 2 * x.numel() * 4 + 16
        tiles = -(-A // metrics.TILE) * -(-B // metrics.TILE)
        emit(f"| {A}x{B}x3 | {tiles} | {fused[0]:.1f} | {fused[1]:.1f}..{fused[2]:.1f} | {whole[0]:.1f} | {base} | {nbytes} | "
             f"{nbytes / HBM_PEAK * 1e6:.2f} | {fused[0] / (nbytes / HBM_PEAK * 1e6):.1f}x | {e_ssim:.3e} | {e_mse:.3e} |")


if __name__ == "__main__":
    main()
