"""The two-network cascade's launches and step, the measurements of profiles/r19_cascade.md (bf16, 8192 rays).

  resample   swn_cascade_resample (draws + union, one launch) followed by swn_pe_from_z - the path forward_cascade takes - against the
             sequence it replaces - swn_sample_pdf, torch.sort(torch.cat), swn_pe_from_z - in ONE process, interleaved: device events, 7
             windows of 20 calls each after 3 warm-up calls; the median and the (max - min) spread over the windows of each, at
             (S, F) = (256, 256) and (256, 512).  Also each side without the encoding.
  step       Cascade.train_step at 8192 x (256 + 256) for the dense NeRF, and beside it - for scale, not a
             target: the cascade evaluates S + F points on the fine half against F - the single model's hierarchical train_step at the
             same (S, F).  Host clock around steps that end in a device synchronise; the median of 3 windows of 3 steps after 2 warm-up steps.

    python scripts/cascade_timing.py [result.json] [--only resample|step]

Run each --only part as its own process under its own time limit (timeout -k 10 <seconds> python scripts/cascade_timing.py ...).
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch

import synth
from switch_nerf_amd import ops
from switch_nerf_amd.cascade import Cascade
from switch_nerf_amd.dense import DENSE, DenseNeRF

N = 8192


def ev_windows(fns, iters=20, windows=7):
    """{name: [us per call, one per window]} with the candidates interleaved window by window."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            ts[k].append(a.elapsed_time(b) / iters * 1e3)
    return ts


def summary(v):
    return dict(median_us=float(np.median(v)), spread_us=float(max(v) - min(v)), windows=[round(x, 1) for x in v])


def resample(dev="cuda"):
    out = {}
    rays = torch.from_numpy(synth.make_rays(5, N)[0]).to(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    for S, F in ((256, 256), (256, 512)):
        z = torch.sort(torch.rand(N, S, device=dev, generator=g) * 0.95 + 0.05, 1)[0].contiguous()
        w = torch.rand(N, S, device=dev, generator=g) ** 4
        u = torch.rand(N, F, device=dev, generator=g)

        def sequence():
            zf = ops.sample_pdf(z, w, u, F)
            zu = torch.sort(torch.cat([z, zf], -1), -1)[0]
            return ops.pe_from_z(rays, zu, 12, torch.bfloat16, 128)

        def resample_then_pe():
            return ops.pe_from_z(rays, ops.cascade_resample(z, w, u, F)[0], 12, torch.bfloat16, 128)
        depths_sequence = lambda: torch.sort(torch.cat([z, ops.sample_pdf(z, w, u, F)], -1), -1)[0]
        depths_resample = lambda: ops.cascade_resample(z, w, u, F)[0]
        assert torch.equal(resample_then_pe().view(torch.int16), sequence().view(torch.int16))
        ts = ev_windows(dict(sequence=sequence, resample_then_pe=resample_then_pe, depths_sequence=depths_sequence,
                             depths_resample=depths_resample))
        out[f"{S}+{F}"] = {k: summary(v) for k, v in ts.items()}
        print(f"resample {S}+{F}: " + ", ".join(f"{k} {np.median(v):.1f} us (spread {max(v) - min(v):.1f})" for k, v in ts.items()), flush=True)
    return out


def window(step, n=3):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def step(S=256, F=256, dev="cuda"):
    rays, img, rgbs = (torch.from_numpy(a).to(dev) for a in synth.make_rays(5, N, 10))
    make = lambda s: DenseNeRF(dict(DENSE, appearance_count=10), dtype=torch.bfloat16, seed=s)
    cas, single = Cascade(make(1), make(2)), make(3)
    chunk = N * S
    run = dict(cascade=lambda: cas.train_step(rgbs, rays, img, S, chunk, 1.0, fine_samples=F),
               hierarchical=lambda: single.train_step(rgbs, rays, img, S, chunk, 1.0, fine_samples=F))
    out = {}
    for k, fn in run.items():
        for _ in range(2):
            fn()
        v = [window(fn) for _ in range(3)]
        out[k] = dict(median_ms=float(np.median(v)), windows=[round(x, 2) for x in v])
        print(f"step dense {N} x ({S} + {F}) {k}: {np.median(v):.2f} ms {out[k]['windows']}", flush=True)
    return out


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
    args = [a for a in args if a != only]
    res = {}
    if only in (None, "resample"):
        res["resample"] = resample()
    if only in (None, "step"):
        res["step_dense"] = step()
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        with open(args[0], "w") as f:
            json.dump(res, f, indent=1)
