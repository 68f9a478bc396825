"""Joint training of a Mega-NeRF in its three forms, the measurements of profiles/r22_mega_graph.md: the eager compact step (the default
path, cell_capacity=None), the eager padded step (cell_capacity = C) and the replayed padded step (graph.GraphedMegaStep, one capture).
The set-up of scripts/mega_train_timing.py: bf16, K = 8 cells of the DENSE configuration, centroids on the corners of a cube, hard
margin; 8192 x 256 and 1024 x 256 rays x samples.  Every variant draws its own jitter and sigma noise each step (the replay draws them
inside the graph), so all three do the same work.  C = the batch's largest cell count rounded up to 256 rows ("fit") and 1.25 x that
("slack"); a replay whose fresh jitter pushes a cell past C is reported as overflowed, not timed.

  steps      ms per step, host clock around `reps` steps ending in a device synchronise; one process, `--rounds` rounds with the order of
             the variants rotating; the median and the spread.  Library entry-point calls per step (counted by wrapping the C-ABI call)
             and kernels per step as torch.profiler sees them.  Padding: K C rows against the batch's P.
  kernels    swn_cells_pack_padded, swn_cells_gather_padded, swn_cells_blend and swn_cells_blend_bwd on the padded row space alone at
             P = 2 097 152: device events, median of 5 windows of 200 calls, against ALGORITHMIC bytes over the 8.0 TB/s HBM3E peak.

Every GPU step runs under its own time limit (an alarm whose default action ends the process: a step that hangs takes the script down
with it, and nothing is started after a failure).  Prints JSON lines.

    python scripts/bench_mega_graph.py [result.json] [--shapes 8192x256,1024x256] [--rounds 5] [--part steps|kernels|all]
"""
import argparse
import json
import os
import signal
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch

import synth
from mega_train_timing import count_calls, count_kernels, ev_time
from switch_nerf_amd import ops
from switch_nerf_amd.dense import DENSE, DenseNeRF
from switch_nerf_amd.graph import GraphedMegaStep
from switch_nerf_amd.mega import MegaNeRF

K = 8
HBM_PEAK = 8.0e12
CEN = np.array([[sx, sy, sz] for sx in (-0.4, 0.4) for sy in (-0.4, 0.4) for sz in (-0.4, 0.4)], np.float32)


class limit:
    """with limit(seconds): one GPU step under its own time limit - SIGALRM's default action ends the process."""

    def __init__(self, seconds):
        self.seconds = int(seconds)

    def __enter__(self):
        signal.signal(signal.SIGALRM, signal.SIG_DFL)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def up256(n):
    return -(-int(n) // 256) * 256


def steps(N, S, rounds):
    dev = "cuda"
    P = N * S
    rays, img, rgbs = (torch.from_numpy(a).to(dev) for a in synth.make_rays(5, N, DENSE["appearance_count"]))
    mega = MegaNeRF([DenseNeRF(DENSE, dtype=torch.bfloat16, seed=10 + i) for i in range(K)], CEN, 1.0, False, False, joint_training=True)

    def eager(cap):
        return lambda: mega.train_step(rgbs, rays, img, S, perturb=1.0, sigma_noise=torch.randn(P, device=dev), cell_capacity=cap)

    with limit(120):
        for _ in range(3):
            st = eager(None)()
        torch.cuda.synchronize()
    counts = st["ctx"]["counts"]
    fit, slack = up256(max(counts)), up256(1.25 * max(counts))
    rec = dict(rays=N, samples=S, points=P, members_per_cell=counts, C_fit=fit, C_slack=slack,
               padded_rows_over_points={"fit": K * fit / P, "slack": K * slack / P})
    variants = {"compact_eager": eager(None)}
    for tag, C in (("fit", fit), ("slack", slack)):
        with limit(120):
            g = GraphedMegaStep(mega, rgbs, rays, img, S, C, perturb=1.0, noise_std=1.0)
            torch.cuda.synchronize()
        variants[f"padded_eager_{tag}"] = eager(C)
        variants[f"graphed_{tag}"] = lambda g=g: g(rgbs, rays, img)
    names = list(variants)
    reps = 5 if P > 1 << 20 else 20
    times, overflowed = {k: [] for k in names}, {k: 0 for k in names}
    for rnd in range(rounds):
        for k in names[rnd % len(names):] + names[:rnd % len(names)]:
            with limit(120):
                try:
                    for _ in range(2):
                        variants[k]()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(reps):
                        variants[k]()
                    torch.cuda.synchronize()
                    times[k].append((time.perf_counter() - t0) / reps * 1e3)
                except RuntimeError as e:
                    if "did not fit" not in str(e):
                        raise
                    overflowed[k] += 1
    for k in names:
        t = times[k]
        rec[k] = dict(ms_median=float(np.median(t)) if t else None, ms_min=min(t) if t else None, ms_max=max(t) if t else None,
                      windows=len(t), overflowed_windows=overflowed[k])
        if t:
            with limit(120):
                try:
                    rec[k]["library_calls"] = sum(count_calls(variants[k]).values())
                    rec[k]["kernels_profiler"] = count_kernels(variants[k])
                except RuntimeError as e:
                    if "did not fit" not in str(e):
                        raise
    return rec


def kernels(P=2097152):
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.cat([torch.rand(P, 3, device=dev, generator=g) * 2 - 1, torch.zeros(P, 4, device=dev)], 1).contiguous()
    noise = torch.randn(P, device=dev, generator=g)
    d_out = torch.randn(P, 4, device=dev, generator=g)
    cen = torch.from_numpy(CEN).to(dev)
    out = {}
    for tag, margin in (("hard", 1.0), ("soft_1.15", 1.15)):
        hard = margin == 1
        with limit(120):
            w, counts = ops.cells_assign(x, cen, 0, margin)
            n = counts.tolist()
            C = up256(max(n))
            begin, rows, slot, _ = ops.cells_pack_padded(w, counts, C)
            sub = torch.randn(K * C, 4, device=dev, generator=g)
            real, total = sum(n), K * C
            cases = {
                "pack_padded": (lambda: ops.cells_pack_padded(w, counts, C), P * K * 4 + P * K * 4 + total * 4),
                "gather_padded": (lambda: ops.cells_gather_padded(x, rows, cen, C, 0, noise), total * 4 + real * 32 + total * 32),
                "blend": (lambda: ops.cells_blend(w, slot, begin, sub, hard), P * (K * 4 + (0 if hard else K * 4) + 16) + real * 16),
                "blend_bwd": (lambda: ops.cells_blend_bwd(w, rows, begin, d_out, total, hard), total * 4 + real * (16 + (0 if hard else 4)) + total * 16),
            }
            rec = dict(points=P, members=real, C=C, rows=total)
            for name, (fn, nbytes) in cases.items():
                us = ev_time(fn)
                rec[name] = dict(us=us, algorithmic_bytes=nbytes, bytes_per_s=nbytes / (us * 1e-6), hbm_fraction=nbytes / (us * 1e-6) / HBM_PEAK)
        out[tag] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("result", nargs="?")
    ap.add_argument("--shapes", default="8192x256,1024x256")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--part", default="all", choices=("steps", "kernels", "all"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mega_graph.py needs a GPU"
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, cells=K, dtype="bf16", cfg="DENSE")
    if args.part in ("steps", "all"):
        for shape in args.shapes.split(","):
            N, S = (int(v) for v in shape.split("x"))
            res[shape] = steps(N, S, args.rounds)
            print(json.dumps({shape: res[shape]}), flush=True)
    if args.part in ("kernels", "all"):
        res["kernels"] = kernels()
        print(json.dumps(dict(kernels=res["kernels"])), flush=True)
    if args.result:
        os.makedirs(os.path.dirname(os.path.abspath(args.result)), exist_ok=True)
        with open(args.result, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
