"""Training a Mega-NeRF through its cells (switch_nerf_amd/mega.py, joint_training), the measurements of profiles/r16_mega_train.md:
8192 rays x 256 samples, bf16, K = 8 cells of the DENSE configuration (centroids on the corners of a cube: balanced cells), hard
margin (what --train_mega_nerf builds), perturbation and sigma noise supplied.

  ms per step     MegaNeRF.train_step against ONE DenseNeRF.train_step on the same batch - the same total rows through one model, the
                  baseline.  Host clock around steps that end in a device synchronise; the two alternate, window by window; each figure
                  is the median of 5 windows of 5 steps after 3 warm-up steps each (the spread is printed).
  launches        library entry-point calls per step (each is one to three kernel launches; counted by wrapping the C-ABI call), and
                  the kernels per step as torch.profiler sees them (torch's own copies / cats included) where the profiler is available.
  blend backward  swn_cells_blend_bwd alone at the step's row count, hard and soft (1.15): device events, median of 5 windows of 200
                  calls; achieved bandwidth on ALGORITHMIC bytes per packed row (16 B read + 4 B index + 4 B weight when soft, 16 B
                  written) over the 8.0 TB/s HBM3E peak.

    python scripts/mega_train_timing.py [result.json] [--rays N] [--samples S]
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
from switch_nerf_amd.dense import DENSE, DenseNeRF
from switch_nerf_amd.mega import MegaNeRF

K = 8
HBM_PEAK = 8.0e12


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def window(step, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def ev_time(fn, iters=200, windows=5):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / iters * 1e3)
    return float(np.median(ts))             # microseconds per call


def count_calls(step):
    """Library entry-point calls of one step, by name."""
    seen = {}
    real = ops.call

    def counting(name, *a):
        seen[name] = seen.get(name, 0) + 1
        return real(name, *a)
    ops.call = counting
    try:
        step()
        torch.cuda.synchronize()
    finally:
        ops.call = real
    return seen


def count_kernels(step):
    """Kernels of one step as torch.profiler records them, or None where it is not available."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        n = sum(e.count for e in prof.key_averages() if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower())
        return int(n) or None
    except Exception as e:      # noqa: BLE001  (a measurement that could not be taken is reported as such, not guessed)
        print(f"torch.profiler not available here: {e!r}", flush=True)
        return None


def main():
    N, S = arg("--rays", 8192), arg("--samples", 256)
    out_path = next((a for a in sys.argv[1:] if a.endswith(".json")), None)
    dev = "cuda"
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, rays=N, samples=S, cells=K, dtype="bf16", cfg="DENSE")
    rays, img, rgbs = synth.make_rays(5, N, DENSE["appearance_count"])
    rays, img, rgbs = (torch.from_numpy(a).to(dev) for a in (rays, img, rgbs))
    g = torch.Generator(device=dev).manual_seed(1)
    pr = torch.rand(N, S, device=dev, generator=g)
    noise = torch.randn(N * S, device=dev, generator=g)
    cen = np.array([[sx, sy, sz] for sx in (-0.4, 0.4) for sy in (-0.4, 0.4) for sz in (-0.4, 0.4)], np.float32)
    mega = MegaNeRF([DenseNeRF(DENSE, dtype=torch.bfloat16, seed=10 + i) for i in range(K)], cen, 1.0, False, False, joint_training=True)
    dense = DenseNeRF(DENSE, dtype=torch.bfloat16, seed=10)

    def step_mega():
        return mega.train_step(rgbs, rays, img, S, perturb=1.0, perturb_rand=pr, sigma_noise=noise)

    def step_dense():
        return dense.train_step(rgbs, rays, img, S, N * S, perturb=1.0, perturb_rand=pr, sigma_noise=noise)

    for _ in range(3):
        st = step_mega()
        step_dense()
    res["members_per_cell"] = st["ctx"]["counts"]
    ms = dict(mega=[], dense=[])
    for _ in range(5):                       # alternating windows
        ms["mega"].append(window(step_mega, 5))
        ms["dense"].append(window(step_dense, 5))
    res["ms_per_step"] = {k: dict(median=float(np.median(v)), min=min(v), max=max(v)) for k, v in ms.items()}
    res["mega_over_dense"] = res["ms_per_step"]["mega"]["median"] / res["ms_per_step"]["dense"]["median"]
    print(json.dumps(dict(members_per_cell=res["members_per_cell"], ms_per_step=res["ms_per_step"], mega_over_dense=res["mega_over_dense"])), flush=True)
    calls = dict(mega=count_calls(step_mega), dense=count_calls(step_dense))
    res["library_calls_per_step"] = {k: sum(v.values()) for k, v in calls.items()}
    res["library_calls_by_name"] = calls
    res["kernels_per_step_profiler"] = dict(mega=count_kernels(step_mega), dense=count_kernels(step_dense))
    print(json.dumps(dict(library_calls_per_step=res["library_calls_per_step"], kernels_per_step_profiler=res["kernels_per_step_profiler"])), flush=True)
    # the blend's backward alone, at the step's row count
    P = N * S
    x = torch.cat([rays[:, None, :3] + rays[:, None, 3:6] * torch.rand(N, S, 1, device=dev, generator=g), torch.zeros(N, S, 4, device=dev)], -1).view(P, 7)
    d_out = torch.randn(P, 4, device=dev, generator=g)
    res["blend_bwd"] = {}
    for tag, margin in (("hard", 1.0), ("soft_1.15", 1.15)):
        w, counts = ops.cells_assign(x, torch.from_numpy(cen).to(dev), 0, margin)
        begin, rows, slot = ops.cells_pack(w, counts)
        total, hard = int(counts.sum().item()), margin == 1
        us = ev_time(lambda: ops.cells_blend_bwd(w, rows, begin, d_out, total, hard))
        nbytes = total * (16 + 4 + (0 if hard else 4) + 16)
        res["blend_bwd"][tag] = dict(rows=total, us=us, algorithmic_bytes=nbytes, bytes_per_s=nbytes / (us * 1e-6),
                                     hbm_fraction=nbytes / (us * 1e-6) / HBM_PEAK)
    print(json.dumps(dict(blend_bwd=res["blend_bwd"])), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
