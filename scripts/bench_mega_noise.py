"""The in-place sigma-noise draw of the Mega-NeRF cells against the gathered read it replaces, the measurements of
profiles/r25_mega_device_noise.md.

  kernels   swn_cells_gather_rng / swn_cells_gather_padded_rng against swn_rng_fill + swn_cells_gather / _padded (the same values through
            a [P] tensor) and against the plain gather without noise: device events, median of 5 windows of 200 calls (the helper of
            scripts/mega_train_timing.py), at the row counts of tests/golden/mega_train.npz (2048 points, 3 cells) and at 2 097 152
            points over 8 cells.
  step      the fixture's joint step (64 rays x 32 + 16 fine, fp32, three cells; compact and padded at (768, 384)) with the noise drawn
            by the step (MegaNeRF.set_device_noise) against the same step handed rng_fill's tensors each time (what a caller of the
            supplied-noise arguments pays): host clock around 20 steps ending in a device synchronise, median of 5 windows.

Every GPU part runs under its own time limit (an alarm whose default action ends the process).  Prints JSON lines.

    python scripts/bench_mega_noise.py [result.json]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]
import numpy as np
import torch

from bench_mega_graph import limit, up256
from mega_train_timing import ev_time
from switch_nerf_amd import ops

SEED = 0x5EEDC0FFEE12345F


def kernels(P, K, R=32):
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.cat([torch.rand(P, 3, device=dev, generator=g) * 2 - 1, torch.zeros(P, 4, device=dev)], 1).contiguous()
    cen = (torch.rand(K, 3, device=dev, generator=g) * 1.2 - 0.6).contiguous()
    step = ops.rng_step_tensor(1, dev)
    out = {}
    for tag, margin in (("hard", 1.0), ("soft_1.15", 1.15)):
        w, counts = ops.cells_assign(x, cen, 0, margin)
        n = counts.tolist()
        total, C = sum(n), up256(max(n))
        _, rows, _ = ops.cells_pack(w, counts)
        _, prow, _, _ = ops.cells_pack_padded(w, counts, C)
        buf = torch.empty(P, dtype=torch.float32, device=dev)
        fill = lambda: ops.rng_fill(P, 3 * R, ops.RNG_NORMAL, SEED, step, ops.RNG_SIGMA, 1.0, out=buf)
        cases = {
            "compact_plain": lambda: ops.cells_gather(x, rows, total, 0, None),
            "compact_fill_then_gather": lambda: ops.cells_gather(x, rows, total, 0, fill()),
            "compact_rng": lambda: ops.cells_gather_rng(x, rows, total, 0, SEED, step, ops.RNG_SIGMA, R, 3, 1.0),
            "padded_plain": lambda: ops.cells_gather_padded(x, prow, cen, C, 0, None),
            "padded_fill_then_gather": lambda: ops.cells_gather_padded(x, prow, cen, C, 0, fill()),
            "padded_rng": lambda: ops.cells_gather_padded_rng(x, prow, cen, C, 0, SEED, step, ops.RNG_SIGMA, R, 3, 1.0),
        }
        rec = dict(points=P, cells=K, members=total, C=C, padded_rows=K * C)
        for name, fn in cases.items():
            with limit(120):
                rec[name + "_us"] = ev_time(fn)
        out[tag] = rec
    return out


def step_times():
    from test_mega_train_gpu import _dev, _load, _mega
    g = _load("mega_train")
    N, S, F = int(g["N"]), int(g["S"]), int(g["F"])
    args = (_dev(g["rgbs"]), _dev(g["rays"]), _dev(g["image_indices"]), S)
    out = {}
    for form, cap in (("compact", None), ("padded", (768, 384))):
        drawn, supplied = _mega(g, 1.0), _mega(g, 1.0)
        drawn.set_device_noise(SEED, 5, 3)
        st = ops.rng_step_tensor(5, "cuda")
        fill = lambda sid, R, kind: ops.rng_fill(N * R, 3 * R, kind, SEED, st, sid, 1.0)

        def run_supplied():
            supplied.grad_step(*args, 1.0, fill(0, S, 0).view(N, S), fill(1, S, 1), F, fill(2, F, 0).view(N, F), fill(3, F, 1), cap)
            ops.rng_advance(st)

        variants = {"drawn": lambda: drawn.grad_step(*args, 1.0, fine_samples=F, cell_capacity=cap, sigma_noise_std=1.0),
                    "supplied": run_supplied}
        rec = {}
        for name, fn in variants.items():
            ts = []
            with limit(240):
                for _ in range(5):
                    fn()
                torch.cuda.synchronize()
                for _ in range(5):
                    t0 = time.perf_counter()
                    for _ in range(20):
                        fn()
                    torch.cuda.synchronize()
                    ts.append((time.perf_counter() - t0) / 20 * 1e3)
            rec[name + "_ms"] = dict(median=float(np.median(ts)), min=min(ts), max=max(ts))
        out[form] = rec
    return out


def main():
    assert torch.cuda.is_available(), "bench_mega_noise.py needs a GPU"
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__)
    res["kernels_fixture"] = kernels(2048, 3)
    print(json.dumps(dict(kernels_fixture=res["kernels_fixture"])), flush=True)
    res["kernels_2M"] = kernels(2097152, 8)
    print(json.dumps(dict(kernels_2M=res["kernels_2M"])), flush=True)
    res["step"] = step_times()
    print(json.dumps(dict(step=res["step"])), flush=True)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
