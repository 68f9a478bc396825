"""swn_cells_blend_sh (csrc/sh.hip), the measurements of profiles/r15_mega_sh.md: per-call device time at P = 2 M points (32768 rays x 64
samples, one direction per ray), K = 8 cells, boundary_margin 1 and 1.15, sh_deg 0 / 2 / 4, of
  fused      one launch: blend of the cells' rows of 3 B + 1 floats + sigmoid(eval_sh) -> raw [P, 4]
  two_step   the same launch leaving the blended rows too (coef_out [P, 3 B + 1]), then a separate evaluation of those rows: the same
             entry point over one cell with the identity packing (hard), which reads every blended row back once
beside the ALGORITHMIC bytes each moves (what it has to read and write once, from the shapes), over the 8.0 TB/s HBM3E peak of the
MI355X.  Event timing after a warm-up; each figure is the median of 5 windows of 20 calls.

    python scripts/bench_mega_sh.py [result.json]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from switch_nerf_amd import ops

N_RAYS, S, K = 32768, 64, 8
P = N_RAYS * S
HBM_PEAK = 8.0e12


def ev_time(fn, iters=20, windows=5):
    for _ in range(5):
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


def main():
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, P=P, K=K, rows_per_group=S)
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand(P, 4, device="cuda", generator=g) * 2 - 1
    cen = torch.rand(K, 3, device="cuda", generator=g) * 1.6 - 0.8
    dirs = torch.nn.functional.normalize(torch.randn(N_RAYS, 3, device="cuda", generator=g), dim=1).contiguous()
    ident = (torch.ones(P, 1, device="cuda"), torch.arange(P, dtype=torch.int32, device="cuda").view(P, 1),
             torch.tensor([0, P], dtype=torch.int32, device="cuda"))
    for margin in (1.0, 1.15):
        w, counts = ops.cells_assign(x, cen, 0, margin)
        begin, rows, slot = ops.cells_pack(w, counts)
        total, hard = int(counts.sum().item()), margin == 1
        del rows
        for deg in (0, 2, 4):
            wd = 3 * (deg + 1) ** 2 + 1
            sub = torch.rand(total, wd, device="cuda", generator=g) * 2 - 1
            _, coef = ops.cells_blend_sh(w, slot, begin, sub, dirs, S, deg, hard, want_coef=True)
            us = dict(fused=ev_time(lambda: ops.cells_blend_sh(w, slot, begin, sub, dirs, S, deg, hard)),
                      blend_rows=ev_time(lambda: ops.cells_blend_sh(w, slot, begin, sub, dirs, S, deg, hard, want_coef=True)),
                      eval_rows=ev_time(lambda: ops.cells_blend_sh(*ident, coef, dirs, S, deg, True)))
            us["two_step"] = us["blend_rows"] + us["eval_rows"]
            route = P * K * 4 + (0 if hard else P * K * 4)          # slot, and the weights where they are read
            nbytes = dict(fused=route + total * wd * 4 + N_RAYS * 12 + P * 16)
            nbytes["blend_rows"] = nbytes["fused"] + P * wd * 4
            nbytes["eval_rows"] = P * 8 + P * wd * 4 + N_RAYS * 12 + P * 16
            nbytes["two_step"] = nbytes["blend_rows"] + nbytes["eval_rows"]
            tag = f"{'m100' if hard else 'm115'}_d{deg}"
            res[tag] = dict(total_rows=total, row_floats=wd, kernel_us=us, algorithmic_bytes=nbytes,
                            hbm_fraction={k: nbytes[k] / (us[k] * 1e-6) / HBM_PEAK for k in us})
            print(json.dumps({tag: res[tag]}), flush=True)
            del sub, coef
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
