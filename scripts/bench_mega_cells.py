"""The spatial-cell kernels of the Mega-NeRF model (csrc/cells.hip), the measurements of profiles/r13_mega_cells.md: per-call device
time of swn_cells_assign / _pack / _gather / _blend at P = 131072 points, K = 8 cells, boundary_margin 1 and 1.15, beside the same
routing done with torch ops on the device the way the reference's MegaNeRF.forward does it (cdist, masks, boolean indexing, masked
adds).  Event timing after a warm-up; each figure is the median of 5 windows of 200 calls.  Achieved bandwidth is on ALGORITHMIC bytes
(what the operation has to read and write once, computed from the shapes below), over the 8.0 TB/s HBM3E peak of the MI355X.

    python scripts/bench_mega_cells.py [result.json]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from switch_nerf_amd import ops

P, K, STRIDE, C = 131072, 8, 7, 4
HBM_PEAK = 8.0e12


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


def torch_assign(x, cen, margin):
    d = torch.cdist(x[:, :3], cen)
    if margin > 1:
        inv = 1 / (d + 1e-8)
        inv[d > margin * d.min(dim=1)[0].unsqueeze(-1).repeat(1, d.shape[1])] = 0
        return inv / inv.sum(dim=-1).unsqueeze(-1)
    return d.argmin(dim=1)


def torch_masks(w, margin):
    return [(w == i) if margin == 1 else (w[:, i] > 0) for i in range(K)]


def torch_gather(x, noise, masks):
    return [(x[m], noise[m]) for m in masks]


def torch_blend(w, masks, subs, margin):
    out = torch.zeros(P, C, device="cuda")
    for i, (m, s) in enumerate(zip(masks, subs)):
        if margin == 1:
            out[m] = s
        else:
            out[m] += s * w[m, i].unsqueeze(-1)
    return out


def main():
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, P=P, K=K, stride=STRIDE, channels=C)
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand(P, STRIDE, device="cuda", generator=g) * 2 - 1
    cen = torch.rand(K, 3, device="cuda", generator=g) * 1.6 - 0.8
    noise = torch.randn(P, device="cuda", generator=g)
    for margin in (1.0, 1.15):
        tag = "m100" if margin == 1 else "m115"
        w, counts = ops.cells_assign(x, cen, 0, margin)
        begin, rows, slot = ops.cells_pack(w, counts)
        total = int(counts.sum().item())
        xin, nin = ops.cells_gather(x, rows, total, 0, noise)
        sub = torch.rand(total, C, device="cuda", generator=g)
        hard = margin == 1
        us = dict(assign=ev_time(lambda: ops.cells_assign(x, cen, 0, margin)),
                  pack=ev_time(lambda: ops.cells_pack(w, counts)),
                  gather=ev_time(lambda: ops.cells_gather(x, rows, total, 0, noise)),
                  blend=ev_time(lambda: ops.cells_blend(w, slot, begin, sub, hard)))
        nbytes = dict(assign=P * 12 + P * K * 4 + K * 4,
                      pack=P * K * 4 + K * 4 + (K + 1) * 4 + total * 4 + P * K * 4,
                      gather=total * 4 + 2 * total * STRIDE * 4 + 2 * total * 4,
                      blend=P * K * 4 + (0 if hard else total * 4) + total * C * 4 + P * C * 4)
        # the reference's formulation with torch ops (boolean indexing synchronises with the host: part of what it costs)
        tw = torch_assign(x, cen, margin)
        masks = torch_masks(tw, margin)
        subs = [sub[int(begin[i]):int(begin[i + 1])] for i in range(K)]
        t_us = dict(assign=ev_time(lambda: torch_assign(x, cen, margin), 50),
                    pack=ev_time(lambda: torch_masks(tw, margin), 50),
                    gather=ev_time(lambda: torch_gather(x, noise, masks), 50),
                    blend=ev_time(lambda: torch_blend(tw, masks, subs, margin), 50))
        res[tag] = dict(total_rows=total, kernel_us=us, algorithmic_bytes=nbytes,
                        hbm_fraction={k: nbytes[k] / (us[k] * 1e-6) / HBM_PEAK for k in us}, torch_us=t_us,
                        kernel_us_sum=sum(us.values()), torch_us_sum=sum(t_us.values()))
        print(json.dumps({tag: res[tag]}), flush=True)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
