"""Times swn_heads_sh_fwd / swn_heads_sh_bwd at P = 8192 x 256, W = 256 (M 256, H2 128), bf16, deg 2 and 3, next to swn_heads_fwd /
swn_heads_bwd and a torch formulation of the SH heads (addmm + polynomial + sigmoid) in the SAME process.

    python scripts/bench_sh_heads.py [--rays 8192] [--samples 256]

Per kernel: 5 warm-up launches, then 20 timed launches between HIP events after a 512 MiB cache flush each; the median is reported,
with the bytes the algorithm has to move (inputs read once, outputs written once) and that as a fraction of the 8 TB/s HBM peak."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from switch_nerf_amd import ops as o  # noqa: E402
import sh_restate as R  # noqa: E402

PEAK = 8.0e12


def timed(fn, flush, warm=5, reps=20):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        flush.zero_()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--samples", type=int, default=256)
    a = ap.parse_args()
    N, S, M, H2, dt = a.rays, a.samples, 256, 128, torch.bfloat16
    P = N * S
    g = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    y, h2 = torch.relu(r(P, M)).to(dt), torch.relu(r(P, H2)).to(dt)
    ws, bs, d_raw = r(M) / 16, r(1), r(P, 4)
    dirs = torch.nn.functional.normalize(r(N, 3), dim=1).contiguous()
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    rows = []

    def report(name, t, nbytes):
        rows.append((name, t[0] * 1e6, t[1] * 1e6, t[2] * 1e6, nbytes / 1e9, nbytes / t[0] / PEAK))
        print(f"{name:28s} median {t[0] * 1e6:8.1f} us  (min {t[1] * 1e6:8.1f}, max {t[2] * 1e6:8.1f})  {nbytes / 1e9:6.3f} GB  "
              f"{nbytes / t[0] / 1e12:5.2f} TB/s = {100 * nbytes / t[0] / PEAK:4.1f} % of peak", flush=True)

    in_fwd = P * (M + H2) * 2
    wc3, bc3 = r(3, H2) / 8, r(3)
    raw3 = o.heads_fwd(y, h2, ws, bs, wc3, bc3, None)
    report("heads_fwd", timed(lambda: o.heads_fwd(y, h2, ws, bs, wc3, bc3, None), flush), in_fwd + P * 16)
    acc = [torch.zeros(M, device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(3, H2, device="cuda"), torch.zeros(3, device="cuda")]
    in_bwd = P * (M + H2) * 2 + P * 32
    out_bwd = P * H2 * 2 + P * 4
    report("heads_bwd", timed(lambda: o.heads_bwd(y, h2, wc3, raw3, d_raw, *acc, rows_per_group=S), flush), in_bwd + out_bwd)
    for deg in (2, 3):
        B = (deg + 1) ** 2
        wc, bc = r(3 * B, H2) / 8, r(3 * B)
        raw = o.heads_sh_fwd(y, h2, ws, bs, wc, bc, None, dirs, S, deg)
        report(f"heads_sh_fwd deg {deg}", timed(lambda: o.heads_sh_fwd(y, h2, ws, bs, wc, bc, None, dirs, S, deg), flush), in_fwd + P * 16)
        report(f"heads_sh_fwd deg {deg} + coef", timed(lambda: o.heads_sh_fwd(y, h2, ws, bs, wc, bc, None, dirs, S, deg, want_coef=True), flush),
               in_fwd + P * 16 + P * 3 * B * 4)
        accs = [torch.zeros(M, device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(3 * B, H2, device="cuda"), torch.zeros(3 * B, device="cuda")]
        report(f"heads_sh_bwd deg {deg}", timed(lambda: o.heads_sh_bwd(y, h2, wc, bc, dirs, raw, d_raw, *accs, S, deg), flush), in_bwd + out_bwd)

        def torch_fwd():
            lin = torch.addmm(bc.to(dt), h2, wc.to(dt).t())
            Y = R.basis(deg, dirs).repeat_interleave(S, 0)
            rgb = torch.sigmoid((lin.view(P, 3, B).float() * Y[:, None, :]).sum(-1))
            sig = torch.nn.functional.softplus(y.float() @ ws + bs - 1)
            return torch.cat([rgb, sig[:, None]], 1)
        report(f"torch formulation deg {deg}", timed(torch_fwd, flush, warm=2, reps=5), in_fwd + P * 16)
    print("| kernel | median us | min | max | GB | of 8 TB/s |\n|---|---|---|---|---|---|")
    for n, m, lo, hi, gb, fr in rows:
        print(f"| {n} | {m:.1f} | {lo:.1f} | {hi:.1f} | {gb:.3f} | {100 * fr:.1f} % |")


if __name__ == "__main__":
    main()
