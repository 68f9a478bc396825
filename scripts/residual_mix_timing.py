"""Timing of the MoE layer's residual branch (use_residual; switch_nerf_amd/csrc/residual.hip).

    python scripts/residual_mix_timing.py [--tokens 2097152]

1. swn_residual_mix_fwd and swn_residual_mix_bwd at P tokens x M = 256, bf16: device time per call (hipEvent, median of 20) and the
   effective rate over the algorithmic bytes - forward: x, y_moe, y_res read, y written (4 P M 2 B) + coef (8 P B); backward: dy, x,
   y_moe, y_res read, d_moe, d_res, dx written (7 P M 2 B) + coef (8 P B).
2. The whole bf16 layer (top-1, cf 1.0, E = 8) with and without use_residual at the same P: forward + backward wall time (median of 5,
   device-synchronised), so the residual branch's share of the layer shows.
Prints one JSON line.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _median_ms(fn, reps):
    for _ in range(3):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


def time_mix(P, M):
    from switch_nerf_amd import ops
    g = torch.Generator(device="cuda").manual_seed(1)
    x, ym, yr, dy = (torch.randn(P, M, device="cuda", generator=g).to(torch.bfloat16) for _ in range(4))
    wc = torch.randn(2, M, device="cuda", generator=g) / M ** 0.5
    bc = torch.zeros(2, device="cuda")
    _, coef = ops.residual_mix_fwd(x, ym, yr, wc, bc)
    fwd = _median_ms(lambda: ops.residual_mix_fwd(x, ym, yr, wc, bc), 20)
    bwd = _median_ms(lambda: ops.residual_mix_bwd(dy, x, ym, yr, coef, wc), 20)
    b_fwd = 4 * P * M * 2 + 8 * P
    b_bwd = 7 * P * M * 2 + 8 * P
    return dict(tokens=P, model_dim=M, dtype="bf16", fwd_ms=round(fwd, 4), fwd_bytes=b_fwd, fwd_tb_per_s=round(b_fwd / fwd / 1e9, 3),
                bwd_ms=round(bwd, 4), bwd_bytes=b_bwd, bwd_tb_per_s=round(b_bwd / bwd / 1e9, 3))


def time_layer(P, use_residual):
    import residual_weights
    import synth
    from switch_nerf_amd.moe import moe_layer
    cfg = synth.BUILDING
    moe = moe_layer(gate_type=dict(type="top", k=1, fp32_gate=True, capacity_factor=1.0, batch_prioritized_routing=True,
                                   gate_dim=cfg["gate_hidden"]), model_dim=256,
                    experts=dict(type="expertmlp", count_per_node=cfg["num_experts"], hidden_size_per_expert=256,
                                 layer_num=cfg["expert_layers"], skips=list(cfg["skips"])),
                    seeds=(1, 1, 1), use_residual=use_residual, dtype=torch.bfloat16).cuda()
    sd = residual_weights.layer_state_dict(51, cfg)
    if not use_residual:
        sd = {k: v for k, v in sd.items() if not k.startswith(("coefficient.", "residual_expert."))}
    moe.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    g = torch.Generator(device="cuda").manual_seed(2)
    x = torch.randn(P, 256, device="cuda", generator=g).to(torch.bfloat16).requires_grad_(True)
    gi = torch.randn(P, 256, device="cuda", generator=g).to(torch.bfloat16)
    dy = torch.randn(P, 256, device="cuda", generator=g).to(torch.bfloat16)

    def step():
        y = moe(x, gate_input=gi)
        ((y * dy).sum() + y.l_aux).backward()
    return round(_median_ms(step, 5), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=1 << 21)
    a = ap.parse_args()
    out = dict(mix=time_mix(a.tokens, 256))
    out["layer_fwd_bwd_ms"] = dict(tokens=a.tokens, plain=time_layer(a.tokens, False), residual=time_layer(a.tokens, True))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
