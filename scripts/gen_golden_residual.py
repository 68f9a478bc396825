"""Fixtures of the MoE layer's residual branch (use_residual, tutel_moe_layer_nobatch.py:504-505, 666-671, 777-788) from the REFERENCE
layer's own run.

Usage (build container only, like oracle/gen_golden.py whose imports it uses):
    python scripts/gen_golden_residual.py

Builds the reference MOELayer(use_residual=True) on the CPU in fp32, loads gate and experts from synth.make_weights(seed) and the
coefficient / residual expert from tests/residual_weights.py, runs the forward and a backward of sum(y * dy) + l_aux, and writes
tests/golden/moe_layer_residual_{tag}.npz: the parameter names and shapes, l_aux, the top-k indices, the per-token mixing weights coef
[P, 2] in full, and y / dx / dgate_input / every parameter gradient as checksums + strided slices (like the dyncap fixtures).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden as gg  # noqa: E402
import synth  # noqa: E402      (on the path through gen_golden)
import residual_weights as rw  # noqa: E402
from switch_nerf.modules.tutel_moe_ext.tutel_moe_layer_nobatch import MOELayer  # noqa: E402

# tag, cfg, top-k, capacity factor, P, seed
CASES = (("top1_cf100", synth.BUILDING, 1, 1.0, 1024, 51),
         ("top1_cf000", synth.BUILDING, 1, 0.0, 1024, 52),
         ("top2_cf100", synth.BUILDING, 2, 1.0, 768, 53),
         ("m64e4_p1000", dict(synth.small_cfg(64, 4), gate_hidden=128), 1, 1.0, 1000, 54))      # (gate input: 128 features)


def reference_layer(cfg, k, cf):
    gate_type = dict(type="top", k=k, fp32_gate=True, capacity_factor=cf, batch_prioritized_routing=True, gate_noise=-1.0,
                     compute_balance_loss=False, dispatcher_no_score=False, is_postscore=True, gate_dim=cfg["gate_hidden"])
    experts = dict(type="expertmlp", count_per_node=cfg["num_experts"], hidden_size_per_expert=cfg["model_dim"],
                   layer_num=cfg["expert_layers"], skips=list(cfg["skips"]), init_factor=1.0, init_trunc_normal=False)
    torch.manual_seed(0)
    return MOELayer(gate_type, cfg["model_dim"], experts=experts, seeds=(1, 1, 1), use_residual=True, return_gates=True)


def gen_moe_layer_residual():
    print("[residual] moe_layer(use_residual=True) fwd + bwd (top-1 cf 1 / cf 0, top-2, M=64 ragged)")
    for tag, cfg, k, cf, P, seed in CASES:
        moe = reference_layer(cfg, k, cf)
        sd = rw.layer_state_dict(seed, cfg)
        moe.load_state_dict({n: torch.from_numpy(v.copy()) for n, v in sd.items()}, strict=True)
        rng = np.random.default_rng(seed + 1000)
        x = rng.standard_normal((P, cfg["model_dim"])).astype(np.float32)
        gi = rng.standard_normal((P, cfg["gate_hidden"])).astype(np.float32)
        xt = torch.from_numpy(x).requires_grad_(True)
        gt = torch.from_numpy(gi).requires_grad_(True)
        y = moe(xt, gate_input=gt)
        l_aux = y.l_aux
        with torch.no_grad():
            coef = torch.softmax(moe.coefficient(xt), dim=-1)           # the forward's mixing weights (tutel_moe_layer_nobatch.py:785-786)
        dy = rng.standard_normal(tuple(y.shape)).astype(np.float32)
        ((y * torch.from_numpy(dy)).sum() + l_aux).backward()
        names = [n for n, _ in moe.named_parameters()]
        out = dict(seed=seed, P=P, k=k, cf=cf, bpr=1, model_dim=cfg["model_dim"], n_experts=cfg["num_experts"], gate_dim=cfg["gate_hidden"],
                   l_aux=l_aux.detach().numpy(), topk=y.gate_extras["gates"].numpy().astype(np.int32), coef=coef.numpy(),
                   names=np.array(names))
        for n, p in moe.named_parameters():
            out["pshape__" + n] = np.array(p.shape, np.int64)
        for n, t in (("y", y.detach()), ("dx", xt.grad), ("dgate_input", gt.grad)):
            a = t.numpy()
            out["sum__" + n] = synth.checksum(a)
            out["slice__" + n] = a.reshape(-1)[:: max(1, a.size // 2048)][:2048]
        for n, p in moe.named_parameters():
            g_ = p.grad.numpy()
            out["gsum__" + n] = synth.checksum(g_)
            out["gslice__" + n] = g_.reshape(-1)[:: max(1, g_.size // 997)][:997]
        c = coef.numpy()
        print(f"  {tag}: coef[:, 0] in [{c[:, 0].min():.3f}, {c[:, 0].max():.3f}], |c0 - 0.5| mean {np.abs(c[:, 0] - 0.5).mean():.3f}")
        gg.save(f"moe_layer_residual_{tag}", **out)


if __name__ == "__main__":
    os.makedirs(gg.OUT, exist_ok=True)
    torch.set_num_threads(8)
    gen_moe_layer_residual()
