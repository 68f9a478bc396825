"""CPU-only: the residual MoE branch of the layer mirror (moe_layer(use_residual=True), tutel_moe_layer_nobatch.py:504-505, 666-671)
constructs with the reference layer's parameter names and shapes (recorded in the fixtures of scripts/gen_golden_residual.py), loads
the reference's state_dict strictly, and leaves the layer without it exactly as it was."""
import os

import numpy as np
import pytest
import torch

import residual_weights
import synth

G = os.path.join(os.path.dirname(__file__), "golden")
TAGS = ["top1_cf100", "top1_cf000", "top2_cf100", "m64e4_p1000"]


def _layer(cfg, k=1, cf=1.0, **kw):
    from switch_nerf_amd.moe import moe_layer
    return moe_layer(gate_type=dict(type="top", k=k, fp32_gate=True, capacity_factor=cf, batch_prioritized_routing=True, gate_noise=-1.0,
                                    compute_balance_loss=False, dispatcher_no_score=False, is_postscore=True, gate_dim=cfg["gate_hidden"]),
                     model_dim=cfg["model_dim"],
                     experts=dict(type="expertmlp", count_per_node=cfg["num_experts"], hidden_size_per_expert=cfg["model_dim"],
                                  layer_num=cfg["expert_layers"], skips=list(cfg["skips"])),
                     seeds=(1, 1, 1), return_gates=True, dtype=torch.float32, **kw)


def _cfg(g):
    M, E = int(g["model_dim"]), int(g["n_experts"])
    return synth.BUILDING if M == 256 else dict(synth.small_cfg(M, E), gate_hidden=int(g["gate_dim"]))


@pytest.mark.parametrize("tag", TAGS)
def test_residual_layer_parameters_equal_the_reference(tag):
    g = np.load(os.path.join(G, f"moe_layer_residual_{tag}.npz"))
    cfg = _cfg(g)
    moe = _layer(cfg, int(g["k"]), float(g["cf"]), use_residual=True)
    assert moe.use_residual
    ref = {str(n): tuple(int(d) for d in g["pshape__" + str(n)]) for n in g["names"]}
    got = {n: tuple(p.shape) for n, p in moe.named_parameters()}
    assert set(got) == set(ref), sorted(set(got) ^ set(ref))      # the set, not the order: the mirror registers the gate first
    assert got == ref
    assert all(p.dtype == torch.float32 for p in moe.parameters())
    moe.load_state_dict({k: torch.from_numpy(v) for k, v in residual_weights.layer_state_dict(int(g["seed"]), cfg).items()}, strict=True)
    assert torch.equal(moe.coefficient.weight, torch.from_numpy(residual_weights.make_residual_weights(int(g["seed"]), cfg)["coefficient.weight"]))


def test_layer_without_residual_keeps_its_parameters():
    cfg = synth.BUILDING
    L = cfg["expert_layers"]
    old = {"gates.0.wg.weight"} | {f"experts.0.weights.{l}" for l in range(L)} | {f"experts.0.bias.{l}" for l in range(L)}
    for kw in ({}, {"use_residual": False}):
        moe = _layer(cfg, **kw)
        assert [n for n, _ in moe.named_parameters()] == ["gates.0.wg.weight"] + [f"experts.0.weights.{l}" for l in range(L)] + \
            [f"experts.0.bias.{l}" for l in range(L)]
        assert set(moe.state_dict()) == old and not moe.use_residual
        assert not hasattr(moe, "coefficient") and not hasattr(moe, "residual_expert")


def test_residual_expert_is_drawn_after_the_experts_from_the_same_seed():
    """Seeded like the reference (tutel_moe_layer_nobatch.py:654-671): the experts come out as without the branch, the residual
    expert continues the same generator."""
    cfg = synth.small_cfg(64, 4)
    a, b = _layer(cfg, use_residual=True), _layer(cfg)
    for l in range(cfg["expert_layers"]):
        assert torch.equal(a.experts[0].weights[l], b.experts[0].weights[l])
    assert not torch.equal(a.residual_expert.weights[0][0], a.experts[0].weights[0][0])
    c = _layer(cfg, use_residual=True)
    assert torch.equal(a.residual_expert.weights[3], c.residual_expert.weights[3])


def test_residual_layer_refuses_cpu_tensors():
    moe = _layer(synth.small_cfg(64, 4), use_residual=True)
    x = torch.randn(10, 64)
    with pytest.raises(RuntimeError, match="HIP library only"):
        moe(x, gate_input=x)
