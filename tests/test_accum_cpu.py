"""CPU-only: the host side of gradient accumulation (SwitchNeRF.set_accumulation) that needs no kernel - the window rule, the argument
check - and the consistency of tests/golden/accum_train.npz (scripts/gen_golden_accum.py)."""
import os

import numpy as np
import pytest
import torch

import synth

G = os.path.join(os.path.dirname(__file__), "golden")


def test_window_rule_is_the_references():
    """(it + 1) % A != 0 (runner.py:589), from the module function and from a model's own micro-step index."""
    from switch_nerf_amd.dense import DenseNeRF
    from switch_nerf_amd.model import accumulation_rule
    for A in range(1, 5):
        m = DenseNeRF(synth.DENSE, dtype=torch.float32, device="cpu")
        m.set_accumulation(A)
        assert (m.accum is None) == (A == 1) and m.accum_steps == A
        for it in range(12):
            want = (it + 1) % A != 0
            assert accumulation_rule(it, A) is want
            assert m._accumulates() is want and m._micro == it + 1
        assert m._accumulates(True) is True and m._accumulates(False) is False and m._micro == 14      # an explicit bool wins, the index advances
        if A > 1:
            assert m.accum.shape == m.grad.shape and m.accum.dtype == torch.float32 and not m.accum.any()
        m.set_accumulation(A)
        assert m._micro == 0


def test_set_accumulation_rejects_less_than_one():
    from switch_nerf_amd.cascade import Cascade
    from switch_nerf_amd.dense import DenseNeRF
    from switch_nerf_amd.model import SwitchNeRF
    m = SwitchNeRF(synth.BUILDING, dtype=torch.float32, device="cpu")
    for bad in (0, -1):
        with pytest.raises(ValueError, match="accumulation"):
            m.set_accumulation(bad)
    assert m.accum_steps == 1 and m.accum is None
    c = Cascade(DenseNeRF(synth.DENSE, dtype=torch.float32, device="cpu"), DenseNeRF(synth.DENSE, dtype=torch.float32, device="cpu"))
    with pytest.raises(ValueError, match="accumulation"):
        c.set_accumulation(0)
    c.set_accumulation(3)
    assert c.accum_steps == 3 and all(h.accum is not None for h in c.halves())


def test_fixture_is_self_consistent():
    """The seeded weights are the ones the fixture was made from; the accumulated gradient before the first optimizer step equals the
    sum of the window's micro-gradients (both of the loss / A) within the rounding of an A-term fp32 sum."""
    g = np.load(os.path.join(G, "accum_train.npz"))
    every, every_micro = int(g["every"]), int(g["every_micro"])
    assert every_micro % every == 0
    for kind, sd in (("moe", synth.make_weights(int(g["seed_moe"]), synth.BUILDING, gate_scale=1.0)),
                     ("dense", synth.make_dense_weights(int(g["seed_dense"]), synth.DENSE))):
        np.testing.assert_array_equal(np.stack([synth.checksum(v) for v in sd.values()]), g[kind + "_sd_checksums"])
        names = [str(n) for n in g[kind + "_param_names"]]
        assert set(names) == set(sd)
        offs, moffs = g[kind + "_offsets"], g[kind + "_micro_offsets"]
        assert len(offs) == len(moffs) == len(names) + 1
        for A, n_micro in g["cases"]:
            tag = f"{kind}_a{A}_"
            for step in range(int(n_micro) // int(A)):
                acc = g[tag + f"s{step}_gslice__"]
                assert g[tag + f"s{step}_pslice__"].shape == acc.shape == (offs[-1],)
                assert g[tag + f"s{step}_gsum__"].shape == g[tag + f"s{step}_psum__"].shape == (len(names), 3)
                micro = [g[tag + f"m{it}_gslice__"] for it in range(step * int(A), (step + 1) * int(A))]
                for i in range(len(names)):
                    a = acc[offs[i]: offs[i + 1]][:: every_micro // every]
                    parts = np.stack([mg[moffs[i]: moffs[i + 1]] for mg in micro]).astype(np.float64)
                    assert a.shape == parts.shape[1:]
                    bound = int(A) * np.finfo(np.float32).eps * np.abs(parts).sum(0) + 1e-45
                    assert (np.abs(a - parts.sum(0)) <= bound).all(), (tag, step, names[i])
            for it in range(int(n_micro)):
                assert np.isfinite(g[tag + f"m{it}_loss"]) and g[f"{kind}_mb{it}_rays"].shape == (int(g["N"]), 8)
