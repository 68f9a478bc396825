"""Seeded weights of the MoE layer's residual branch (use_residual): the `coefficient` Linear and the one-expert `residual_expert`
ExpertMLP, with the reference layer's names and shapes.  The fixture generator (scripts/gen_golden_residual.py) and the tests regenerate
them; no fixture stores them."""
from __future__ import annotations

import numpy as np

import synth

COEF_SCALE = 2.0      # spreads the mixing weights c well away from 0.5 (|logit difference| ~ 1.6 for unit-variance inputs)


def make_residual_weights(seed: int, cfg=synth.BUILDING, coef_scale: float = COEF_SCALE):
    """{state_dict key: np.float32 array}: coefficient.weight [2, M], coefficient.bias [2], residual_expert.weights.{l} [1, M, M]
    ([in, out] like the experts), residual_expert.bias.{l} [1, 1, M]."""
    rng = np.random.default_rng(seed + 7000)
    M, L = cfg["model_dim"], cfg["expert_layers"]
    sd = {}
    sd["coefficient.weight"], sd["coefficient.bias"] = synth._linear(rng, 2, M, scale=coef_scale)
    for l in range(L):
        wt, bt = synth._linear(rng, M, M)
        sd[f"residual_expert.weights.{l}"] = np.ascontiguousarray(wt.T[None])
        sd[f"residual_expert.bias.{l}"] = bt.reshape(1, 1, M).copy()
    return sd


def layer_state_dict(seed: int, cfg=synth.BUILDING):
    """The whole residual layer's state_dict: gate and experts of synth.make_weights(seed) (the `layers.0.` entries) plus the above."""
    sd = {k[len("layers.0."):]: v for k, v in synth.make_weights(seed, cfg).items() if k.startswith("layers.0.")}
    sd.update(make_residual_weights(seed, cfg))
    return sd
