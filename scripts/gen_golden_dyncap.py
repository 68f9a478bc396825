"""Fixtures of the dynamic MoE capacity (capacity_factor <= 0, tutel_fast_dispatch.py:210-216) from the REFERENCE's own run.

Usage (build container only, like oracle/gen_golden.py whose recipes it calls):
    python scripts/gen_golden_dyncap.py

Writes new tests/golden/*.npz files only:
  render_train_cf000_bpr, render_train_cf000_nobpr, render_train_cfm050_bpr   (oracle/gen_golden.py gen_render: 64 rays x 64
      samples, chunk 1024, fp32 train step at cf = 0 / -0.5)
  moe_layer_dyncap_top1_cf000, moe_layer_dyncap_top1_cfm050, moe_layer_dyncap_top2_cf000   (the reference's MoE layer at cf <= 0,
      fwd + bwd; the same recipe as gen_golden.py's moe-layer fixtures with the capacity factor as a parameter; outputs and gradients
      as checksums + strided slices)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden as gg  # noqa: E402
import synth  # noqa: E402      (on the path through gen_golden)


def gen_render_dyncap():
    gg.gen_render((("cf000_bpr", 1.0, 0.0, True), ("cf000_nobpr", 1.0, 0.0, False), ("cfm050_bpr", 1.0, -0.5, True)))


def gen_moe_layer_dyncap():
    print("[dyncap] moe_layer fwd + bwd at capacity_factor <= 0 (top-1, top-2)")
    for tag, k, cf, P, seed, bpr in (("top1_cf000", 1, 0.0, 1024, 41, True), ("top1_cfm050", 1, -0.5, 1024, 42, True),
                                     ("top2_cf000", 2, 0.0, 768, 43, True)):
        cfg = synth.BUILDING
        sd = synth.make_weights(seed, cfg)
        nerf, h = gg.build_reference_model(cfg, sd, bpr=bpr, capacity_factor=cf)
        moe = nerf.layers["0"]
        if k != 1:
            moe.gates[0].top_k = k
        rng = np.random.default_rng(seed + 1000)
        x = rng.standard_normal((P, cfg["model_dim"])).astype(np.float32)
        gi = rng.standard_normal((P, cfg["gate_hidden"])).astype(np.float32)
        xt = torch.from_numpy(x).requires_grad_(True)
        gt = torch.from_numpy(gi).requires_grad_(True)
        y = moe(xt, gate_input=gt)
        l_aux = y.l_aux
        dy = rng.standard_normal(y.shape).astype(np.float32)
        (y * torch.from_numpy(dy)).sum().backward()
        grads = {n: p.grad.clone() for n, p in moe.named_parameters()}
        out = dict(seed=seed, P=P, k=k, cf=cf, bpr=int(bpr), l_aux=l_aux.detach().numpy(), topk=y.gate_extras["gates"].numpy().astype(np.int32))
        # the [P, 256] outputs as a checksum and a strided slice (2 values of every token's row): keeps the fixture small
        for n, t in (("y", y.detach()), ("dx", xt.grad), ("dgate_input", gt.grad)):
            a = t.numpy()
            out["sum__" + n] = synth.checksum(a)
            out["slice__" + n] = a.reshape(-1)[:: max(1, a.size // 2048)][:2048]
        for n, g_ in grads.items():
            out["gsum__" + n] = synth.checksum(g_.numpy())
            out["gslice__" + n] = g_.numpy().reshape(-1)[:: max(1, g_.numel() // 997)][:997]
        gg.save(f"moe_layer_dyncap_{tag}", **out)


if __name__ == "__main__":
    os.makedirs(gg.OUT, exist_ok=True)
    torch.set_num_threads(8)
    gen_render_dyncap()
    gen_moe_layer_dyncap()
