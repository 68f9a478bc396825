"""SHA-256 of what one step computes on every path of the MoE step's host-side orchestration (SwitchNeRF in its local, fused, packed,
ragged, hierarchical, no-batch and expert-parallel forms, the dense model, and the three autograd functions of MoELayer), each at the
smallest shape that selects the path, on seeded tests/synth.py inputs.  One JSON line per case: per field the digest of the first run
and whether a second run in the same process gave the same bits (`same`; where it did not, `rel` = the max relative difference of
the two runs).  Run it once per commit and compare the lines: a field a commit reproduces must have equal digests on both.

    python scripts/step_bits.py                     every case, one line each
    python scripts/step_bits.py --case ragged       one case (a caller that wants a time limit per case runs them one by one)
    python scripts/step_bits.py --list              the case names
    ... --save DIR      also write the fields that did NOT reproduce as DIR/<case>.<field>.npy
    ... --against DIR   for every field with a file in DIR: `vs` = the max relative difference to it
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import synth  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def model(dtype=BF16, seed=300, **kw):
    from switch_nerf_amd.model import SwitchNeRF
    m = SwitchNeRF(synth.BUILDING, dtype=dtype, **kw)
    m.load_state_dict(synth.make_weights(seed, synth.BUILDING, gate_scale=1.0))
    return m


def train(N=64, S=64, chunk=2048, dtype=BF16, switches=None, ep=None, fine=0, dense=False, **kw):
    """One grad_step of a fresh model: raw, rgb, loss and the flat gradient."""
    def run():
        if dense:
            from switch_nerf_amd.dense import DenseNeRF
            m = DenseNeRF(synth.DENSE, dtype=dtype)
            m.load_state_dict(synth.make_dense_weights(300, synth.DENSE))
        else:
            m = model(dtype, **kw)
        if switches:
            m.set_kernel_switches(**switches)
        if ep is not None:
            from switch_nerf_amd.parallel import ExpertParallel
            m.set_expert_parallel(ExpertParallel(0, 1, m.E, **ep))
        rays, img, rgbs = synth.make_rays(301, N)
        g = torch.Generator().manual_seed(302)
        pr, noise = torch.rand(N, S, generator=g).cuda(), torch.randn(N * S, generator=g).cuda()
        more = {}
        if fine:
            more = dict(fine_samples=fine, fine_u=torch.rand(N, fine, generator=g).cuda(), sigma_noise_fine=torch.randn(N * fine, generator=g).cuda())
        st = m.grad_step(dev(rgbs), dev(rays), dev(img), S, chunk, perturb=1.0, perturb_rand=pr, sigma_noise=noise, **more)
        return dict(raw=st["ctx"]["raw"], rgb=st["rgb"], loss=st["loss"], grad=m.grad)
    return run


def infer_no_batch():
    m = model(capacity_factor=0.75)
    rays, img, _ = synth.make_rays(301, 96)
    c = m.forward_rays(dev(rays), dev(img), 64, 2048, training=False, no_batch=True)
    return dict(raw=c["raw"], rgb=c["rgb"])


def moe_layer(k=1, residual=False):
    """MoELayer forward + backward, P = 2048 tokens (capacity 256 per expert at k = 1): y, dx and the parameter gradients."""
    def run():
        from switch_nerf_amd.moe import moe_layer as make
        cfg = synth.BUILDING
        M, E = cfg["model_dim"], cfg["num_experts"]
        torch.manual_seed(303)
        moe = make(gate_type=dict(type="top", k=k, capacity_factor=1.0, batch_prioritized_routing=True, gate_dim=M), model_dim=M,
                   experts=dict(type="expertmlp", count_per_node=E, hidden_size_per_expert=M, layer_num=cfg["expert_layers"],
                                skips=list(cfg["skips"])), seeds=(1, 1, 1), use_residual=residual, dtype=BF16).cuda()
        rng = np.random.default_rng(304)
        x = dev(rng.standard_normal((2048, M)).astype(np.float32)).requires_grad_(True)
        gi = dev(rng.standard_normal((2048, M)).astype(np.float32)).requires_grad_(True)
        y = moe(x, gate_input=gi)
        ((y * dev(rng.standard_normal((2048, M)).astype(np.float32))).sum() + y.l_aux).backward()
        return dict(y=y.detach(), dx=x.grad, dgate=gi.grad, param_grads=torch.cat([p.grad.reshape(-1) for p in moe.parameters()]))
    return run


CASES = {
    "fused": train(),
    "fused_tail_off": train(switches=dict(fused_tail=False)),
    "fused_tail_bwd_off": train(switches=dict(fused_tail_bwd=False)),
    "fp32": train(dtype=F32),
    "cf0_packed": train(capacity_factor=0.0),
    "cf050_drops": train(N=128, chunk=4096, capacity_factor=0.5),
    "ragged": train(N=80, chunk=4096),      # 5120 points: one chunk of 4096 and a last one of 1024
    "hierarchical": train(fine=64),
    "no_batch_inference": infer_no_batch,
    "ep_kept_rows": train(ep=dict()),
    "ep_padded": train(ep=dict(padded=True)),
    "ep_owner_tail": train(ep=dict(owner_tail=True)),
    "dense": train(dense=True, chunk=4096),
    "moe_top1": moe_layer(1),
    "moe_top2": moe_layer(2),
    "moe_residual": moe_layer(1, residual=True),
}


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append")
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--save")
    ap.add_argument("--against")
    a = ap.parse_args()
    if a.list:
        print(" ".join(CASES))
        return
    for name in a.case or list(CASES):
        runs = []
        for _ in range(2):
            out = CASES[name]()
            torch.cuda.synchronize()
            runs.append({k: v.detach().float().cpu().contiguous() for k, v in out.items()})
        line = {"case": name}
        for k, v in runs[0].items():
            same = torch.equal(v, runs[1][k])
            f = {"values": v.numel(), "sha256": hashlib.sha256(v.numpy().tobytes()).hexdigest(), "same": same}
            if not same:
                f["rel"] = rel(runs[1][k], v)
                if a.save:
                    os.makedirs(a.save, exist_ok=True)
                    np.save(os.path.join(a.save, f"{name}.{k}.npy"), v.numpy())
            ref = os.path.join(a.against, f"{name}.{k}.npy") if a.against else None
            if ref and os.path.exists(ref):
                f["vs"] = rel(v, torch.from_numpy(np.load(ref)))
            line[k] = f
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
