"""Fixture of gradient accumulation (SwitchNeRF.set_accumulation) from the REFERENCE's own models, its rendering.render_rays, its
autograd and torch.optim.Adam, on the CPU: the loop of runner.py:646-690 (loss / accumulation_steps, backward adding into .grad,
optimizer step and zero_grad on every accumulation_steps-th iteration), in fp32, perturb 0, no noise.

Usage (build container only, like oracle/gen_golden.py whose helpers it uses):
    python scripts/gen_golden_accum.py

Writes tests/golden/accum_train.npz, data only.  Weights are never stored: the MoE model is synth.make_weights(SEED_MOE) on
synth.BUILDING (the cfg of gen_render), the dense one synth.make_dense_weights(SEED_DENSE) on synth.DENSE; the file holds their checksums.
Micro-batch i of every case is synth.make_rays(RAY_SEED + i, 64), stored as <model>_mb<i>_rays / _image_indices / _rgbs: 64 rays x 32
samples, MoE chunk 1024 (2 chunks).  Cases, keyed
<model>_a<A>_ with model in (moe, dense):  A = 2: 4 micro-batches = 2 optimizer steps;  A = 3: 3 micro-batches = 1 step.  Per case:
    m<i>_loss                 the micro-loss as the reference reports it (undivided): mse + 5e-4 * mean gate loss (MoE), mse (dense)
    m<i>_moe_gates [N, S]     MoE: the experts chosen (int8)
    m<i>_gslice__             the gradient of that micro-batch's DIVIDED loss (loss / A), thinned slices
    s<j>_gsum__ / s<j>_gslice__   the accumulated gradient (.grad) before optimizer step j (checksums [P, 3]; thinned slices)
    s<j>_psum__ / s<j>_pslice__   the parameter after step j of torch.optim.Adam(lr 5e-4)
The gsum__ / gslice__ data of render_train_*.npz with the P parameters of a model packed into one array each, in the order of
<model>_param_names: the slices end to end, parameter i at [<model>_offsets[i], <model>_offsets[i + 1]) (<model>_micro_offsets for m<i>).
Slices: every max(1, numel // 499)-th element, at most 499 (the format of render_train_*.npz), thinned for the file's size to every
EVERY-th position of those (`every`, stored); the micro-gradient slices to every EVERY_MICRO-th (`every_micro`, a multiple of EVERY).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden as gg  # noqa: E402
import synth  # noqa: E402      (on the path through gen_golden)
from switch_nerf.models import model_utils  # noqa: E402
from switch_nerf import rendering  # noqa: E402

N, S, CHUNK = 64, 32, 1024
SEED_MOE, SEED_DENSE, RAY_SEED, LR, WT, N_SLICE, EVERY, EVERY_MICRO = 51, 161, 310, 5e-4, 5e-4, 499, 6, 18
CASES = ((2, 4), (3, 3))          # (accumulation steps, micro-batches)


def sl(a):
    a = np.asarray(a).reshape(-1)
    return a[:: max(1, a.size // N_SLICE)][:N_SLICE].copy()


def pack(parts):
    """The parameters' slices end to end, in the order of <model>_param_names -> (packed, offsets [P + 1])."""
    return np.concatenate(parts), np.cumsum([0] + [len(q) for q in parts]).astype(np.int64)


def build(kind):
    if kind == "moe":
        sd = synth.make_weights(SEED_MOE, synth.BUILDING, gate_scale=1.0)
        nerf, h = gg.build_reference_model(synth.BUILDING, sd, coarse=S, chunk=CHUNK, perturb=0.0, sigma_noise=False)
        return nerf, h, sd, synth.BUILDING["appearance_count"]
    cfg = synth.DENSE
    sd = synth.make_dense_weights(SEED_DENSE, cfg)
    h = gg.make_hparams(synth.BUILDING, coarse=S, chunk=65536, perturb=0.0)
    h.use_moe = False
    h.layers, h.skip_layers, h.layer_dim = cfg["layers"], list(cfg["skip_layers"]), cfg["layer_dim"]
    torch.manual_seed(0)
    nerf = model_utils.get_nerf(h, cfg["appearance_count"])
    assert set(nerf.state_dict()) == set(sd), sorted(set(nerf.state_dict()) ^ set(sd))
    nerf.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    return nerf, h, sd, cfg["appearance_count"]


def gen_case(kind, A, n_micro, out):
    tag = f"{kind}_a{A}_"
    nerf, h, sd, n_img = build(kind)
    nerf.train()
    params = [p for _, p in nerf.named_parameters()]
    names = [n for n, _ in nerf.named_parameters()]
    opt = torch.optim.Adam(nerf.parameters(), lr=LR)
    opt.zero_grad(set_to_none=True)
    step = 0
    for it in range(n_micro):
        should_accumulate = (it + 1) % A != 0                                # runner.py:589
        rays, img, rgbs = synth.make_rays(RAY_SEED + it, N, n_img)
        out[f"{kind}_mb{it}_rays"], out[f"{kind}_mb{it}_image_indices"], out[f"{kind}_mb{it}_rgbs"] = rays, img, rgbs
        res, _ = rendering.render_rays(nerf, None, torch.from_numpy(rays), torch.from_numpy(img), h, None, None, get_depth=True,
                                       get_depth_variance=True, get_bg_fg_rgb=False)
        loss = torch.nn.functional.mse_loss(res["rgb_coarse"], torch.from_numpy(rgbs))
        if kind == "moe":
            loss = loss + WT * res["gate_loss_coarse"].mean()                # :646-651
            out[tag + f"m{it}_moe_gates"] = res["moe_gates_coarse"].numpy().astype(np.int8).reshape(N, S)
        all_loss = loss / A                                                  # :657
        micro = torch.autograd.grad(all_loss, params, retain_graph=True)
        all_loss.backward()                                                  # :679 (adds into .grad)
        out[tag + f"m{it}_loss"] = loss.detach().numpy()
        out[tag + f"m{it}_gslice__"], out[kind + "_micro_offsets"] = pack([sl(g_.numpy())[::EVERY_MICRO] for g_ in micro])
        print(f"  {tag} micro {it}: loss {loss.item():.6f}  accumulate {should_accumulate}")
        if not should_accumulate:
            out[tag + f"s{step}_gsum__"] = np.stack([synth.checksum(p.grad.numpy()) for p in params])
            out[tag + f"s{step}_gslice__"], out[kind + "_offsets"] = pack([sl(p.grad.numpy())[::EVERY] for p in params])
            opt.step()                                                       # :681-686
            opt.zero_grad(set_to_none=True)                                  # :689-690
            out[tag + f"s{step}_psum__"] = np.stack([synth.checksum(p.detach().numpy()) for p in params])
            out[tag + f"s{step}_pslice__"], _ = pack([sl(p.detach().numpy())[::EVERY] for p in params])
            step += 1
    assert step == n_micro // A
    out[kind + "_param_names"] = np.array(names)
    out[kind + "_sd_checksums"] = np.stack([synth.checksum(v) for v in sd.values()])


def main():
    out = dict(N=N, S=S, chunk=CHUNK, seed_moe=SEED_MOE, seed_dense=SEED_DENSE, ray_seed=RAY_SEED, lr=LR, wt=WT, every=EVERY, every_micro=EVERY_MICRO,
               cases=np.array(CASES))
    for kind in ("moe", "dense"):
        for A, n_micro in CASES:
            gen_case(kind, A, n_micro, out)
    gg.save("accum_train", **out)


if __name__ == "__main__":
    os.makedirs(gg.OUT, exist_ok=True)
    torch.set_num_threads(8)
    print(f"[accum] {N} rays x {S} samples per micro-batch; (A, micro-batches) = {CASES}; MoE and dense")
    main()
