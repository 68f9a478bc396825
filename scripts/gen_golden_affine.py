"""Fixtures of the per-image affine colour transform (--affine_appearance, opts.py:55; models/nerf_moe.py:153-161, 426-438) from the
REFERENCE model's own run.

Usage (build container only, like oracle/gen_golden.py whose helpers it uses):
    python scripts/gen_golden_affine.py

Builds the reference NeRFMoE / MipNeRFMoE through model_utils.get_nerf with hparams.affine_appearance = True and layers.2.in_ch = M + 27,
loads tests/affine_weights.py's seeded weights, and writes under tests/golden/:
  model_fwd_affine.npz          NeRFMoE.forward on [P, 7] rows: outputs, moe_gates, the model's named_parameters() list and shapes
  render_train_affine.npz       the G5 recipe (64 rays x 64 samples, chunk 1024, fp32, cf 1.0, BPR, no perturbation): rgb / depth / sigma /
                                gate loss / loss / every parameter gradient (checksums + strided slices; embedding_a and affine in full)
  render_train_affine_mip.npz   the same through MipNeRFMoE (two levels of 64 intervals, like gen_mip)
The image indices (affine_weights.affine_image_indices) share images among rays and never hit image UNHIT_IMAGE.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden as gg  # noqa: E402
import synth  # noqa: E402      (on the path through gen_golden)
import affine_weights as aw  # noqa: E402
from switch_nerf.models import model_utils  # noqa: E402
from switch_nerf import rendering, rendering_mip  # noqa: E402

FULL = ("embedding_a.weight", "affine.weight", "affine.bias")      # small gradients stored whole


def reference_model(cfg, sd, **kw):
    h = gg.make_hparams(cfg, **kw)
    h.affine_appearance = True
    h.model["layers"]["2"]["in_ch"] = cfg["model_dim"] + 27
    torch.manual_seed(0)
    nerf = model_utils.get_nerf(h, cfg["appearance_count"])
    nerf.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    return nerf, h


def param_list(nerf):
    out = dict(names=np.array([n for n, _ in nerf.named_parameters()]))
    for n, p in nerf.named_parameters():
        out["pshape__" + n] = np.array(p.shape, np.int64)
    return out


def grads(nerf):
    out = {}
    for n, p in nerf.named_parameters():
        g_ = p.grad.numpy()
        out["gsum__" + n] = synth.checksum(g_)
        out["gslice__" + n] = g_.reshape(-1)[:: max(1, g_.size // 499)][:499]
        if n in FULL:
            out["gfull__" + n] = g_
    return out


def gen_model_forward():
    print("[affine] NeRFMoE.forward, P=4096")
    cfg, seed, P = synth.BUILDING, 141, 4096
    nerf, h = reference_model(cfg, aw.make_affine_weights(seed, cfg))
    rng = np.random.default_rng(seed + 1)
    img = aw.affine_image_indices(seed, P, cfg["appearance_count"])
    x = np.concatenate([rng.uniform(-1, 1, (P, 3)), rng.standard_normal((P, 3)), img[:, None]], 1).astype(np.float32)
    noise = rng.standard_normal((P, 1)).astype(np.float32)
    nerf.eval()
    with torch.no_grad():
        r = nerf(torch.from_numpy(x), sigma_noise=torch.from_numpy(noise))
    gg.save("model_fwd_affine", seed=seed, gate_scale=1.0, x=x, sigma_noise=noise, outputs=r["outputs"].numpy(),
            moe_loss=r["extras"]["moe_loss"].numpy(), moe_gates=r["extras"]["moe_gates"][0].numpy().astype(np.int32), **param_list(nerf))


def gen_render():
    print("[affine] render_rays / training step (64 rays x 64 samples, chunk 1024), fwd + grads")
    cfg, seed, gate_scale = synth.BUILDING, 151, 0.02
    N, S, chunk = 64, 64, 1024
    nerf, h = reference_model(cfg, aw.make_affine_weights(seed, cfg, gate_scale=gate_scale), coarse=S, chunk=chunk, perturb=0.0,
                              sigma_noise=False)
    rays, _, rgbs = synth.make_rays(seed + 1, N)
    img = aw.affine_image_indices(seed, N, cfg["appearance_count"])
    assert len(np.unique(img)) < N and aw.UNHIT_IMAGE not in img
    nerf.train()
    res, _ = rendering.render_rays(nerf, None, torch.from_numpy(rays), torch.from_numpy(img), h, None, None,
                                   get_depth=True, get_depth_variance=True, get_bg_fg_rgb=False)
    photo = torch.nn.functional.mse_loss(res["rgb_coarse"], torch.from_numpy(rgbs))
    loss = photo + 5e-4 * res["gate_loss_coarse"].mean()
    loss.backward()
    assert not nerf.embedding_a.weight.grad[aw.UNHIT_IMAGE].any()
    gg.save("render_train_affine", seed=seed, gate_scale=gate_scale, N=N, S=S, chunk=chunk, unhit_image=aw.UNHIT_IMAGE,
            rgb=res["rgb_coarse"].detach().numpy(), depth=res["depth_coarse"].numpy(), depth_variance=res["depth_variance_coarse"].numpy(),
            sigma=res["sigma_coarse"].detach().numpy(), gate_loss=res["gate_loss_coarse"].detach().numpy(),
            moe_gates=res["moe_gates_coarse"].numpy().astype(np.int32).reshape(N, S), loss=loss.detach().numpy(),
            photo=photo.detach().numpy(), **param_list(nerf), **grads(nerf))


def gen_render_mip():
    print("[affine] mip path: MipNeRFMoE, 2 levels of 64 intervals, loss = (fine + coarse) / 2, fwd + grads")
    cfg, seed, gate_scale = synth.BUILDING, 171, 0.02
    N, S, Fn, chunk = 64, 65, 65, 1024
    nerf, h = reference_model(cfg, aw.make_affine_weights(seed, cfg, gate_scale=gate_scale), coarse=S, chunk=chunk, perturb=0.0,
                              sigma_noise=False, fine=Fn, mip=True)
    rays, _, rgbs = synth.make_rays(seed + 1, N)
    img = aw.affine_image_indices(seed, N, cfg["appearance_count"])
    radii = (np.random.default_rng(seed + 2).uniform(0.5, 2.0, (N, 1)) * 1e-3).astype(np.float32)
    nerf.train()
    res, _ = rendering_mip.render_rays(nerf, torch.from_numpy(rays), torch.from_numpy(radii), torch.from_numpy(img), h,
                                       get_depth=True, get_depth_variance=True)
    t = torch.from_numpy(rgbs)
    photo = (torch.nn.functional.mse_loss(res["rgb_fine"], t) + torch.nn.functional.mse_loss(res["rgb_coarse"], t)) / 2
    loss = photo + 5e-4 * (res["gate_loss_fine"].mean() + res["gate_loss_coarse"].mean()) / 2.0
    loss.backward()
    assert not nerf.embedding_a.weight.grad[aw.UNHIT_IMAGE].any()
    gg.save("render_train_affine_mip", seed=seed, gate_scale=gate_scale, N=N, S=S, F=Fn, chunk=chunk, radii=radii,
            unhit_image=aw.UNHIT_IMAGE, rgb_coarse=res["rgb_coarse"].detach().numpy(), rgb_fine=res["rgb_fine"].detach().numpy(),
            depth=res["depth_fine"].numpy(), depth_variance=res["depth_variance_fine"].numpy(),
            gate_loss_coarse=res["gate_loss_coarse"].detach().numpy(), gate_loss_fine=res["gate_loss_fine"].detach().numpy(),
            moe_gates_coarse=res["moe_gates_coarse"].numpy().astype(np.int32).reshape(N, S - 1),
            moe_gates_fine=res["moe_gates_fine"].numpy().astype(np.int32).reshape(N, Fn - 1),
            loss=loss.detach().numpy(), photo=photo.detach().numpy(), **param_list(nerf), **grads(nerf))


if __name__ == "__main__":
    os.makedirs(gg.OUT, exist_ok=True)
    torch.set_num_threads(8)
    gen_model_forward()
    gen_render()
    gen_render_mip()
