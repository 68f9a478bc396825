"""Fixtures of the per-sample point outputs (return_pts / return_pts_rgb / return_pts_alpha / return_alpha with moe_return_gates,
rendering.py:299, :413-417, :443-452) from the REFERENCE's own render_rays in eval mode (perturb 0, no sigma noise).

Usage (build container only, like oracle/gen_golden.py whose recipes it calls):
    python scripts/gen_golden_points.py

Writes new tests/golden/*.npz files only:
  points_coarse   64 rays x 64 samples, chunk 1024 (the gen_render recipe, eval)
  points_fine     64 rays x (32 coarse + 64 fine), chunk 1024
  points_bg       the gen_bg scene (foreground MoE + 4-D background NeRF, ellipsoid bound), 96 rays x (64 + 64): rays with a background
  points_dense    the dense NeRF of gen_dense, 256 rays x 64 samples
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden as gg  # noqa: E402
import synth  # noqa: E402      (on the path through gen_golden)
from switch_nerf import rendering  # noqa: E402
from switch_nerf.models import model_utils  # noqa: E402

KEYS = ("pts", "pts_rgb", "pts_alpha", "alpha", "moe_gates", "sigma")


def _points_on(h):
    h.return_pts = h.return_pts_rgb = h.return_pts_alpha = h.return_alpha = True
    h.perturb, h.use_sigma_noise = 0.0, False


def _collect(res, out, typs, gates=True):
    for typ in typs:
        for k in KEYS:
            key = f"{k}_{typ}"
            if k == "moe_gates":
                if gates:
                    g = res[key].numpy().astype(np.int32)
                    out[key] = g.reshape(g.shape[0], g.shape[1])
                continue
            out[key] = res[key].detach().numpy().astype(np.float32)
    rt = "fine" if "rgb_fine" in res else "coarse"
    out["rgb"] = res[f"rgb_{rt}"].detach().numpy()


def gen_moe(tag, S, Fn, seed_w, seed_r, N=64, chunk=1024):
    print(f"[points] {tag}: {N} rays x ({S} + {Fn}) samples, chunk {chunk}, eval")
    cfg = synth.BUILDING
    sd = synth.make_weights(seed_w, cfg, gate_scale=0.02)
    nerf, h = gg.build_reference_model(cfg, sd, coarse=S, chunk=chunk, perturb=0.0, sigma_noise=False, fine=Fn)
    _points_on(h)
    rays, img, _ = synth.make_rays(seed_r, N)
    nerf.eval()
    with torch.no_grad():
        res, _ = rendering.render_rays(nerf, None, torch.from_numpy(rays), torch.from_numpy(img), h, None, None,
                                       get_depth=True, get_depth_variance=False, get_bg_fg_rgb=False)
    out = dict(seed=seed_w, rays_seed=seed_r, gate_scale=0.02, N=N, S=S, F=Fn, chunk=chunk)
    _collect(res, out, ("coarse", "fine") if Fn else ("coarse",))
    gg.save(f"points_{tag}", **out)


def gen_bg():
    print("[points] bg: the gen_bg scene, 96 rays x (64 + 64) samples, eval")
    cfg, cfg_bg = synth.BUILDING, synth.DENSE_BG
    center, radius = torch.from_numpy(synth.SPHERE_CENTER), torch.from_numpy(synth.SPHERE_RADIUS)
    sd = synth.make_weights(81, cfg, gate_scale=0.02)
    sd_bg = synth.make_dense_weights(82, cfg_bg)
    N, S, Fn, chunk = 96, 64, 64, 1024
    nerf, h = gg.build_reference_model(cfg, sd, coarse=S, chunk=chunk, perturb=0.0, sigma_noise=False, fine=Fn)
    _points_on(h)
    h.layers, h.skip_layers, h.bg_layer_dim = cfg_bg["layers"], list(cfg_bg["skip_layers"]), cfg_bg["layer_dim"]
    bg = model_utils.get_bg_nerf(h, cfg_bg["appearance_count"])
    bg.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd_bg.items()})
    rays, img, _ = synth.make_bg_rays(83, N)
    r = torch.from_numpy(rays)
    fg_far = torch.maximum(rendering._intersect_sphere(r[:, :3], r[:, 3:6], center, radius), r[:, 6])
    has_bg = (r[:, 7] > fg_far).numpy()
    assert 0 < has_bg.sum() < N
    nerf.eval()
    bg.eval()
    with torch.no_grad():
        res, present = rendering.render_rays(nerf, bg, r, torch.from_numpy(img), h, center, radius,
                                             get_depth=True, get_depth_variance=False, get_bg_fg_rgb=True)
    assert present
    out = dict(seed=81, seed_bg=82, rays_seed=83, gate_scale=0.02, N=N, S=S, F=Fn, chunk=chunk, has_bg=has_bg.astype(np.int32))
    _collect(res, out, ("coarse", "fine"))
    gg.save("points_bg", **out)


def gen_dense():
    print("[points] dense NeRF: 256 rays x 64 samples, eval")
    cfg = synth.DENSE
    sd = synth.make_dense_weights(161, cfg)
    h = gg.make_hparams(synth.BUILDING, coarse=64, chunk=65536, perturb=0.0)
    h.use_moe = False
    h.moe_return_gates = False
    h.layers, h.skip_layers, h.layer_dim = cfg["layers"], list(cfg["skip_layers"]), cfg["layer_dim"]
    _points_on(h)
    torch.manual_seed(0)
    nerf = model_utils.get_nerf(h, cfg["appearance_count"])
    nerf.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    N, S = 256, 64
    rays, img, _ = synth.make_rays(163, N)
    nerf.eval()
    with torch.no_grad():
        res, _ = rendering.render_rays(nerf, None, torch.from_numpy(rays), torch.from_numpy(img), h, None, None,
                                       get_depth=True, get_depth_variance=False, get_bg_fg_rgb=False)
    out = dict(seed=161, rays_seed=163, N=N, S=S, F=0, chunk=65536)
    _collect(res, out, ("coarse",), gates=False)
    gg.save("points_dense", **out)


if __name__ == "__main__":
    os.makedirs(gg.OUT, exist_ok=True)
    torch.set_num_threads(8)
    gen_moe("coarse", 64, 0, 51, 52)
    gen_moe("fine", 32, 64, 61, 62)
    gen_bg()
    gen_dense()
