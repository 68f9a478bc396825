"""Fixtures of the spherical-harmonics colour branch (--sh_deg) from the REFERENCE's own eval_sh (spherical_harmonics.py), its own NeRF
with rgb_dim = 3 (d + 1)^2 (models/nerf.py) and its own render_rays (rendering.py:317-349), on the CPU.

Usage (build container only, like oracle/gen_golden.py whose helpers it uses):
    python scripts/gen_golden_sh.py

Writes under tests/golden/ (data only: inputs, seeds, the reference's outputs and error figures):
  sh_eval.npz          eval_sh for deg 0..4 on 64 directions (the last 8 not of unit length) with random coefficients [64, 3, B]
  sh_dense_fwd.npz     NeRF(rgb_dim = 3 B).forward for deg 2 and 3 on 257 points: [P, 3 B + 1]; the seed of the state dict
                       (tests/sh_weights.make_sh_weights) and its checksum; fwd_err = max |fp32 - the same module in fp64|
  sh_dense_train.npz   render_rays + MSE + backward with sh_deg = 2, perturb = 0: coarse (128 rays x 32 samples) and hierarchical
                       (+ 16 fine samples), in the format of dense_nerf_train.npz (seed, outputs, gradient checksums and slices)
  sh_heads_bounds.npz  for every case of tests/sh_weights.head_cases(): max |fp32 - fp64| of the reference formulation of the heads
                       (F.linear + eval_sh + sigmoid, softplus; backward by autograd) per output - what the fp32 bounds of the
                       kernel-level tests are made of (8 x, the convention of profiles/r11_topk_gate_kernel_parity.md)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden as gg  # noqa: E402
import synth  # noqa: E402      (on the path through gen_golden)
import sh_weights as SW  # noqa: E402
from switch_nerf.models.nerf import NeRF, ShiftedSoftplus  # noqa: E402
from switch_nerf.spherical_harmonics import eval_sh  # noqa: E402
from switch_nerf import rendering  # noqa: E402


def gen_eval():
    print("[sh] eval_sh, deg 0..4, 64 directions")
    rng = np.random.default_rng(4001)
    d = rng.standard_normal((64, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[-8:] *= rng.uniform(0.3, 3.0, (8, 1))
    d = d.astype(np.float32)
    out = dict(dirs=d)
    for deg in range(5):
        coef = rng.standard_normal((64, 3, (deg + 1) ** 2)).astype(np.float32)
        out[f"coef_{deg}"] = coef
        out[f"out_{deg}"] = eval_sh(deg, torch.from_numpy(coef), torch.from_numpy(d)).numpy()
        out[f"out64_{deg}"] = eval_sh(deg, torch.from_numpy(coef).double(), torch.from_numpy(d).double()).numpy()
    gg.save("sh_eval", **out)


def reference_model(seed, deg, cfg=SW.SH_CFG, dtype=torch.float32):
    sd = SW.make_sh_weights(seed, deg, cfg)
    m = NeRF(cfg["pos_xyz_dim"], 0, cfg["layers"], list(cfg["skip_layers"]), cfg["layer_dim"], cfg["appearance_dim"], False,
             cfg["appearance_count"], 3 * (deg + 1) ** 2, cfg["xyz_dim"], ShiftedSoftplus())
    assert set(m.state_dict()) == set(sd), sorted(set(m.state_dict()) ^ set(sd))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    return sd, m.to(dtype)


def gen_fwd():
    print("[sh] NeRF(rgb_dim = 3 B).forward, deg 2 and 3, 257 points")
    P, cfg = 257, SW.SH_CFG
    rng = np.random.default_rng(4002)
    x = np.concatenate([rng.uniform(-1, 1, (P, 3)), rng.integers(0, cfg["appearance_count"], (P, 1))], 1).astype(np.float32)
    noise = rng.standard_normal((P, 1)).astype(np.float32)
    out = dict(x=x, sigma_noise=noise, **{"cfg__" + k: np.asarray(v, np.int64) for k, v in cfg.items()})
    for deg in (2, 3):
        seed = 4010 + deg
        sd, m = reference_model(seed, deg)
        _, m64 = reference_model(seed, deg, dtype=torch.float64)
        with torch.no_grad():
            o = m.eval()(torch.from_numpy(x), sigma_noise=torch.from_numpy(noise))
            o64 = m64.eval()(torch.from_numpy(x).double(), sigma_noise=torch.from_numpy(noise).double())
            s = m(torch.from_numpy(x[:, :3]), sigma_only=True)
        err = float((o.double() - o64).abs().max())
        print(f"  deg {deg}: out {tuple(o.shape)}, fp32 against fp64 {err:.3e}")
        out.update({f"seed_{deg}": seed, f"out_{deg}": o.numpy(), f"sigma_only_{deg}": s.numpy(), f"fwd_err_{deg}": err,
                    f"sd_checksum_{deg}": np.sum([synth.checksum(v) for v in sd.values()], 0)})
    gg.save("sh_dense_fwd", **out)


def gen_train():
    print("[sh] render_rays + mse + backward, sh_deg 2, perturb 0: coarse and hierarchical")
    deg, seed, N, S, Fn, cfg = 2, 4020, 128, 32, 16, SW.SH_CFG
    rays, img, rgbs = synth.make_rays(4021, N, cfg["appearance_count"])
    out = dict(seed=seed, deg=deg, N=N, S=S, F=Fn, rays_seed=4021)
    for tag, fine in (("coarse", 0), ("fine", Fn)):
        sd, nerf = reference_model(seed, deg)
        h = gg.make_hparams(synth.BUILDING, coarse=S, chunk=1000, perturb=0.0, fine=fine)      # (a ragged last model chunk)
        h.use_moe, h.pos_dir_dim, h.appearance_dim, h.sh_deg, h.moe_return_gates = False, 0, cfg["appearance_dim"], deg, False
        nerf.train()
        res, _ = rendering.render_rays(nerf, None, torch.from_numpy(rays), torch.from_numpy(img), h, None, None, get_depth=True,
                                       get_depth_variance=True, get_bg_fg_rgb=False)
        loss = torch.nn.functional.mse_loss(res[f"rgb_{tag}"], torch.from_numpy(rgbs))
        loss.backward()
        out.update({f"rgb_{tag}": res[f"rgb_{tag}"].detach().numpy(), f"depth_{tag}": res[f"depth_{tag}"].detach().numpy(),
                    f"sigma_head_{tag}": res["sigma_coarse"].detach().numpy()[:64], f"loss_{tag}": loss.detach().numpy()})
        for n, p in nerf.named_parameters():
            g_ = p.grad
            out[f"gsum_{tag}__" + n] = synth.checksum(g_.numpy())
            out[f"gslice_{tag}__" + n] = g_.numpy().reshape(-1)[:: max(1, g_.numel() // 499)][:499]
        print(f"  {tag}: loss {float(loss):.6f}")
    gg.save("sh_dense_train", **out)


def reference_heads(c, deg, rpg, dtype):
    """The reference formulation of the heads on one case: F.linear heads, eval_sh against the row's direction, sigmoid; softplus(x - 1).
    h2 is the ReLU of a leaf, so that its gradient carries the mask the kernel's dh2 carries."""
    t = {k: (None if v is None else torch.from_numpy(v).to(dtype)) for k, v in c.items()}
    B = (deg + 1) ** 2
    pre = t["h2"].clone().requires_grad_(True)
    pre.data[t["h2"] == 0] = -1.0                       # (the zeros of h2 came from negative pre-activations)
    h2 = torch.relu(pre)
    leaves = {k: t[k].clone().requires_grad_(True) for k in ("ws", "bs", "wc", "bc")}
    y = t["y"]
    lin = torch.nn.functional.linear(h2, leaves["wc"], leaves["bc"])
    dirs = t["dirs"].repeat_interleave(rpg, 0)
    rgb = torch.sigmoid(eval_sh(deg, lin.view(-1, 3, B), dirs))
    u = y @ leaves["ws"] + leaves["bs"]
    if t["noise"] is not None:
        u = u + t["noise"]
    u.retain_grad()
    sigma = ShiftedSoftplus()(u)
    raw = torch.cat([rgb, sigma[:, None]], 1)
    raw.backward(t["d_raw"])
    P = y.shape[0]
    return dict(rgb=rgb.detach(), sigma=sigma.detach(), coef=lin.detach(), dh2=pre.grad, dsig=u.grad, d_ws=leaves["ws"].grad,
                d_bs=leaves["bs"].grad, d_wc=leaves["wc"].grad, d_bc=leaves["bc"].grad,
                colsum=pre.grad.view(P // rpg, rpg, -1).sum(1))


def gen_heads_bounds():
    print("[sh] the reference formulation of the heads, fp32 against fp64, on the kernel tests' cases")
    out, names = {}, ("rgb", "sigma", "coef", "dh2", "dsig", "d_ws", "d_bs", "d_wc", "d_bc", "colsum")
    for case in SW.head_cases():
        deg, N, S, rpg, noise = case
        c = SW.head_case(*case)
        a, b = reference_heads(c, deg, rpg, torch.float32), reference_heads(c, deg, rpg, torch.float64)
        # an error of zero (one row, one term) would leave no room for another summation order: floor at one rounding of the result
        err = [max(float((a[k].double() - b[k]).abs().max()), float(b[k].abs().max()) * 2.0 ** -24) for k in names]
        out[SW.case_key(*case)] = np.asarray(err)
    out["names"] = np.array(names)
    worst = np.max(np.stack([v for k, v in out.items() if k != "names"]), 0)
    print("  worst per output: " + ", ".join(f"{n} {e:.2e}" for n, e in zip(names, worst)))
    gg.save("sh_heads_bounds", **out)


if __name__ == "__main__":
    os.makedirs(gg.OUT, exist_ok=True)
    torch.set_num_threads(8)
    gen_eval()
    gen_fwd()
    gen_train()
    gen_heads_bounds()
