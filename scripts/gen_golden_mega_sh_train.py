"""Fixtures of TRAINING a Mega-NeRF whose cells use spherical-harmonics colour (switch_nerf_amd/mega.py, joint_training + sh_training) from
the REFERENCE's own MegaNeRF(.., True).train() around its own NeRF(rgb_dim = 3 B) sub-models (what --train_mega_nerf with --sh_deg
builds, models/model_utils.py:118-123), its own eval_sh + sigmoid (rendering.py:344-349), its own render_rays, autograd and
torch.optim.Adam, on the CPU.

Usage (build container only, like scripts/gen_golden_mega_train.py and scripts/gen_golden_mega_sh.py whose helpers it uses):
    python scripts/gen_golden_mega_sh_train.py

Writes under tests/golden/, data only (seeds, inputs, checksums of the state dicts, results, gradient checksums and 499-element slices;
the weights are tests/sh_weights.make_sh_weights(seed + i, deg, cfg) and are never stored):
  mega_sh_train.npz   render level, sh_deg 2, boundary_margin 1, the 3 cells of gen_golden_mega_sh's cfg (seed 511), 64 rays x 32 samples,
                      hparams.sh_deg = 2, in the layout of mega_train.npz:
                        a_*  coarse only; b_*  with 16 fine samples; c_*  two Adam steps (lr 5e-4), the second on rays whose every
                        sample lies in cell 0 (cells 1 and 2: a ZERO gradient, not a missing one)
  mega_sh_train_module_d{0,2,4}.npz   module level: P = 256 points (128 at degree 4) x [P, 3 + 1], one direction per point, sigma noise and
                      a stored d_raw [P, 4] applied to raw = cat(sigmoid(eval_sh(module output, dirs)), sigma): raw_<tag> and the
                      gradients' checksums / slices packed as in mega_train_module.npz (<tag>_gsums, <tag>_gslices, offsets).  Degree 2 at
                      margins 1 (m100) and 1.15 (m115), degrees 0 and 4 at 1.15.
A condition, not a measurement: no point any model call receives (the fine samples included) lies within 4 x the reference's own distance
error of a membership decision (gen_golden_mega_train.on_a_decision); the seed is advanced until the count is zero, and the count is
asserted.  One flipped membership changes every gradient, so nothing is excluded.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)
import gen_golden as gg  # noqa: E402
import synth  # noqa: E402      (on the path through gen_golden)
import gen_golden_mega_sh as GS  # noqa: E402
import gen_golden_mega_train as GT  # noqa: E402
from switch_nerf.models.mega_nerf import MegaNeRF  # noqa: E402
from switch_nerf.spherical_harmonics import eval_sh  # noqa: E402
from switch_nerf import rendering  # noqa: E402

CFG, CENTROIDS = GS.CFG, GS.CENTROIDS
assert np.array_equal(CENTROIDS, GT.CENTROIDS)          # (on_a_decision measures against these)
N, S, FINE, LR, DEG = 64, 32, 16, 5e-4, 2
MODULE_CASES = {0: (("m115", 1.15),), 2: (("m100", 1.0), ("m115", 1.15)), 4: (("m115", 1.15),)}
LIMIT = os.path.getsize(os.path.join(gg.OUT, "mega_fg.npz"))


def fresh_mega(seed, deg, margin):
    sds, subs = GS.reference_subs(seed, deg, CFG)
    return sds, MegaNeRF(subs, torch.from_numpy(CENTROIDS), margin, False, False, True).train()


def hparams(fine):
    h = gg.make_hparams(synth.BUILDING, coarse=S, chunk=65536, perturb=0.0, fine=fine)
    h.use_moe, h.pos_dir_dim, h.appearance_dim, h.sh_deg, h.return_sigma, h.moe_return_gates = False, 0, CFG["appearance_dim"], DEG, False, False
    return h


def render(mega, rays, img, rgbs, fine):
    seen = []
    hook = mega.register_forward_pre_hook(lambda mod, args: seen.append(args[0].detach().numpy().copy()))
    res, _ = rendering.render_rays(mega, None, torch.from_numpy(rays), torch.from_numpy(img), hparams(fine), None, None, get_depth=True,
                                   get_depth_variance=True, get_bg_fg_rgb=False)
    hook.remove()
    assert all(a.shape[1] == 4 for a in seen)            # (no direction columns: rendering.py:320-323)
    typ = "fine" if fine else "coarse"
    return res[f"rgb_{typ}"], res[f"depth_{typ}"], torch.nn.functional.mse_loss(res[f"rgb_{typ}"], torch.from_numpy(rgbs)), seen


def gen_render_level(seed, out):
    ray_seed = 741
    while True:
        rays, img, rgbs = synth.make_rays(ray_seed, N, CFG["appearance_count"])
        rays2 = GT.cell0_rays(rays, ray_seed + 1)
        sds, mega = fresh_mega(seed, DEG, 1)
        cases, bad = {}, 0
        for tag, fine in (("a_", 0), ("b_", FINE)):
            mega.zero_grad()
            rgb, depth, loss, seen = render(mega, rays, img, rgbs, fine)
            n_bad, err = GT.on_a_decision(np.concatenate(seen), 1.0)
            bad += n_bad
            loss.backward()
            c = {tag + "rgb": rgb.detach().numpy(), tag + "depth": depth.detach().numpy(), tag + "loss": loss.detach().numpy(),
                 tag + "dist_err": err, tag + "members": np.array([GT.members(s) for s in seen])}
            if fine:
                c[tag + "pts_fine"] = seen[1][:, :3]
            GT.grads(mega, tag, c)
            cases.update(c)
            print(f"  ({tag[0]}) ray seed {ray_seed}: loss {loss.item():.6f}, members {c[tag + 'members'].tolist()}, on a decision {n_bad} "
                  f"(dist_err {err:.3e})")
        _, mega = fresh_mega(seed, DEG, 1)
        opt = torch.optim.Adam(mega.parameters(), lr=LR)
        c = {}
        for step, r in ((1, rays), (2, rays2)):
            opt.zero_grad()
            _, _, loss, seen = render(mega, r, img, rgbs, 0)
            n_bad, _ = GT.on_a_decision(np.concatenate(seen), 1.0)
            bad += n_bad
            loss.backward()
            m = GT.members(np.concatenate(seen))
            if step == 1:
                for n, p in mega.named_parameters():
                    assert np.array_equal(GT.sl(p.grad.numpy()), cases["a_gslice__" + n]), n
            else:
                assert m[1] == 0 and m[2] == 0 and m[0] == N * S, m
                for n, p in mega.named_parameters():          # the empty cells: a zero gradient, not a missing one (mega_nerf.py:51-59)
                    if not n.startswith("sub_modules.0."):
                        assert p.grad is not None and not p.grad.any(), n
            opt.step()
            GT.params(mega, f"c_p{step}_", c)
            c[f"c_loss{step}"] = loss.detach().numpy()
            print(f"  (c) step {step}: loss {loss.item():.6f}, members {m}, on a decision {n_bad}")
        if bad == 0:
            break
        ray_seed += 10
        print(f"  -> {bad} points on a membership decision: next ray seed {ray_seed}")
    assert bad == 0
    out.update(cases)
    out.update(c)
    out["param_names"] = np.array([n for n, _ in mega.named_parameters()])
    out.update(ray_seed=ray_seed, rays=rays, image_indices=img, rgbs=rgbs, rays_cell0=rays2, N=N, S=S, F=FINE, lr=LR, deg=DEG)
    return sds


def gen_module_level(deg):
    P, seed, B = (128 if deg == 4 else 256), GS.SEED_FG[deg], (deg + 1) ** 2
    pt_seed = seed + 70
    while True:
        rng = np.random.default_rng(pt_seed)
        x = np.concatenate([rng.uniform(-1, 1, (P, 3)), rng.integers(0, CFG["appearance_count"], (P, 1))], 1).astype(np.float32)
        dirs = (GS.unit(rng, P) * rng.uniform(0.8, 1.25, (P, 1))).astype(np.float32)      # (used as given: not all of unit length)
        noise = rng.standard_normal((P, 1)).astype(np.float32)
        d_raw = rng.standard_normal((P, 4)).astype(np.float32)
        bad = sum(GT.on_a_decision(x, margin)[0] for _, margin in MODULE_CASES[deg])
        if bad == 0:
            break
        pt_seed += 10
        print(f"  -> degree {deg}: {bad} points on a membership decision: next point seed {pt_seed}")
    assert bad == 0
    out = dict(seed=seed, point_seed=pt_seed, deg=deg, x=x, dirs=dirs, sigma_noise=noise, d_raw=d_raw, centroids=CENTROIDS)
    for tag, margin in MODULE_CASES[deg]:
        sds, mega = fresh_mega(seed, deg, margin)
        res = mega(torch.from_numpy(x), sigma_noise=torch.from_numpy(noise))
        assert res.shape == (P, 3 * B + 1)
        raw = torch.cat([torch.sigmoid(eval_sh(deg, res[:, :3 * B].view(-1, 3, B), torch.from_numpy(dirs))), res[:, 3 * B:]], -1)
        raw.backward(torch.from_numpy(d_raw))
        named = [(n, p.grad.numpy()) for n, p in mega.named_parameters()]
        out["param_names"] = np.array([n for n, _ in named])
        out["raw_" + tag] = raw.detach().numpy()
        out[tag + "_gsums"], out[tag + "_gslices"], out["offsets"] = GT.packed(named)
        out[tag + "_dist_err"] = GT.on_a_decision(x, margin)[1]
        print(f"  module level d{deg} {tag}: raw {tuple(raw.shape)}, members {GT.members(x)}")
    out.update(GS.cfg_arrays(CFG, sds))
    save(f"mega_sh_train_module_d{deg}", out)


def save(name, out):
    gg.save(name, **out)
    assert os.path.getsize(os.path.join(gg.OUT, name + ".npz")) < LIMIT, "a fixture file stays below the size of mega_fg.npz"


if __name__ == "__main__":
    os.makedirs(gg.OUT, exist_ok=True)
    torch.set_num_threads(8)
    seed = GS.SEED_FG[DEG]
    print(f"[mega sh train] 3 cells, sh_deg {DEG} (seed {seed}), margin 1: {N} rays x {S} samples, + {FINE} fine, two Adam steps")
    out = dict(seed=seed, centroids=CENTROIDS, margin=1.0)
    sds = gen_render_level(seed, out)
    out.update(GS.cfg_arrays(CFG, sds))
    save("mega_sh_train", out)
    for deg in (0, 2, 4):
        gen_module_level(deg)
