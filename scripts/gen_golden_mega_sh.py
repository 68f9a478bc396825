"""Fixtures of the Mega-NeRF spatial-cell model with spherical-harmonics sub-models (switch_nerf_amd/mega.py with DenseNeRF cfg["sh_deg"])
from the REFERENCE's own MegaNeRF (models/mega_nerf.py) around its own NeRF(rgb_dim = 3 B) sub-models (models/nerf.py), its own eval_sh
(spherical_harmonics.py) + sigmoid (rendering.py:344-349) and its own render_rays, on the CPU.

Usage (build container only, like scripts/gen_golden_mega.py whose layout it follows):
    python scripts/gen_golden_mega_sh.py

Writes under tests/golden/ (data only: inputs, centroids, seeds and checksums of the state dicts, the reference's results, error figures):
  mega_sh_fg_d0.npz / _d2.npz / _d4.npz   3 foreground cells, sh_deg 0 / 2 / 4 (d2 with cluster_2d), boundary_margin 1 (m100) and 1.15
                    (m115): x [P, 3 + 1], one direction per point, the reference's weights, its packed per-cell outputs, forward
                    [P, 3 B + 1] with sigma noise, sigma_only [P, 1], and raw [P, 4] = (sigmoid(eval_sh(forward, dirs)), sigma).  P is
                    256 (128 for d4) so that a file stays below the size of mega_fg.npz
  mega_sh_bg.npz    the xyz_real background variant (xyz_dim 4, x [P, 3 + 4 + 1]), cluster_2d, boundary_margin 1.15, sh_deg 2; its
                    per-cell outputs are the reference NeRF's forward on inverted-sphere points
  mega_sh_render.npz  rendering.render_rays with hparams.sh_deg = 2 and both models of a container behind an ellipsoidal bound (the
                    sub-models of mega_sh_fg_d2 / mega_sh_bg, centroids inside the bound): 64 rays x 32 (16 background) samples coarse,
                    and with 32 (16) fine samples and cluster_2d
Error figures (none comes from the code under test):
  excluded_*     a point is excluded only when the membership the reference found (float32, torch.cdist) differs from the membership of
                 a float64 evaluation of the direct distances of the same inputs; asserted here to be at most 1 % in every fixture
  blend_sh_tol   4 x max |reference float32 pipeline (its blend of its per-cell outputs, its eval_sh + sigmoid) - the float64 evaluation
                 of the same formula (tests/mega_sh_restate.blend_sh on the float64 weights and the same per-cell outputs)| over rgb
                 and sigma, both margins, the points that are not excluded: the rule of weights_tol / blend_tol of mega_fg.npz
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
import mega_restate as R  # noqa: E402
import mega_sh_restate as RS  # noqa: E402
from switch_nerf.models.mega_nerf import MegaNeRF  # noqa: E402
from switch_nerf.models.nerf import NeRF, ShiftedSoftplus  # noqa: E402
from switch_nerf.spherical_harmonics import eval_sh  # noqa: E402
from switch_nerf import rendering  # noqa: E402

CFG = dict(layer_dim=256, layers=2, skip_layers=(1,), pos_xyz_dim=3, pos_dir_dim=0, appearance_dim=8, appearance_count=4, xyz_dim=3)
CENTROIDS = np.array([[-0.5, -0.4, 0.1], [0.5, -0.3, -0.2], [0.0, 0.5, 0.3]], np.float32)      # those of scripts/gen_golden_mega.py
SEED_FG = {0: 501, 2: 511, 4: 521}
SEED_BG = 531


def reference_subs(seed, deg, cfg):
    sds, subs = [], []
    for i in range(len(CENTROIDS)):
        sd = SW.make_sh_weights(seed + i, deg, cfg)
        m = NeRF(cfg["pos_xyz_dim"], 0, cfg["layers"], list(cfg["skip_layers"]), cfg["layer_dim"], cfg["appearance_dim"], False,
                 cfg["appearance_count"], 3 * (deg + 1) ** 2, cfg["xyz_dim"], ShiftedSoftplus())
        assert set(m.state_dict()) == set(sd)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
        sds.append(sd)
        subs.append(m.eval())
    return sds, subs


def cfg_arrays(cfg, sds):
    out = {"cfg__" + k: np.asarray(v, np.int64) for k, v in cfg.items()}
    out["sd_checksums"] = np.stack([np.sum([synth.checksum(v) for v in sd.values()], 0) for sd in sds])
    return out


def reference_weights(mega, xt, dim_start, margin):
    """mega_nerf.py:21-30, the reference's own operations."""
    d = torch.cdist(xt[:, dim_start:3], mega.centroids[:, dim_start:])
    if margin > 1:
        inv = 1 / (d + 1e-8)
        inv[d > margin * d.min(dim=1)[0].unsqueeze(-1).repeat(1, d.shape[1])] = 0
        return inv / inv.sum(dim=-1).unsqueeze(-1)
    return torch.nn.functional.one_hot(d.argmin(dim=1), d.shape[1]).float()


def one_margin(tag, mega, x, dirs, noise, dim_start, margin, xyz_real, deg):
    xt, nt, dt = torch.from_numpy(x), torch.from_numpy(noise), torch.from_numpy(dirs)
    mega.boundary_margin = margin
    col0, xd, B = (3, 4, (deg + 1) ** 2) if xyz_real else (0, 3, (deg + 1) ** 2)
    with torch.no_grad():
        out = mega(xt, sigma_noise=nt)
        sig = mega(xt[:, :col0 + xd], sigma_only=True, sigma_noise=nt)
        w = reference_weights(mega, xt, dim_start, margin)
        sub = torch.cat([child(xt[w[:, i] > 0][:, col0:], False, nt[w[:, i] > 0]) for i, child in enumerate(mega.sub_modules)
                         if (w[:, i] > 0).any()], 0)
        raw = torch.cat([torch.sigmoid(eval_sh(deg, out[:, :3 * B].view(-1, 3, B), dt)), out[:, 3 * B:]], -1)      # rendering.py:344-349
    assert out.shape == (len(x), 3 * B + 1)
    w64 = R.assign(x, CENTROIDS, dim_start, margin, torch.float64)
    excluded = ((w64 > 0) != (w > 0)).any(1).numpy()
    keep = ~excluded
    _, begin, _, slot = R.pack(w)
    assert torch.equal(R.blend(w, slot, begin, sub, margin == 1), out), "the packed per-cell outputs do not reproduce the reference's output"
    w64 = w64.numpy()
    w64[excluded] = w.double().numpy()[excluded]          # (so that both packings line up; not measured there)
    raw64, _ = RS.blend_sh(w64, slot, begin, sub.numpy(), dirs, 1, deg, margin == 1)
    err = np.abs(raw.double().numpy() - raw64)[keep]
    e_rgb, e_sig = float(err[:, :3].max()), float(err[:, 3].max())
    print(f"  {tag}: excluded {int(excluded.sum())} / {len(x)}, rgb err {e_rgb:.3e}, sigma err {e_sig:.3e}, members {(w > 0).sum(0).tolist()}")
    assert excluded.mean() <= 0.01
    return {f"weights_{tag}": w.numpy(), f"out_{tag}": out.numpy(), f"raw_{tag}": raw.numpy(), f"sigma_{tag}": sig.numpy(),
            f"sub_{tag}": sub.numpy(), f"excluded_{tag}": excluded, f"rgb_err_{tag}": e_rgb, f"sigma_err_{tag}": e_sig}


def unit(rng, n):
    d = rng.standard_normal((n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def finish(name, out, tags):
    out["blend_sh_tol"] = 4 * max(max(out[f"rgb_err_{t}"], out[f"sigma_err_{t}"]) for t in tags)
    print(f"  blend_sh_tol {out['blend_sh_tol']:.3e}")
    gg.save(name, **out)
    assert os.path.getsize(os.path.join(gg.OUT, name + ".npz")) <= 200 * 1024


def gen_fg(deg):
    P, c2d = (128 if deg == 4 else 256), deg == 2
    print(f"[mega sh] foreground: 3 cells, sh_deg {deg}, margins 1 and 1.15, cluster_2d {c2d}, {P} points")
    seed = SEED_FG[deg]
    sds, subs = reference_subs(seed, deg, CFG)
    rng = np.random.default_rng(seed + 50)
    x = np.concatenate([rng.uniform(-1, 1, (P, 3)), rng.integers(0, CFG["appearance_count"], (P, 1))], 1).astype(np.float32)
    dirs = (unit(rng, P) * rng.uniform(0.8, 1.25, (P, 1))).astype(np.float32)      # (used as given: not all of unit length)
    noise = rng.standard_normal((P, 1)).astype(np.float32)
    mega = MegaNeRF(subs, torch.from_numpy(CENTROIDS), 1.15, False, c2d).eval()
    out = dict(seed=seed, deg=deg, x=x, dirs=dirs, sigma_noise=noise, centroids=CENTROIDS, cluster_2d=int(c2d), xyz_real=0,
               **cfg_arrays(CFG, sds))
    for tag, margin in (("m100", 1.0), ("m115", 1.15)):
        out.update(one_margin(tag, mega, x, dirs, noise, 1 if c2d else 0, margin, False, deg))
    finish(f"mega_sh_fg_d{deg}", out, ("m100", "m115"))
    return subs


def gen_bg():
    P, deg = 256, 2
    print(f"[mega sh] background: xyz_real, cluster_2d, margin 1.15, sh_deg {deg}, {P} points")
    cfg = dict(CFG, xyz_dim=4)
    sds, subs = reference_subs(SEED_BG, deg, cfg)
    rng = np.random.default_rng(SEED_BG + 50)
    x = np.concatenate([rng.uniform(-1, 1, (P, 3)), unit(rng, P), rng.uniform(0, 1, (P, 1)),
                        rng.integers(0, cfg["appearance_count"], (P, 1))], 1).astype(np.float32)
    dirs = unit(rng, P).astype(np.float32)
    noise = rng.standard_normal((P, 1)).astype(np.float32)
    mega = MegaNeRF(subs, torch.from_numpy(CENTROIDS), 1.15, True, True).eval()
    out = dict(seed=SEED_BG, deg=deg, x=x, dirs=dirs, sigma_noise=noise, centroids=CENTROIDS, cluster_2d=1, xyz_real=1, **cfg_arrays(cfg, sds))
    out.update(one_margin("m115", mega, x, dirs, noise, 1, 1.15, True, deg))
    finish("mega_sh_bg", out, ("m115",))
    return subs


def membership_differs(x, centroids, dim_start, margin):
    """How many of the points a model was called on have a float32 (torch.cdist) membership other than the float64 one."""
    xt = torch.from_numpy(np.ascontiguousarray(x[:, :3]))
    d = torch.cdist(xt[:, dim_start:], torch.from_numpy(centroids[:, dim_start:]))
    m32 = d <= margin * d.min(dim=1, keepdim=True)[0]
    m64 = R.assign(x, centroids, dim_start, margin, torch.float64) > 0
    return int((m32 != m64).any(1).sum())


def gen_render(subs, subs_bg):
    print("[mega sh] render_rays, sh_deg 2, both models of a container: 64 rays x 32 (16 background) samples; 32 (16) fine samples")
    N, S, Fn, margin, deg = 64, 32, 32, 1.15, 2
    center, radius = synth.SPHERE_CENTER, synth.SPHERE_RADIUS
    centroids = (center + 0.5 * radius * CENTROIDS).astype(np.float32)          # inside the foreground bound
    rays, img, _ = synth.make_bg_rays(541, N, CFG["appearance_count"])
    out = dict(N=N, S=S, F=Fn, margin=margin, deg=deg, seed=SEED_FG[deg], seed_bg=SEED_BG, rays=rays, image_indices=img, centroids=centroids,
               sphere_center=center, sphere_radius=radius)
    for typ, fine, c2d in (("coarse", 0, False), ("fine", Fn, True)):
        fg = MegaNeRF(subs, torch.from_numpy(centroids), margin, False, c2d).eval()
        bg = MegaNeRF(subs_bg, torch.from_numpy(centroids), margin, True, c2d).eval()
        seen = {fg: [], bg: []}
        hooks = [m.register_forward_pre_hook(lambda mod, args: seen[mod].append(args[0].numpy().copy())) for m in (fg, bg)]
        h = gg.make_hparams(synth.BUILDING, coarse=S, chunk=1000, perturb=0.0, fine=fine)      # (a ragged last model chunk)
        h.use_moe, h.pos_dir_dim, h.appearance_dim, h.sh_deg, h.return_sigma, h.moe_return_gates = False, 0, CFG["appearance_dim"], deg, False, False
        h.container_path = "container"                   # (rendering.py:52: what puts the real position in front of the background points)
        with torch.no_grad():
            res, present = rendering.render_rays(fg, bg, torch.from_numpy(rays), torch.from_numpy(img), h, torch.from_numpy(center),
                                                 torch.from_numpy(radius), get_depth=True, get_depth_variance=True, get_bg_fg_rgb=True)
        for hk in hooks:
            hk.remove()
        n_bg = int((res[f"bg_rgb_{typ}"].abs().sum(1) > 0).sum())
        assert present and 0 < n_bg < N, n_bg
        assert all(a.shape[1] == w for m, w in ((fg, 4), (bg, 8)) for a in seen[m])          # (no direction columns: rendering.py:320-323)
        n_diff = [membership_differs(np.concatenate(seen[m]), centroids, 1 if c2d else 0, margin) for m in (fg, bg)]
        print(f"  {typ}: {n_bg} rays leave the bound; points whose membership differs: foreground {n_diff[0]}, background {n_diff[1]}")
        assert n_diff == [0, 0]              # (the test compares every ray)
        out[f"cluster_2d_{typ}"] = int(c2d)
        out.update({f"{k}_{typ}": res[f"{k}_{typ}"].numpy() for k in ("rgb", "depth", "depth_variance", "fg_rgb", "bg_rgb")})
    gg.save("mega_sh_render", **out)


if __name__ == "__main__":
    os.makedirs(gg.OUT, exist_ok=True)
    torch.set_num_threads(8)
    subs = {deg: gen_fg(deg) for deg in (0, 2, 4)}
    subs_bg = gen_bg()
    gen_render(subs[2], subs_bg)
