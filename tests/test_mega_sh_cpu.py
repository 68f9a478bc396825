"""CPU-only: the numpy restatement of the Mega-NeRF blend with spherical-harmonics sub-models (tests/mega_sh_restate.py) pinned on the
reference's own results (tests/golden/mega_sh_*.npz, scripts/gen_golden_mega_sh.py), and what switch_nerf_amd.mega decides before any
kernel runs: the configuration read off an SH state dict, the combinations MegaNeRF refuses, the hparams.sh_deg rule of render_rays.

A point is excluded only where the reference's float32 membership (torch.cdist) differs from a float64 evaluation of the same
distances; the fixtures are chosen so that this is at most 1 % (asserted here again; the committed fixtures have none)."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import mega_restate as R
import mega_sh_restate as RS
import sh_weights as SW
import synth

G = os.path.join(os.path.dirname(__file__), "golden")
CASES = [("mega_sh_fg_d0", "m100", 1.0), ("mega_sh_fg_d0", "m115", 1.15), ("mega_sh_fg_d2", "m100", 1.0), ("mega_sh_fg_d2", "m115", 1.15),
         ("mega_sh_fg_d4", "m100", 1.0), ("mega_sh_fg_d4", "m115", 1.15), ("mega_sh_bg", "m115", 1.15)]
CFG = dict(layer_dim=256, layers=2, skip_layers=(1,), pos_xyz_dim=3, pos_dir_dim=0, appearance_dim=8, appearance_count=4, xyz_dim=3)
CEN = np.array([[-0.5, -0.4, 0.1], [0.5, -0.3, -0.2], [0.0, 0.5, 0.3]], np.float32)


@pytest.mark.parametrize("name,tag,margin", CASES)
def test_restatement_vs_reference_golden(name, tag, margin):
    g = np.load(os.path.join(G, name + ".npz"))
    x, cen, ds, deg, hard = g["x"], g["centroids"], int(g["cluster_2d"]), int(g["deg"]), margin == 1
    B = (deg + 1) ** 2
    w_ref = g["weights_" + tag]
    w64 = R.assign(x, cen, ds, margin, torch.float64).numpy()
    excluded = ((w64 > 0) != (w_ref > 0)).any(1)
    np.testing.assert_array_equal(excluded, g["excluded_" + tag])
    keep = ~excluded
    assert keep.mean() >= 0.99
    counts, begin, rows, slot = R.pack(w_ref)
    sub = g["sub_" + tag]
    assert begin[-1] == len(sub) and sub.shape[1] == 3 * B + 1 == g["out_" + tag].shape[1]
    # the reference's own weights and per-cell outputs reproduce its module output exactly (same loop, same order, float32) ...
    np.testing.assert_array_equal(RS.blend_rows(w_ref, slot, begin, sub, hard, np.float32), g["out_" + tag])
    # ... and the float64 evaluation of the whole formula, with the restated float64 weights, its rendered form within the stored bound
    w64[excluded] = w_ref[excluded]
    raw, rows64 = RS.blend_sh(w64, slot, begin, sub, g["dirs"], 1, deg, hard)
    err = np.abs(raw - g["raw_" + tag])[keep]
    print(f"{name} {tag}: rgb err {err[:, :3].max():.3e}, sigma err {err[:, 3].max():.3e}, bound {float(g['blend_sh_tol']):.3e}")
    assert err.max() <= float(g["blend_sh_tol"])
    assert ((raw[:, :3] > 0) & (raw[:, :3] < 1)).all()
    np.testing.assert_allclose(rows64[keep, 3 * B], g["sigma_" + tag][keep, 0], rtol=1e-5, atol=1e-6)      # (sigma_only: the same density)
    # one direction for a group of rows is the same evaluation
    d8 = np.repeat(g["dirs"][: len(x) // 8], 8, 0)
    np.testing.assert_array_equal(RS.eval_rows(rows64, d8, 1, deg), RS.eval_rows(rows64, g["dirs"][: len(x) // 8], 8, deg))


def test_basis_is_the_references():
    g = np.load(os.path.join(G, "sh_eval.npz"))
    for deg in range(5):
        B = (deg + 1) ** 2
        rows = np.concatenate([g[f"coef_{deg}"].reshape(64, 3 * B), np.zeros((64, 1))], 1)
        rgb = RS.eval_rows(rows, g["dirs"], 1, deg)[:, :3]          # (compared behind the sigmoid: inverting it would cancel near 0 and 1)
        np.testing.assert_allclose(rgb, 1 / (1 + np.exp(-g[f"out64_{deg}"])), rtol=0, atol=1e-14)


@pytest.mark.parametrize("xyz_dim", [3, 4])
@pytest.mark.parametrize("deg", [0, 2, 4])
def test_dense_cfg_from_sh_state_dict(deg, xyz_dim):
    from switch_nerf_amd.mega import dense_cfg_from_state_dict
    cfg = dict(CFG, xyz_dim=xyz_dim)
    got = dense_cfg_from_state_dict(SW.make_sh_weights(7, deg, cfg), xyz_dim, allow_sh=True)
    assert got == dict(cfg, sh_deg=deg) and got["pos_dir_dim"] == 0
    plain = dict(cfg, pos_dir_dim=2)
    for allow in (False, True):
        got = dense_cfg_from_state_dict(synth.make_dense_weights(7, plain), xyz_dim, allow_sh=allow)
        assert got == plain and "sh_deg" not in got
    if deg > 0:          # (without the switch the SH layout raises as before)
        with pytest.raises(NotImplementedError, match="sh_deg.*allow_sh=True"):
            dense_cfg_from_state_dict(SW.make_sh_weights(7, deg, cfg), xyz_dim)


def test_dense_cfg_rejects_other_layouts():
    from switch_nerf_amd.mega import dense_cfg_from_state_dict
    sd = SW.make_sh_weights(7, 2, CFG)
    bad = dict(sd, **{"rgb.weight": sd["rgb.weight"][:15], "rgb.bias": sd["rgb.bias"][:15]})
    with pytest.raises(ValueError, match="15 rows"):
        dense_cfg_from_state_dict(bad, 3, allow_sh=True)
    plain = synth.make_dense_weights(7, dict(CFG, pos_dir_dim=2))
    mixed = dict(plain, **{"rgb.weight": sd["rgb.weight"], "rgb.bias": sd["rgb.bias"]})      # 27 rows behind a direction block
    with pytest.raises(ValueError, match="no direction block"):
        dense_cfg_from_state_dict(mixed, 3, allow_sh=True)
    with pytest.raises(NotImplementedError, match="affine"):
        dense_cfg_from_state_dict(dict(sd, **{"affine.weight": np.zeros((12, 8), np.float32)}), 3, allow_sh=True)
    no_app = {k: v for k, v in sd.items() if k != "embedding_a.weight"}          # appearance_dim == 0: another topology
    with pytest.raises(NotImplementedError, match="embedding_a"):
        dense_cfg_from_state_dict(no_app, 3, allow_sh=True)


def test_mega_sh_construction_and_refusals():
    from switch_nerf_amd.dense import DenseNeRF
    from switch_nerf_amd.mega import MegaNeRF
    sds = [SW.make_sh_weights(20 + i, 2, CFG) for i in range(3)]
    m = MegaNeRF.from_state_dicts(sds, CEN, None, boundary_margin=1.15, device="cpu")
    assert m.sh_deg == 2 and m.n_out == 28 and all(s.sh_deg == 2 and s.cfg["pos_dir_dim"] == 0 for s in m.sub_modules)
    for got, sd in zip(m.state_dicts(), sds):
        assert set(got) == set(sd)
        for k in sd:
            np.testing.assert_array_equal(got[k].numpy(), sd[k])
    bg = MegaNeRF.from_state_dicts([SW.make_sh_weights(30 + i, 2, dict(CFG, xyz_dim=4)) for i in range(3)], CEN, None, xyz_real=True, device="cpu")
    assert bg.sh_deg == 2 and bg.xyz_real and bg.xyz_dim == 4
    plain = MegaNeRF.from_state_dicts([synth.make_dense_weights(40 + i, dict(CFG, pos_dir_dim=2)) for i in range(3)], CEN, None, device="cpu")
    assert plain.sh_deg is None and plain.n_out == 4
    with pytest.raises(ValueError, match="different spherical-harmonics degrees"):
        MegaNeRF.from_state_dicts(sds[:2] + [SW.make_sh_weights(22, 3, CFG)], CEN, None, device="cpu")
    with pytest.raises(ValueError, match="mix spherical-harmonics colour and plain"):
        MegaNeRF(m.sub_modules[:2] + plain.sub_modules[:1], CEN, 1.15, False, False)
    with pytest.raises(NotImplementedError, match="appearance_dim == 0"):
        DenseNeRF(dict(CFG, sh_deg=2, appearance_dim=0), dtype=torch.float32, device="cpu")
    with pytest.raises(NotImplementedError, match="affine_appearance"):
        DenseNeRF(dict(CFG, sh_deg=2, affine_appearance=True), dtype=torch.float32, device="cpu")
    with pytest.raises(NotImplementedError, match="call_rgb is the spherical-harmonics form"):
        plain.call_rgb(torch.zeros(4, 7), torch.zeros(4, 3))
    with pytest.raises(Exception, match="Unexpected input shape"):          # (direction columns are not part of an SH model's input)
        m(torch.zeros(4, 7))
    with pytest.raises(ValueError, match="call_rgb: dirs"):
        m.call_rgb(torch.zeros(6, 4), torch.zeros(2, 3), 4)


class _StandInShNeRF(torch.nn.Module):
    """The parameter layout of the reference's NeRF(rgb_dim = 3 B, pos_dir_dim = 0) (key names and shapes only)."""

    def __init__(self, cfg, deg):
        super().__init__()
        W, xd = cfg["layer_dim"], cfg["xyz_dim"]
        in_xyz = xd + xd * 2 * cfg["pos_xyz_dim"]
        lin = torch.nn.Linear
        self.xyz_encodings = torch.nn.ModuleList([
            torch.nn.Sequential(lin(in_xyz if i == 0 else (W + in_xyz if i in cfg["skip_layers"] else W), W), torch.nn.ReLU(True))
            for i in range(cfg["layers"])])
        self.embedding_a = torch.nn.Embedding(cfg["appearance_count"], cfg["appearance_dim"])
        self.xyz_encoding_final = lin(W, W)
        self.dir_a_encoding = torch.nn.Sequential(lin(W + cfg["appearance_dim"], W // 2), torch.nn.ReLU(True))
        self.sigma = lin(W, 1)
        self.rgb = lin(W // 2, 3 * (deg + 1) ** 2)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return x


class _StandInContainer(torch.nn.Module):
    def __init__(self, fg, bg, centroids, cluster_2d):
        super().__init__()
        for i, m in enumerate(fg):
            setattr(self, f"sub_module_{i}", m)
        for i, m in enumerate(bg):
            setattr(self, f"bg_sub_module_{i}", m)
        self.register_buffer("centroids", centroids)
        self.cluster_2d = cluster_2d

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return x


def test_from_container_with_sh_sub_models(tmp_path):
    from switch_nerf_amd.mega import MegaNeRF
    deg, cfg_bg = 3, dict(CFG, xyz_dim=4)
    mods, sds = {}, {}
    for key, cfg, seed in (("fg", CFG, 60), ("bg", cfg_bg, 70)):
        sds[key] = [SW.make_sh_weights(seed + i, deg, cfg) for i in range(3)]
        mods[key] = []
        for sd in sds[key]:
            mod = _StandInShNeRF(cfg, deg)
            mod.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
            mods[key].append(mod)
    path = str(tmp_path / "container.pt")
    torch.jit.save(torch.jit.script(_StandInContainer(mods["fg"], mods["bg"], torch.from_numpy(CEN), False)), path)
    for background, key, cfg in ((False, "fg", CFG), (True, "bg", cfg_bg)):
        m = MegaNeRF.from_container(path, 1.15, background=background, device="cpu")
        assert m.sh_deg == deg and m.xyz_real == background and m.n_out == 3 * 16 + 1
        for sub, sd in zip(m.sub_modules, sds[key]):
            assert {k: sub.cfg[k] for k in cfg} == cfg and sub.cfg["sh_deg"] == deg
            out = sub.state_dict()
            for k in sd:
                np.testing.assert_array_equal(out[k].numpy(), sd[k])


def test_render_rays_sh_deg_must_match_the_models():
    from switch_nerf_amd.mega import MegaNeRF
    from switch_nerf_amd.rendering import render_rays
    m = MegaNeRF.from_state_dicts([SW.make_sh_weights(20 + i, 2, CFG) for i in range(3)], CEN, None, device="cpu")
    bg3 = MegaNeRF.from_state_dicts([SW.make_sh_weights(30 + i, 3, dict(CFG, xyz_dim=4)) for i in range(3)], CEN, None, xyz_real=True, device="cpu")
    plain = MegaNeRF.from_state_dicts([synth.make_dense_weights(40 + i, dict(CFG, pos_dir_dim=2)) for i in range(3)], CEN, None, device="cpu")
    rays = torch.zeros(4, 8)
    h = Namespace(coarse_samples=8, fine_samples=0, model_chunk_size=1000, sh_deg=3)
    with pytest.raises(NotImplementedError, match=r"hparams\.sh_deg = 3 but the model was built with sh_deg = 2"):
        render_rays(m, None, rays, None, h, None, None)
    h.sh_deg = None
    with pytest.raises(NotImplementedError, match=r"hparams\.sh_deg = None but the model was built with sh_deg = 2"):
        render_rays(m, None, rays, None, h, None, None)
    h.sh_deg = 2
    with pytest.raises(NotImplementedError, match=r"hparams\.sh_deg = 2 but the background model was built with sh_deg = 3"):
        render_rays(m, bg3, rays, None, h, None, None)
    with pytest.raises(NotImplementedError, match=r"hparams\.sh_deg = 2 but the model was built with sh_deg = None"):
        render_rays(plain, None, rays, None, h, None, None)
