"""CPU-only: the fp64 restatement of the spherical-harmonics colour path (tests/sh_restate.py) pinned on the reference's own outputs,
the configurations the dense NeRF refuses, and the reference key layout of an sh_deg model (host-resident model: no kernel runs)."""
import os

import numpy as np
import pytest
import torch

import sh_restate as R
import sh_weights as SW
import synth

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_restated_basis_matches_reference_eval_sh():
    """fp64 restatement against the reference's fp64 run: rounding of the two evaluation orders only; its fp32 run: fp32 rounding of
    sums of up to 25 terms of size |coef| |Y| (non-unit directions up to length 3 make |Y| reach ~50 at degree 4)."""
    g = np.load(os.path.join(G, "sh_eval.npz"))
    dirs = torch.from_numpy(g["dirs"])
    assert (np.abs(np.linalg.norm(g["dirs"][-8:], axis=1) - 1) > 0.05).any()
    for deg in range(5):
        coef = torch.from_numpy(g[f"coef_{deg}"])
        out = R.eval_sh(deg, coef.double(), dirs.double())
        scale = (coef.double().abs() * R.basis(deg, dirs.double()).abs()[:, None, :]).sum(-1)       # sum of |terms| per output
        assert ((out - torch.from_numpy(g[f"out64_{deg}"])).abs() <= 1e-14 * scale + 1e-300).all(), deg
        assert ((out - torch.from_numpy(g[f"out_{deg}"]).double()).abs() <= 2.0 ** -21 * scale).all(), deg
        assert R.basis(deg, dirs).shape == (64, (deg + 1) ** 2)


def test_restated_module_matches_reference_forward():
    g = np.load(os.path.join(G, "sh_dense_fwd.npz"))
    cfg = {k[5:]: (tuple(int(i) for i in v) if v.ndim else int(v)) for k, v in g.items() if k.startswith("cfg__")}
    assert cfg == SW.SH_CFG
    for deg in (2, 3):
        sd = SW.make_sh_weights(int(g[f"seed_{deg}"]), deg)
        np.testing.assert_allclose(np.sum([synth.checksum(v) for v in sd.values()], 0), g[f"sd_checksum_{deg}"], rtol=1e-12)
        out = R.module_forward(sd, cfg, g["x"], g["sigma_noise"])
        assert out.shape == (257, 3 * (deg + 1) ** 2 + 1)
        # the reference's fp32 run sits within its own measured fp32 error of fp64 (2 x: the restatement's order of operations differs)
        assert float((out - torch.from_numpy(g[f"out_{deg}"]).double()).abs().max()) <= 2 * float(g[f"fwd_err_{deg}"])
        sig = R.module_forward(sd, cfg, g["x"], None)[:, -1:]
        assert float((sig - torch.from_numpy(g[f"sigma_only_{deg}"]).double()).abs().max()) <= 2 * float(g[f"fwd_err_{deg}"])


def test_restated_heads_gradients_match_autograd():
    """heads_bwd's closed forms against autograd through heads_fwd (fp64), rows_per_group 1 and S."""
    for case in ((2, 5, 13, 13, True), (3, 5, 13, 1, True)):
        deg, N, S, rpg, _ = case
        c = {k: (None if v is None else torch.from_numpy(v).double()) for k, v in SW.head_case(*case).items()}
        pre = c["h2"].clone()
        pre[c["h2"] == 0] = -1.0
        pre.requires_grad_(True)
        leaves = {k: c[k].clone().requires_grad_(True) for k in ("ws", "bs", "wc", "bc")}
        raw, _ = R.heads_fwd(c["y"], torch.relu(pre), leaves["ws"], leaves["bs"], leaves["wc"], leaves["bc"], c["noise"], c["dirs"], rpg, deg)
        raw.backward(c["d_raw"])
        b = R.heads_bwd(c["y"], c["h2"], c["ws"], c["bs"], c["wc"], c["bc"], c["noise"], c["dirs"], rpg, deg, c["d_raw"])
        for k, ref in (("dh2", pre.grad), ("d_ws", leaves["ws"].grad), ("d_bs", leaves["bs"].grad[0]), ("d_wc", leaves["wc"].grad),
                       ("d_bc", leaves["bc"].grad)):
            assert float((b[k] - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max())), k


BAD = [(dict(sh_deg=2, affine_appearance=True), NotImplementedError), (dict(sh_deg=2, pos_dir_dim=4), ValueError),
       (dict(sh_deg=2, appearance_dim=0), NotImplementedError), (dict(sh_deg=5), ValueError), (dict(sh_deg=-1), ValueError),
       (dict(sh_deg=1.5), ValueError)]


@pytest.mark.parametrize("extra,exc", BAD)
def test_refused_configurations_name_the_key(extra, exc):
    from switch_nerf_amd.dense import DenseNeRF
    with pytest.raises(exc, match="sh_deg"):
        DenseNeRF(dict(SW.SH_CFG, **extra), dtype=torch.float32, device="cpu")


def test_switch_nerf_and_mega_refuse_sh():
    from switch_nerf_amd.model import SwitchNeRF
    from switch_nerf_amd import mega, rendering
    from argparse import Namespace
    with pytest.raises(NotImplementedError, match=r"sh_deg.*nerf_moe.py:186-189"):
        SwitchNeRF(dict(synth.small_cfg(), sh_deg=2), dtype=torch.float32, device="cpu")
    moe = SwitchNeRF(synth.small_cfg(), dtype=torch.float32, device="cpu")
    with pytest.raises(NotImplementedError, match=r"sh_deg.*nerf_moe.py:186-189"):
        rendering._check_sh(moe, None, Namespace(sh_deg=2))
    with pytest.raises(NotImplementedError, match="sh_deg"):
        mega.dense_cfg_from_state_dict({k: torch.from_numpy(v) for k, v in SW.make_sh_weights(1, 2).items()}, 3)


def test_render_rays_hparams_must_match_the_model():
    from argparse import Namespace
    from switch_nerf_amd.dense import DenseNeRF
    from switch_nerf_amd import rendering
    m = DenseNeRF(SW.sh_cfg(2), dtype=torch.float32, device="cpu")
    plain = DenseNeRF(dict(SW.SH_CFG, pos_dir_dim=2), dtype=torch.float32, device="cpu")
    rendering._check_sh(m, None, Namespace(sh_deg=2))
    rendering._check_sh(plain, None, Namespace(sh_deg=None))
    rendering._check_sh(plain, None, Namespace())
    for model, want in ((m, 3), (m, None), (plain, 2)):
        with pytest.raises(NotImplementedError, match="sh_deg"):
            rendering._check_sh(model, None, Namespace(sh_deg=want))
    with pytest.raises(NotImplementedError, match="background"):
        rendering._check_sh(m, plain, Namespace(sh_deg=2))


@pytest.mark.parametrize("deg", [0, 2, 4])
def test_state_dict_layout_round_trip(deg):
    """The reference key layout: rgb.weight [3 B, W / 2], dir_a_encoding.0.weight [W / 2, W + appearance_dim] (no direction block)."""
    from switch_nerf_amd.dense import DenseNeRF
    cfg, B = SW.sh_cfg(deg), (deg + 1) ** 2
    sd = SW.make_sh_weights(77, deg)
    m = DenseNeRF(cfg, dtype=torch.float32, device="cpu")
    assert m.sh_deg == deg and m.in_dir == 0 and m.n_ray_feat == cfg["appearance_dim"]
    m.load_state_dict({"module." + k: v for k, v in sd.items()})
    back = m.state_dict()
    assert set(back) == set(sd)
    assert tuple(back["rgb.weight"].shape) == (3 * B, 128) and tuple(back["rgb.bias"].shape) == (3 * B,)
    assert tuple(back["dir_a_encoding.0.weight"].shape) == (128, 256 + cfg["appearance_dim"])
    for k, v in sd.items():
        assert np.array_equal(back[k].numpy(), v), k
    assert tuple(m.grad_dict()["rgb.weight"].shape) == (3 * B, 128)
    if deg != 2:
        with pytest.raises(ValueError, match="rgb.weight"):
            m.load_state_dict(SW.make_sh_weights(77, 2))


def test_plain_dense_layout_is_unchanged():
    from switch_nerf_amd.dense import DenseNeRF
    m = DenseNeRF(synth.DENSE, dtype=torch.float32, device="cpu")
    assert m.sh_deg is None and m.in_dir == 27 and m.DP == 32 and m.n_color == 3
    assert m.spec["color.w"][1] == (3, 128) and m.spec["l2r.w"][1] == (27 + 48, 128)
