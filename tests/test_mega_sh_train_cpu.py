"""CPU-only: the second opt-in of switch_nerf_amd.mega.MegaNeRF - training cells with spherical-harmonics colour (sh_training) - what it
accepts and what stays refused, the new entry points' declarations and bindings, the row-count independence of swn_heads_coef_bwd's
workspace, and the consistency of the fixtures (tests/golden/mega_sh_train*.npz; scripts/gen_golden_mega_sh_train.py): the seeded
weights' checksums and no point any model call received on a membership decision."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import mega_restate as R
import sh_weights as SW
import synth

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
CFG = dict(layer_dim=256, layers=2, skip_layers=(1,), pos_xyz_dim=3, pos_dir_dim=0, appearance_dim=8, appearance_count=4, xyz_dim=3)
CEN = np.array([[-0.5, -0.4, 0.1], [0.5, -0.3, -0.2], [0.0, 0.5, 0.3]], np.float32)
NEW = ("swn_cells_blend_sh_bwd", "swn_heads_coef_fwd", "swn_heads_coef_bwd_workspace_bytes", "swn_heads_coef_bwd")


def _subs(cfg, dtype=torch.float32, n=3):
    from switch_nerf_amd.dense import DenseNeRF
    return [DenseNeRF(cfg, dtype=dtype, device="cpu") for _ in range(n)]


def test_sh_training_is_opt_in_and_the_refusal_names_the_keyword():
    from switch_nerf_amd.mega import MegaNeRF
    sh = dict(CFG, sh_deg=2)
    with pytest.raises(NotImplementedError, match="spherical-harmonics") as e:
        MegaNeRF(_subs(sh), CEN, 1.0, False, False, joint_training=True)
    assert "sh_training=True" in str(e.value)
    for deg in range(5):
        for margin in (1.0, 1.15):
            m = MegaNeRF(_subs(dict(CFG, sh_deg=deg)), CEN, margin, False, False, joint_training=True, sh_training=True)
            assert m.joint_training and m.sh_training and m.training and m.sh_deg == deg and m.n_out == 3 * (deg + 1) ** 2 + 1
    assert "sh_training" in inspect.signature(MegaNeRF.from_state_dicts).parameters
    assert "sh_training" not in inspect.signature(MegaNeRF.from_container).parameters
    sds = [SW.make_sh_weights(511 + i, 2, CFG) for i in range(3)]
    m = MegaNeRF.from_state_dicts(sds, CEN, None, boundary_margin=1.0, device="cpu", joint_training=True, sh_training=True)
    assert m.sh_deg == 2 and m.training and len(list(m.parameters())) == 39
    # sh_training alone trains nothing, and changes nothing for plain-colour cells
    m = MegaNeRF(_subs(sh), CEN, 1.0, False, False, sh_training=True)
    assert not m.joint_training and not m.training
    with pytest.raises(NotImplementedError, match="inference only"):
        m.train()
    m = MegaNeRF(_subs(dict(CFG, pos_dir_dim=2)), CEN, 1.0, False, False, joint_training=True, sh_training=True)
    assert m.sh_deg is None and m.training


def test_what_sh_training_still_refuses(monkeypatch):
    from switch_nerf_amd import mega
    from switch_nerf_amd.mega import MegaNeRF
    sh = dict(CFG, sh_deg=2)
    kw = dict(joint_training=True, sh_training=True)
    with pytest.raises(NotImplementedError, match="xyz_real"):
        MegaNeRF(_subs(dict(sh, xyz_dim=4)), CEN, 1.0, True, False, **kw)
    with pytest.raises(NotImplementedError, match="fp16"):
        MegaNeRF(_subs(sh, torch.float16), CEN, 1.0, False, False, **kw)
    subs = _subs(sh)
    subs[1].set_device_noise(3)
    with pytest.raises(NotImplementedError, match="device noise"):
        MegaNeRF(subs, CEN, 1.0, False, False, **kw)
    subs = _subs(sh)
    subs[2].ep = object()
    with pytest.raises(NotImplementedError, match="expert parallelism"):
        MegaNeRF(subs, CEN, 1.0, False, False, **kw)
    subs = _subs(sh)
    subs[1] = _subs(dict(CFG, sh_deg=3), n=1)[0]
    with pytest.raises(ValueError, match="different spherical-harmonics degrees"):
        MegaNeRF(subs, CEN, 1.0, False, False, **kw)
    m = MegaNeRF(_subs(sh), CEN, 1.0, False, False, **kw)
    with pytest.raises(NotImplementedError, match="device noise"):
        m.set_device_noise(7)
    with pytest.raises(NotImplementedError, match="expert parallelism"):
        m.set_expert_parallel(object())
    with pytest.raises(NotImplementedError, match="data parallelism"):
        m.apply_step(grad_allreduce=lambda flat: 1.0)
    # the points carry no direction columns; the directions come beside them, one per rows_per_group points
    with pytest.raises(Exception, match="Unexpected input shape"):
        m.forward_points(torch.zeros(4, 7))
    with pytest.raises(ValueError, match="dirs"):
        m.forward_points(torch.zeros(4, 4))
    with pytest.raises(ValueError, match="dirs"):
        m.forward_points(torch.zeros(4, 4), dirs=torch.zeros(4, 3), rows_per_group=2)
    with pytest.raises(ValueError, match="dirs"):
        m.forward_points(torch.zeros(6, 4), dirs=torch.zeros(2, 3), rows_per_group=4)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(NotImplementedError, match="graph capture is not built"):
        m.forward_points(torch.zeros(4, 4), dirs=torch.zeros(4, 3))
    monkeypatch.undo()
    from argparse import Namespace
    h = Namespace(coarse_samples=2, fine_samples=0, model_chunk_size=8, sh_deg=2)
    with pytest.raises(NotImplementedError, match="evaluation mode"):
        mega.render_rays(m, None, torch.zeros(4, 8), torch.zeros(4, dtype=torch.long), h)
    # a plain-colour model takes no directions
    p = MegaNeRF(_subs(dict(CFG, pos_dir_dim=2)), CEN, 1.0, False, False, joint_training=True)
    with pytest.raises(ValueError, match="dirs belong"):
        p.forward_points(torch.zeros(4, 7), dirs=torch.zeros(4, 3))


def test_dense_forward_coef_refusals():
    from switch_nerf_amd.dense import DenseNeRF
    out = torch.zeros(4, 28)
    with pytest.raises(NotImplementedError, match="spherical-harmonics"):
        DenseNeRF(dict(CFG, pos_dir_dim=2), dtype=torch.float32, device="cpu").forward_coef(torch.zeros(4, 4), None, out)
    with pytest.raises(NotImplementedError, match="xyz_dim 3"):
        DenseNeRF(dict(CFG, sh_deg=2, xyz_dim=4), dtype=torch.float32, device="cpu").forward_coef(torch.zeros(4, 5), None, out)
    with pytest.raises(NotImplementedError, match="bfloat16 / float32"):
        DenseNeRF(dict(CFG, sh_deg=2), dtype=torch.float16, device="cpu").forward_coef(torch.zeros(4, 4), None, out)
    with pytest.raises(ValueError, match="inner_sigmoid"):
        DenseNeRF(dict(CFG, sh_deg=2), dtype=torch.float32, device="cpu").forward_coef(torch.zeros(4, 4), None, out, inner_sigmoid=True)


def test_new_symbols_are_declared_and_bound():
    from switch_nerf_amd import _lib
    header = open(os.path.join(os.path.dirname(HERE), "include", "swn.h")).read()
    sigs = next(v for v in vars(_lib).values() if isinstance(v, dict) and "swn_cells_blend_sh" in v)
    for name in NEW:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name + " is not declared in swn.h"
        assert name in sigs and len(sigs[name]) == m.group(1).count(",") + 1, name
    lib = _lib.load()
    for name in NEW:
        assert getattr(lib, name) is not None


def test_coef_bwd_workspace_does_not_grow_with_the_rows():
    from switch_nerf_amd import _lib
    lib = _lib.load()
    for M, H2 in ((256, 128), (512, 256)):
        for deg in range(5):
            got = []
            for n in (1 << 21, 1 << 22):
                nb = C.c_size_t(0)
                assert lib.swn_heads_coef_bwd_workspace_bytes(n, M, H2, deg, C.byref(nb)) == 0
                got.append(nb.value)
            assert got[0] == got[1] > 0
            # ... and stays far below the folded kernels' per-point workspace at rows_per_group = 1 (3 H2 + 4 floats per point)
            assert got[0] < (1 << 21) * (3 * H2 + 4) * 4 // 8
    nb = C.c_size_t(0)
    assert lib.swn_heads_coef_bwd_workspace_bytes(16, 256, 128, 5, C.byref(nb)) != 0
    assert lib.swn_heads_coef_bwd_workspace_bytes(16, 256, 128, 2, None) != 0


def _cfg_of(g):
    return {k[5:]: (tuple(int(v) for v in g[k]) if g[k].ndim else int(g[k])) for k in g.files if k.startswith("cfg__")}


def test_fixture_weights_and_points_off_every_decision():
    g = np.load(os.path.join(G, "mega_sh_train.npz"))
    limit = os.path.getsize(os.path.join(G, "mega_fg.npz"))
    assert os.path.getsize(os.path.join(G, "mega_sh_train.npz")) < limit
    cfg, deg = _cfg_of(g), int(g["deg"])
    assert cfg == CFG and deg == 2 and float(g["margin"]) == 1.0
    np.testing.assert_array_equal(g["centroids"], CEN)
    names = [f"sub_modules.{i}.{k}" for i in range(3) for k in SW.make_sh_weights(int(g["seed"]) + i, deg, cfg)]
    for i, ref in enumerate(g["sd_checksums"]):
        sd = SW.make_sh_weights(int(g["seed"]) + i, deg, cfg)
        np.testing.assert_allclose(np.sum([synth.checksum(v) for v in sd.values()], 0), ref, rtol=1e-12)
    assert sorted(str(n) for n in g["param_names"]) == sorted(names)
    err = max(float(g["a_dist_err"]), float(g["b_dist_err"]))
    t = np.linspace(0, 1, int(g["S"]), dtype=np.float32)
    for key, want in (("rays", g["a_members"][0].tolist()), ("rays_cell0", [int(g["N"]) * int(g["S"]), 0, 0])):
        r = g[key]
        z = r[:, 6:7] * (1 - t) + r[:, 7:8] * t
        pts = (r[:, None, :3] + r[:, None, 3:6] * z[:, :, None]).reshape(-1, 3)
        assert not (R.boundary_gap(pts, CEN, 0, 1.0) <= 4 * err).any()
        assert R.pack(R.assign(pts, CEN, 0, 1.0))[0].tolist() == want
    assert g["b_pts_fine"].shape == (int(g["N"]) * int(g["F"]), 3)
    assert not (R.boundary_gap(g["b_pts_fine"], CEN, 0, 1.0) <= 4 * err).any()
    assert R.pack(R.assign(g["b_pts_fine"], CEN, 0, 1.0))[0].tolist() == g["b_members"][1].tolist()
    off = g["c_offsets"]
    moved = [not np.array_equal(g["c_p1_slices"][off[i]:off[i + 1]], g["c_p2_slices"][off[i]:off[i + 1]])
             for i, n in enumerate(g["param_names"]) if not str(n).startswith("sub_modules.0.") and str(n).endswith("rgb.weight")]
    assert moved == [True, True]
    # module level
    for d, tags in ((0, (("m115", 1.15),)), (2, (("m100", 1.0), ("m115", 1.15))), (4, (("m115", 1.15),))):
        path = os.path.join(G, f"mega_sh_train_module_d{d}.npz")
        gm = np.load(path)
        assert os.path.getsize(path) < limit and _cfg_of(gm) == CFG and int(gm["deg"]) == d
        P = 128 if d == 4 else 256
        assert gm["x"].shape == (P, 4) and gm["dirs"].shape == (P, 3) and gm["d_raw"].shape == (P, 4) and gm["sigma_noise"].shape == (P, 1)
        for i, ref in enumerate(gm["sd_checksums"]):
            sd = SW.make_sh_weights(int(gm["seed"]) + i, d, cfg)
            np.testing.assert_allclose(np.sum([synth.checksum(v) for v in sd.values()], 0), ref, rtol=1e-12)
        for tag, margin in tags:
            assert not (R.boundary_gap(gm["x"], CEN, 0, margin) <= 4 * float(gm[tag + "_dist_err"])).any()
            assert gm["raw_" + tag].shape == (P, 4) and len(gm[tag + "_gsums"]) == 39
