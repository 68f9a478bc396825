"""CPU-only: the opt-in training switch of switch_nerf_amd.mega.MegaNeRF (joint_training) - the constructor flag, the parameter views,
what stays refused - and the consistency of the training fixtures (tests/golden/mega_train.npz, mega_train_module.npz;
scripts/gen_golden_mega_train.py): the seeded weights' checksums, and no stored point on a membership decision."""
import os

import numpy as np
import pytest
import torch

import mega_restate as R
import mega_train_restate as RT
import synth

G = os.path.join(os.path.dirname(__file__), "golden")
CFG = dict(layer_dim=256, layers=2, skip_layers=(1,), pos_xyz_dim=3, pos_dir_dim=2, appearance_dim=8, appearance_count=4, xyz_dim=3)
CEN = np.array([[-0.5, -0.4, 0.1], [0.5, -0.3, -0.2], [0.0, 0.5, 0.3]], np.float32)


def _subs(cfg=CFG, dtype=torch.float32, n=3):
    from switch_nerf_amd.dense import DenseNeRF
    subs = []
    for i in range(n):
        m = DenseNeRF(cfg, dtype=dtype, device="cpu")
        if cfg.get("sh_deg") is None:                  # (an sh_deg model keeps its random initialisation: only its kind matters here)
            m.load_state_dict(synth.make_dense_weights(501 + i, cfg))
        subs.append(m)
    return subs


def test_joint_training_flag_and_parameter_views():
    from switch_nerf_amd.mega import MegaNeRF
    sds = [synth.make_dense_weights(501 + i, CFG) for i in range(3)]
    m = MegaNeRF.from_state_dicts(sds, CEN, CFG, boundary_margin=1.0, device="cpu", joint_training=True)
    assert m.joint_training and m.training and all(s.training for s in m.sub_modules)
    assert m.eval() is m and not m.training and not any(s.training for s in m.sub_modules)
    assert m.train() is m and m.training and all(s.training for s in m.sub_modules)
    named = dict(m.named_parameters())
    assert list(named) == [f"sub_modules.{i}.{k}" for i in range(3) for k in dict(m.sub_modules[i].named_parameters())]
    assert set(named) == {f"sub_modules.{i}.{k}" for i in range(3) for k in sds[i]}
    for i in range(3):
        for k, v in sds[i].items():
            np.testing.assert_array_equal(named[f"sub_modules.{i}.{k}"].numpy(), v)
    assert len(list(m.parameters())) == len(named) == 39
    gd = m.grad_dict()
    assert set(gd) == set(named) and all(tuple(gd[k].shape) == tuple(named[k].shape) and not gd[k].any() for k in gd)
    assert m.set_iteration(1000) == pytest.approx(5e-4 * 0.1 ** (1000 / 500000)) and all(s.lr == m.lr for s in m.sub_modules)
    # the constructor itself, and soft margins
    m2 = MegaNeRF(_subs(), CEN, 1.15, False, True, joint_training=True)
    assert m2.joint_training and m2.training and m2.cluster_dim_start == 1


def test_default_stays_inference_only():
    from switch_nerf_amd.mega import MegaNeRF
    m = MegaNeRF(_subs(), CEN, 1.15, False, False)
    assert not m.joint_training and not m.training and not any(s.training for s in m.sub_modules)
    with pytest.raises(NotImplementedError, match="inference only"):
        m.train()
    assert m.train(False) is m and m.eval() is m
    x = torch.zeros(4, 7)
    for call in (lambda: m.forward_points(x), lambda: m.backward_points({}, x[:, :4]), lambda: m.apply_step(),
                 lambda: m.grad_step(x[:, :3], torch.zeros(4, 8), torch.zeros(4, dtype=torch.long), 2),
                 lambda: m.train_step(x[:, :3], torch.zeros(4, 8), torch.zeros(4, dtype=torch.long), 2)):
        with pytest.raises(NotImplementedError, match="inference only"):
            call()


def test_from_container_stays_inference_only():
    import inspect
    from switch_nerf_amd.mega import MegaNeRF
    assert "joint_training" not in inspect.signature(MegaNeRF.from_container).parameters
    assert "joint_training" in inspect.signature(MegaNeRF.from_state_dicts).parameters


def test_what_training_refuses(monkeypatch):
    from switch_nerf_amd import mega
    from switch_nerf_amd.mega import MegaNeRF
    sh = dict(CFG, pos_dir_dim=0, sh_deg=1)
    with pytest.raises(NotImplementedError, match="spherical-harmonics"):
        MegaNeRF(_subs(sh), CEN, 1.0, False, False, joint_training=True)
    with pytest.raises(NotImplementedError, match="xyz_real"):
        MegaNeRF(_subs(dict(CFG, xyz_dim=4)), CEN, 1.0, True, False, joint_training=True)
    with pytest.raises(NotImplementedError, match="fp16"):
        MegaNeRF(_subs(dtype=torch.float16), CEN, 1.0, False, False, joint_training=True)
    subs = _subs()
    subs[1].set_device_noise(3)
    with pytest.raises(NotImplementedError, match="device noise"):
        MegaNeRF(subs, CEN, 1.0, False, False, joint_training=True)
    subs = _subs()
    subs[2].ep = object()
    with pytest.raises(NotImplementedError, match="expert parallelism"):
        MegaNeRF(subs, CEN, 1.0, False, False, joint_training=True)
    # all of them still build without the flag, as before
    MegaNeRF(_subs(sh), CEN, 1.0, False, False)
    MegaNeRF(_subs(dict(CFG, xyz_dim=4)), CEN, 1.0, True, False)
    m = MegaNeRF(_subs(), CEN, 1.0, False, False, joint_training=True)
    with pytest.raises(NotImplementedError, match="device noise"):
        m.set_device_noise(7)
    m.set_device_noise(None)
    with pytest.raises(NotImplementedError, match="expert parallelism"):
        m.set_expert_parallel(object())
    with pytest.raises(NotImplementedError, match="data parallelism"):
        m.apply_step(grad_allreduce=lambda flat: 1.0)
    rays, img = torch.zeros(4, 8), torch.zeros(4, dtype=torch.long)
    # graph capture: refused at the first launch-free line of a pass made while the stream is capturing (no device is touched here)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(NotImplementedError, match="graph capture is not built"):
        m.forward_points(torch.zeros(4, 7))
    monkeypatch.undo()
    from argparse import Namespace
    h = Namespace(coarse_samples=2, fine_samples=0, model_chunk_size=8)
    with pytest.raises(NotImplementedError, match="evaluation mode"):      # training mode: no autograd bridge for a MegaNeRF yet
        mega.render_rays(m, None, rays, img, h)
    assert "autograd bridge" in " ".join(mega.render_rays.__doc__.split())


def test_fixture_weights_and_points_off_every_decision():
    g, gm, fg = (np.load(os.path.join(G, n + ".npz")) for n in ("mega_train", "mega_train_module", "mega_fg"))
    cfg = {k[5:]: (tuple(int(v) for v in g[k]) if g[k].ndim else int(g[k])) for k in g.files if k.startswith("cfg__")}
    assert cfg == CFG and int(g["seed"]) == int(gm["seed"]) == int(fg["seed"])
    np.testing.assert_array_equal(g["centroids"], fg["centroids"])
    names = [f"sub_modules.{i}.{k}" for i in range(3) for k in synth.make_dense_weights(int(g["seed"]) + i, cfg)]
    for f in (g, gm):
        for i, ref in enumerate(f["sd_checksums"]):
            sd = synth.make_dense_weights(int(f["seed"]) + i, cfg)
            np.testing.assert_allclose(np.sum([synth.checksum(v) for v in sd.values()], 0), ref, rtol=1e-12)
        assert sorted(str(n) for n in f["param_names"]) == sorted(names)
    # the coarse sample points of both ray sets, at the reference's distance error as the generator measured it on every model input
    err = max(float(g["a_dist_err"]), float(g["b_dist_err"]))
    t = np.linspace(0, 1, int(g["S"]), dtype=np.float32)
    for key, want in (("rays", g["a_members"][0].tolist()), ("rays_cell0", [int(g["N"]) * int(g["S"]), 0, 0])):
        r = g[key]
        z = r[:, 6:7] * (1 - t) + r[:, 7:8] * t
        pts = (r[:, None, :3] + r[:, None, 3:6] * z[:, :, None]).reshape(-1, 3)
        assert not (R.boundary_gap(pts, g["centroids"], 0, 1.0) <= 4 * err).any()
        assert R.pack(R.assign(pts, g["centroids"], 0, 1.0))[0].tolist() == want
    # ... and the fine samples the reference's model was called on (their positions depend on computed weights: recorded by a hook)
    assert g["b_pts_fine"].shape == (int(g["N"]) * int(g["F"]), 3)
    assert not (R.boundary_gap(g["b_pts_fine"], g["centroids"], 0, 1.0) <= 4 * err).any()
    assert R.pack(R.assign(g["b_pts_fine"], g["centroids"], 0, 1.0))[0].tolist() == g["b_members"][1].tolist()
    for tag, margin in (("m100", 1.0), ("m115", 1.15)):
        assert not fg["excluded_" + tag].any()
        assert not (R.boundary_gap(fg["x"], fg["centroids"], 0, margin) <= 4 * float(fg["dist_err"])).any()
        assert gm["out_" + tag].shape == (len(fg["x"]), 4) and gm["d_out"].shape == (len(fg["x"]), 4)
    # the stored step-2 parameters of the cells no point reached differ from their step-1 values: a zero gradient, not a missing one
    off = g["c_offsets"]
    moved = [not np.array_equal(g["c_p1_slices"][off[i]:off[i + 1]], g["c_p2_slices"][off[i]:off[i + 1]])
             for i, n in enumerate(g["param_names"]) if not str(n).startswith("sub_modules.0.") and str(n).endswith("rgb.weight")]
    assert moved == [True, True]


def test_blend_backward_restatement_is_the_adjoint():
    """<blend(sub), d_out> == <sub, blend_bwd(d_out)> in float64 arithmetic on the float32 results, hard and soft, with an empty cell."""
    rng = np.random.default_rng(11)
    x = rng.uniform(-1, 1, (300, 3)).astype(np.float32)
    cen = np.concatenate([CEN, [[50.0, 50.0, 50.0]]]).astype(np.float32)
    for margin in (1.0, 1.15):
        w = R.assign(x, cen, 0, margin)
        counts, begin, rows, slot = R.pack(w)
        assert counts[3] == 0
        total = int(begin[-1])
        sub = rng.standard_normal((total, 4)).astype(np.float32)
        d_out = rng.standard_normal((300, 4)).astype(np.float32)
        lhs = (R.blend(w, slot, begin, sub, margin == 1).double() * torch.from_numpy(d_out).double()).sum()
        rhs = (torch.from_numpy(sub).double() * RT.blend_bwd(w, slot, begin, d_out, total, margin == 1).double()).sum()
        assert abs(float(lhs - rhs)) <= 1e-4 * (1 + abs(float(lhs)))
