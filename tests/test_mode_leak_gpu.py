"""A forward's mode (saving or not, which heads) travels in its context, so calls on one model do not steer each other: a sequence of
calls on ONE model gives what each call gives alone on a fresh model.  Equality is exact: two fresh models of one seed agree bit for bit
on each of these calls (no launch here accumulates with atomics), as tests/test_sh_gpu.py's autograd-bridge test already relies on.
layer_dim is 256, the narrowest model the head kernels take (swn_heads_sh_fwd, swn_heads_coef_fwd: model_dim in {256, 512})."""
import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu
CFG = dict(layer_dim=256, layers=2, skip_layers=(1,), pos_xyz_dim=4, pos_dir_dim=0, appearance_dim=8, appearance_count=4, xyz_dim=3,
           sh_deg=2)
P, N, S = 64, 8, 8


def _fresh():
    from switch_nerf_amd.dense import DenseNeRF
    return DenseNeRF(CFG, dtype=torch.float32, seed=11)


def _inputs():
    g = torch.Generator().manual_seed(12)
    x = torch.cat([torch.rand(P, 3, generator=g) - 0.5, torch.randint(0, 4, (P, 1), generator=g).float()], 1).cuda()
    rays, img, _ = synth.make_rays(13, N, CFG["appearance_count"])
    rays, img = torch.from_numpy(np.ascontiguousarray(rays)).cuda(), torch.from_numpy(np.ascontiguousarray(img)).cuda()
    return x, rays, img, torch.randn(N * S, 4, generator=g).cuda()


def _call(m, x, rays, img, d_raw):
    m.eval()
    out = m(x).clone()
    m.train()
    return (out,)


def _coef(m, x, rays, img, d_raw):
    buf = torch.zeros(P, 28, device="cuda")
    c = m.forward_coef(x, None, buf)
    assert c["coef_rows"].data_ptr() == buf.data_ptr() and not c["no_grad"]
    return (buf,)


def _train(m, x, rays, img, d_raw):
    m.grad.zero_()
    c = m.forward_rays(rays, img, S, N * S, training=True, composite=False)
    m.backward_net(c, d_raw)
    return c["raw"].clone(), m.grad.clone()


def test_a_sequence_of_calls_on_one_model_equals_each_call_alone():
    inputs = _inputs()
    a = _fresh()
    for name, fn in (("call", _call), ("forward_coef", _coef), ("train", _train), ("call", _call)):
        got, alone = fn(a, *inputs), fn(_fresh(), *inputs)
        for i, (u, v) in enumerate(zip(got, alone)):
            assert u.shape == v.shape and u.abs().sum().item() > 0
            assert torch.equal(u, v), f"{name}[{i}]: max difference {(u - v).abs().max().item():.3e}"


def test_background_training_pass_after_an_evaluation_pass_saves():
    from switch_nerf_amd.background import BackgroundScene
    from switch_nerf_amd.dense import DenseNeRF
    plain = dict(CFG, pos_dir_dim=2, appearance_count=10, sh_deg=None)
    scene = BackgroundScene(DenseNeRF(plain, dtype=torch.float32, seed=14), DenseNeRF(dict(plain, xyz_dim=4), dtype=torch.float32, seed=15),
                            synth.SPHERE_CENTER, synth.SPHERE_RADIUS)
    rays, img, _ = synth.make_bg_rays(83, 16)
    rays, img = torch.from_numpy(np.ascontiguousarray(rays)).cuda(), torch.from_numpy(np.ascontiguousarray(img)).cuda()
    ev = scene.forward(rays, img, S, 16 * S, training=False)
    tr = scene.forward(rays, img, S, 16 * S, training=True)
    assert ev["Nb"] > 0 and ev["bg"]["c"]["no_grad"] is True and ev["c"]["no_grad"] is True
    assert tr["bg"]["c"]["no_grad"] is False and tr["c"]["no_grad"] is False
