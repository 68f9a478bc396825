"""Spherical-harmonics colour (cfg["sh_deg"]) of the dense NeRF on the GPU: the training step and the module call against the reference
model's own run (tests/golden/sh_dense_*.npz, scripts/gen_golden_sh.py), and the step's other drivers (autograd bridge, Adam, bf16,
chunked evaluation, point outputs) against the plain step.

A sh_deg = None model is untouched by this branch: tests/test_dense_gpu.py runs unchanged and passes (its goldens were recorded from the
reference long before; the procedure to confirm a parent-commit value is to run that file on both commits)."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import sh_restate as R
import sh_weights as SW
import synth

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _model(dtype, seed, deg=2):
    from switch_nerf_amd.dense import DenseNeRF
    m = DenseNeRF(SW.sh_cfg(deg), dtype=dtype)
    m.load_state_dict(SW.make_sh_weights(seed, deg))
    return m


def _hp(S, fine=0, chunk=1000, deg=2, **kw):
    return Namespace(coarse_samples=S, fine_samples=fine, model_chunk_size=chunk, perturb=0.0, use_sigma_noise=False, sigma_noise_std=0.0,
                     use_cascade=False, sh_deg=deg, **kw)


@pytest.mark.parametrize("tag", ["coarse", "fine"])
def test_sh_train_step_vs_reference_golden_fp32(tag):
    """The tolerances of tests/test_dense_gpu.py::test_dense_train_step_vs_reference_golden_fp32: rgb atol 1e-4, loss rtol 1e-5,
    gradient checksums 1e-3 of the absolute sum, slices rtol 2e-3 / atol 2e-4 max|ref|."""
    g = np.load(os.path.join(G, "sh_dense_train.npz"))
    N, S, Fn = int(g["N"]), int(g["S"]), int(g["F"]) if tag == "fine" else 0
    m = _model(torch.float32, int(g["seed"]), int(g["deg"]))
    rays, img, rgbs = synth.make_rays(int(g["rays_seed"]), N, SW.SH_CFG["appearance_count"])
    st = m.train_step(_dev(rgbs), _dev(rays), _dev(img), S, 1000, perturb=0.0, optimizer_step=False, fine_samples=Fn)
    np.testing.assert_allclose(st["rgb"].cpu().numpy(), g[f"rgb_{tag}"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(st["depth"].cpu().numpy(), g[f"depth_{tag}"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(st["ctx"]["raw"][:, 3].cpu().numpy().reshape(N, S)[:64], g[f"sigma_head_{tag}"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(st["loss"].item(), float(g[f"loss_{tag}"]), rtol=1e-5)
    worst = 0.0
    gd = m.grad_dict()
    assert tuple(gd["rgb.weight"].shape) == (27, 128) and gd["rgb.weight"].abs().sum(1).min().item() > 0
    for k, t in gd.items():
        got = t.cpu().numpy()
        ref_sum = g[f"gsum_{tag}__" + k]
        scale = max(1e-12, float(ref_sum[1]))
        assert abs(synth.checksum(got)[0] - ref_sum[0]) <= 1e-3 * scale + 1e-9, k
        assert abs(synth.checksum(got)[1] - ref_sum[1]) <= 1e-3 * scale + 1e-9, k
        sl = got.reshape(-1)[:: max(1, got.size // 499)][:499]
        ref = g[f"gslice_{tag}__" + k]
        worst = max(worst, float(np.abs(sl - ref).max() / (np.abs(ref).max() + 1e-12)))
        np.testing.assert_allclose(sl, ref, rtol=2e-3, atol=1e-7 + 2e-4 * np.abs(ref).max(), err_msg=k)
    print(f"sh {tag}: worst relative gradient-slice error {worst:.2e}")


@pytest.mark.parametrize("deg", [2, 3])
def test_sh_module_call_vs_reference_forward(deg):
    """__call__(x [P, 3 + 1]) -> [P, 3 B + 1], raw coefficients then sigma, against the reference module.  Bound: 8 x the reference's own
    fp32 error against fp64 on these inputs (fwd_err in the fixture), taken against the fp64 restatement; the reference's fp32 output
    itself then lies within 9 x."""
    g = np.load(os.path.join(G, "sh_dense_fwd.npz"))
    m = _model(torch.float32, int(g[f"seed_{deg}"]), deg).eval()
    out = m(_dev(g["x"]), sigma_noise=_dev(g["sigma_noise"]))
    B, err = (deg + 1) ** 2, float(g[f"fwd_err_{deg}"])
    assert tuple(out.shape) == (257, 3 * B + 1)
    ref64 = R.module_forward(SW.make_sh_weights(int(g[f"seed_{deg}"]), deg), SW.SH_CFG, g["x"], g["sigma_noise"])
    e64 = float((out.double().cpu() - ref64).abs().max())
    e32 = float(np.abs(out.cpu().numpy() - g[f"out_{deg}"]).max())
    print(f"deg {deg}: against fp64 {e64:.3e}, against the reference's fp32 {e32:.3e}, reference fp32 error {err:.3e}")
    assert e64 <= 8 * err and e32 <= 9 * err
    sig = m(_dev(g["x"][:, :3]), sigma_only=True)
    assert tuple(sig.shape) == (257, 1) and float(np.abs(sig.cpu().numpy() - g[f"sigma_only_{deg}"]).max()) <= 9 * err
    with pytest.raises(Exception, match="Unexpected input shape"):
        m(torch.zeros(4, 7, device="cuda"))


@pytest.mark.parametrize("fine", [0, 16])
def test_autograd_bridge_fills_the_same_gradient_and_adam_moves_every_coefficient_row(fine):
    from switch_nerf_amd.rendering import render_rays
    N, S, seed = 37, 24, 4030
    rays, img, rgbs = synth.make_rays(4031, N, SW.SH_CFG["appearance_count"])
    a, b = _model(torch.float32, seed), _model(torch.float32, seed)
    a.grad_step(_dev(rgbs), _dev(rays), _dev(img), S, 1000, perturb=0.0, fine_samples=fine)
    opt = torch.optim.Adam(b.trainable_parameters(), lr=5e-4)
    res, _ = render_rays(b, None, _dev(rays), _dev(img), _hp(S, fine), None, None, True, True, False)
    typ = "fine" if fine else "coarse"
    assert set(res) == {f"rgb_{typ}", "gate_loss_coarse", f"depth_{typ}", f"depth_variance_{typ}"} | ({"gate_loss_fine"} if fine else set())
    loss = torch.nn.functional.mse_loss(res[f"rgb_{typ}"], _dev(rgbs))
    loss.backward()
    assert torch.equal(b.flat_param.grad, a.grad), (b.flat_param.grad - a.grad).abs().max().item()
    ga, gb = a.grad_dict(), b._to_ref_layout(b._views(b.flat_param.grad))
    assert all(torch.equal(ga[k], gb[k]) for k in ga)
    before = b.p["color.w"].clone()
    opt.step()
    assert ((b.p["color.w"] - before).abs().sum(1) > 0).all() and b.p["color.w"].shape[0] == 27
    with pytest.raises(NotImplementedError, match="sh_deg"):
        render_rays(b, None, _dev(rays), _dev(img), _hp(S, fine, deg=3), None, None, True, True, False)
    with pytest.raises(NotImplementedError, match="sh_deg"):
        render_rays(b, None, _dev(rays), _dev(img), _hp(S, fine, deg=None), None, None, True, True, False)


def test_evaluation_chunked_equals_unchunked_and_point_outputs():
    """A ragged last model chunk (37 x 24 = 888 points in chunks of 500) gives the unchunked result bit for bit, coarse and hierarchical;
    return_pts_rgb / return_sigma hand out the heads' own rgb and sigma; the colour is the restatement's on the pass's coefficients."""
    from switch_nerf_amd.rendering import render_rays
    N, S = 37, 24
    rays, img, _ = synth.make_rays(4041, N, SW.SH_CFG["appearance_count"])
    m = _model(torch.float32, 4040).eval()
    for fine in (0, 16):
        typ = "fine" if fine else "coarse"
        a, _ = render_rays(m, None, _dev(rays), _dev(img), _hp(S, fine, chunk=500, return_pts_rgb=True, return_sigma=True), None, None, True, True, False)
        a = {k: v.clone() for k, v in a.items()}
        b, _ = render_rays(m, None, _dev(rays), _dev(img), _hp(S, fine, chunk=1 << 20, return_pts_rgb=True, return_sigma=True), None, None, True, True, False)
        assert set(a) == set(b) and f"rgb_{typ}" in a and "sigma_coarse" in a and "pts_rgb_coarse" in a
        for k in a:
            assert torch.equal(a[k], b[k]), k
    c = m.forward_rays(_dev(rays), _dev(img), S, 500, 0.0, None, None, training=False)
    assert torch.equal(a["pts_rgb_coarse"].reshape(-1, 3), c["raw"][:, :3]) and torch.equal(a["sigma_coarse"].reshape(-1), c["raw"][:, 3])
    # the colour of the pass = sigmoid(eval_sh(coefficients of the points, the RAY's direction rays[:, 3:6]))
    t = torch.linspace(0, 1, S)
    z = torch.from_numpy(rays[:, 6:7]) * (1 - t) + torch.from_numpy(rays[:, 7:8]) * t
    pts = (torch.from_numpy(rays[:, None, :3]) + torch.from_numpy(rays[:, None, 3:6]) * z[:, :, None]).reshape(-1, 3)
    x = torch.cat([pts, torch.from_numpy(img).float().repeat_interleave(S)[:, None]], 1).numpy()
    out = R.module_forward(SW.make_sh_weights(4040, 2), SW.SH_CFG, x)
    rgb = torch.sigmoid(R.eval_sh(2, out[:, :27].view(-1, 3, 9), torch.from_numpy(rays[:, 3:6]).double().repeat_interleave(S, 0)))
    assert float((c["raw"][:, :3].double().cpu() - rgb).abs().max()) <= 1e-4          # (the project's rgb tolerance)


def test_bf16_step_stays_within_the_rgb_bound_of_fp32():
    """The project's bound on a 16-bit step's rgb against the fp32 step (2^-7, tests/test_fullsize_gpu.py)."""
    g = np.load(os.path.join(G, "sh_dense_train.npz"))
    N, S = int(g["N"]), int(g["S"])
    rays, img, rgbs = synth.make_rays(int(g["rays_seed"]), N, SW.SH_CFG["appearance_count"])
    a, b = _model(torch.float32, int(g["seed"])), _model(torch.bfloat16, int(g["seed"]))
    ra = a.train_step(_dev(rgbs), _dev(rays), _dev(img), S, 1000, perturb=0.0, optimizer_step=False)["rgb"].clone()
    st = b.train_step(_dev(rgbs), _dev(rays), _dev(img), S, 1000, perturb=0.0, optimizer_step=True)
    d = (st["rgb"] - ra).abs().max().item()
    print(f"bf16 against fp32 rgb: {d:.3e}")
    assert d <= 2.0 ** -7
    assert torch.isfinite(b.grad).all() and b.g["color.w"].abs().sum(1).min().item() > 0


def test_graph_capture_and_background_refuse_sh():
    from switch_nerf_amd import graph
    from switch_nerf_amd.background import BackgroundScene
    from switch_nerf_amd.dense import DenseNeRF
    m = _model(torch.float32, 1)
    rays, img, rgbs = synth.make_rays(2, 8, SW.SH_CFG["appearance_count"])
    with pytest.raises(NotImplementedError, match="sh_deg"):
        graph.GraphedTrainStep(m, _dev(rgbs), _dev(rays), _dev(img), 8, 64)
    with pytest.raises(NotImplementedError, match="sh_deg"):
        graph.GraphedRender(m, _dev(rays), _dev(img), 8, 64)
    bg = DenseNeRF(dict(SW.SH_CFG, pos_dir_dim=2, xyz_dim=4), dtype=torch.float32)
    with pytest.raises(NotImplementedError, match="sh_deg"):
        BackgroundScene(m, bg)
