"""The two-network cascade (switch_nerf_amd/cascade.py, --use_cascade) in fp32 mode against the reference's own Cascade
(tests/golden/cascade_dense.npz, scripts/gen_golden_cascade.py), at the tolerances of test_hierarchical_train_step_vs_reference_golden_fp32:
rgb atol 1e-4, depth rtol 1e-4 / atol 1e-5, loss rtol 1e-5, gradient checksums 1e-3 of the absolute-sum checksum, gradient slices
rtol 2e-3 + 2e-4 of the slice's maximum; z_union within 1e-5; parameters after two Adam steps within test_mega_train_gpu.py's 2e-5.
SwitchNeRF halves are refused."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
N_SLICE = 499


def dev():
    return torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _sl(a):
    a = np.asarray(a).reshape(-1)
    return a[:: max(1, a.size // N_SLICE)][:N_SLICE]


def dense_cascade(g=None, dtype=torch.float32, fine=True, seed=None):
    from switch_nerf_amd.cascade import Cascade
    from switch_nerf_amd.dense import DenseNeRF
    seed = int(g["seed"]) if seed is None else seed
    halves = []
    for i in range(2 if fine else 1):
        m = DenseNeRF(synth.DENSE, dtype=dtype, lr=5e-4)
        m.load_state_dict(synth.make_dense_weights(seed + i, synth.DENSE))
        halves.append(m)
    return Cascade(halves[0], halves[1] if fine else None)


def hparams(S, F, perturb=0.0, chunk=65536, **kw):
    h = Namespace(coarse_samples=S, fine_samples=F, model_chunk_size=chunk, perturb=perturb, use_sigma_noise=False, sigma_noise_std=0.0,
                  use_cascade=True, moe_return_gates=False, return_sigma=False)
    h.__dict__.update(kw)
    return h


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(G, "cascade_dense.npz"))


def _grads(cas):
    out = {}
    for name, half in (("coarse", cas.coarse), ("fine", cas.fine)):
        out.update({f"{name}.{k}": v for k, v in half.grad_dict().items()})
    return out


@pytest.mark.parametrize("case", ["p0", "p1"])
def test_cascade_train_step_vs_reference_golden_fp32(g, case):
    cas = dense_cascade(g)
    N, S, F = int(g["N"]), int(g["S"]), int(g["F"])
    perturb = 0.0 if case == "p0" else 1.0
    pr = t(g["p1_perturb_rand"]) if perturb else None
    fu = t(g["p1_fine_u"]) if perturb else None
    st = cas.grad_step(t(g["rgbs"]), t(g["rays"]), t(g["image_indices"]), S, N * S, perturb, pr, fine_samples=F, fine_u=fu)
    torch.cuda.synchronize()
    zu = st["ctx_fine"]["z_union"].cpu().numpy()
    print(f"({case}) rgb_fine err {np.abs(st['rgb'].cpu().numpy() - g[case + '_rgb_fine']).max():.3e}, rgb_coarse err "
          f"{np.abs(st['rgb_coarse'].cpu().numpy() - g[case + '_rgb_coarse']).max():.3e}, z_union err {np.abs(zu - g[case + '_z_union']).max():.3e}, "
          f"loss {st['loss'].item():.8f} / {float(g[case + '_loss']):.8f}")
    assert zu.shape == (N, S + F)
    np.testing.assert_allclose(zu, g[case + "_z_union"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(st["rgb"].cpu().numpy(), g[case + "_rgb_fine"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(st["rgb_coarse"].cpu().numpy(), g[case + "_rgb_coarse"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(st["depth"].cpu().numpy(), g[case + "_depth_fine"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(st["ctx_fine"]["depth_variance"].cpu().numpy(), g[case + "_depth_variance_fine"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(st["loss"].item(), float(g[case + "_loss"]), rtol=1e-5)
    assert float(st["gate_loss"].item()) == 0.0
    assert set(st) >= {"loss", "photo_loss", "coarse_loss", "psnr", "rgb", "rgb_coarse", "depth", "depth_variance", "gate_loss"}
    every = int(g["every_p0"] if case == "p0" else g["every_p1"])
    gd, worst = _grads(cas), 0.0
    assert sorted(gd) == sorted(str(k) for k in g["param_names"])
    for k, v in gd.items():
        got = v.cpu().numpy()
        ref_sum, ref = g[f"{case}_gsum__{k}"], g[f"{case}_gslice__{k}"]
        scale = max(1e-12, float(ref_sum[1]))
        assert abs(synth.checksum(got)[0] - ref_sum[0]) <= 1e-3 * scale + 1e-9, k
        assert abs(synth.checksum(got)[1] - ref_sum[1]) <= 1e-3 * scale + 1e-9, k
        sl = _sl(got)[::every]
        worst = max(worst, float(np.abs(sl - ref).max() / (np.abs(ref).max() + 1e-12)))
        np.testing.assert_allclose(sl, ref, rtol=2e-3, atol=1e-7 + 2e-4 * np.abs(ref).max(), err_msg=k)
    print(f"({case}) worst relative gradient-slice error {worst:.2e}")


def _check_params(cas, g, step):
    names, off = [str(k) for k in g["param_names"]], g["adam_offsets"]
    now = dict(cas.named_parameters())
    worst = 0.0
    for i, k in enumerate(names):
        ref = g[f"adam_p{step}_slices"][off[i]:off[i + 1]]
        ev = int(g["every_adam"])
        got = _sl(now[k].cpu().numpy())[::ev]
        g1 = g["p0_gslice__" + k][::ev]
        small = np.abs(g1) < 1e-7 * max(1e-12, np.abs(g["p0_gslice__" + k]).max())      # update direction ill-defined there
        worst = max(worst, float(np.abs(np.where(small, ref, got) - ref).max()))
        np.testing.assert_allclose(np.where(small, ref, got), ref, rtol=0, atol=2e-5, err_msg=f"step {step} {k}")
    print(f"step {step}: worst parameter error {worst:.2e}")


def test_cascade_two_adam_steps_vs_reference_and_autograd_path(g):
    """train_step twice (one Adam step per half, each its own count) against the reference's torch.optim.Adam; then the same two steps
    through render_rays in training mode under autograd with torch.optim.Adam over both leaves: train_step's parameters again."""
    from switch_nerf_amd import rendering
    N, S, F = int(g["N"]), int(g["S"]), int(g["F"])
    rays, img, rgbs = t(g["rays"]), t(g["image_indices"]), t(g["rgbs"])
    cas = dense_cascade(g)
    for step in (1, 2):
        st = cas.train_step(rgbs, rays, img, S, N * S, 0.0, fine_samples=F)
        np.testing.assert_allclose(st["loss"].item(), float(g[f"adam_loss{step}"]), rtol=1e-5)
        _check_params(cas, g, step)
    assert cas.coarse.step_count == 2 and cas.fine.step_count == 2
    auto = dense_cascade(g).train()
    leaves = auto.trainable_parameters()
    assert len(leaves) == 2 and leaves[0] is auto.coarse.flat_param and leaves[1] is auto.fine.flat_param
    opt = torch.optim.Adam(leaves, lr=5e-4)
    for step in (1, 2):
        opt.zero_grad()
        res, _ = rendering.render_rays(auto, None, rays, img, hparams(S, F), None, None, False, True, False)
        assert res["rgb_fine"].grad_fn is not None and res["rgb_coarse"].grad_fn is not None and res["gate_loss_fine"].grad_fn is not None
        loss = (torch.nn.functional.mse_loss(res["rgb_fine"], rgbs) + torch.nn.functional.mse_loss(res["rgb_coarse"], rgbs)) / 2
        loss.backward()
        assert all(p.grad is not None and bool(p.grad.any()) for p in leaves)
        opt.step()
        _check_params(auto, g, step)
    for a, b in zip(cas.halves(), auto.halves()):
        d = (a.flat - b.flat).abs().max().item()
        print(f"train_step vs autograd + torch Adam: max parameter difference {d:.2e}")
        assert d <= 1e-6          # (the same HIP gradients; torch's Adam and swn_adam_step round their update differently)


def test_cascade_render_rays_eval_keys_and_values(g):
    from switch_nerf_amd import rendering
    N, S, F = int(g["N"]), int(g["S"]), int(g["F"])
    rays, img = t(g["rays"]), t(g["image_indices"])
    cas = dense_cascade(g).eval()
    res, bg = rendering.render_rays(cas, None, rays, img, hparams(S, F, perturb=1.0), None, None, True, True, False)
    # (the dense halves report their all-zero gate losses like every dense render here; the reference has no such key without MoE)
    assert bg is False and sorted(res) == sorted([str(k) for k in g["eval_keys"]] + ["gate_loss_coarse", "gate_loss_fine"])
    assert "depth_coarse" not in res
    for k in ("rgb_coarse", "rgb_fine"):
        np.testing.assert_allclose(res[k].cpu().numpy(), g["eval_" + k], rtol=0, atol=1e-4)
    for k in ("depth_fine", "depth_variance_fine"):
        np.testing.assert_allclose(res[k].cpu().numpy(), g["eval_" + k], rtol=1e-4, atol=1e-5)
    res_s, _ = rendering.render_rays(cas, None, rays, img, hparams(S, F, return_sigma=True), None, None, False, False, False)
    assert res_s["sigma_fine"].shape == (N, S + F) and res_s["sigma_coarse"].shape == (N, S) and "depth_fine" not in res_s
    cas0 = dense_cascade(g, fine=False).eval()
    res0, _ = rendering.render_rays(cas0, None, rays, img, hparams(S, 0), None, None, True, True, False)
    assert sorted(res0) == sorted([str(k) for k in g["eval0_keys"]] + ["gate_loss_coarse"])
    np.testing.assert_allclose(res0["rgb_coarse"].cpu().numpy(), g["eval0_rgb_coarse"], rtol=0, atol=1e-4)


def test_cascade_levels_state_and_call(g):
    """The fine level IS the fine half on z_union (its own forward_rays gives the same bits), every coarse depth is in the union, the
    state round-trips through the coarse. / fine. layout, __call__ equals each half's own, coarse_photo = False seeds no coarse gradient."""
    from switch_nerf_amd import rendering
    N, S, F = int(g["N"]), int(g["S"]), int(g["F"])
    rays, img, rgbs = t(g["rays"]), t(g["image_indices"]), t(g["rgbs"])
    cas = dense_cascade(g).eval()
    res, _ = rendering.render_rays(cas, None, rays, img, hparams(S, F, moe_return_gates=True), None, None, True, True, False)
    assert not any(k.startswith("moe_gates") for k in res)           # (no router in a dense half)
    c, cf = cas.forward_cascade(rays, img, S, F, N * S, training=False)
    own = cas.fine.forward_rays(rays, img, S + F, N * S, training=False, z_in=cf["z_union"], tag="f")
    assert torch.equal(own["raw"], cf["raw"]) and torch.equal(own["rgb"], res["rgb_fine"])
    zu = cf["z_union"]
    assert bool((zu[:, 1:] >= zu[:, :-1]).all())
    assert all(bool(torch.isin(c["z"][i], zu[i]).all()) for i in range(0, N, 7))
    sd = cas.state_dict()
    assert all(k.startswith(("coarse.", "fine.")) for k in sd)
    assert sorted(k[7:] for k in sd if k.startswith("coarse.")) == sorted(cas.coarse.state_dict()) == sorted(k[5:] for k in sd if k.startswith("fine."))
    other = dense_cascade(g, seed=7)
    other.load_state_dict({k: v.clone() for k, v in sd.items()})
    assert torch.equal(other.coarse.flat, cas.coarse.flat) and torch.equal(other.fine.flat, cas.fine.flat)
    assert not torch.equal(cas.coarse.flat, cas.fine.flat)
    x = torch.cat([rays[:, :6], img.view(-1, 1).float()], 1)
    for use_coarse, half in ((True, cas.coarse), (False, cas.fine)):
        assert torch.equal(cas(use_coarse, x), half(x)) and torch.equal(cas(use_coarse, x[:, :3], True), half(x[:, :3], True))
    cas.train()
    st = cas.grad_step(rgbs, rays, img, S, N * S, 0.0, fine_samples=F, coarse_photo=False)
    assert st["loss"].item() == st["photo_loss"].item() and not bool(cas.coarse.grad.any()) and bool(cas.fine.grad.any())
    with pytest.raises(ValueError, match="needs a fine half"):
        rendering.render_rays(dense_cascade(g, fine=False).train(), None, rays, img, hparams(S, F), None, None)


def test_cascade_bf16_loss_falls():
    N, S, F = 256, 128, 192
    rays, img, rgbs = (t(a) for a in synth.make_rays(31, N))
    cas = dense_cascade(dtype=torch.bfloat16, seed=171)
    losses = [cas.train_step(rgbs, rays, img, S, 8192, 0.0, fine_samples=F)["loss"].item() for _ in range(6)]
    print(losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_cascade_fp16_one_scaler_and_steps_together():
    """IEEE half: one LossScaler for both halves, and both skip - or take - every step together."""
    from switch_nerf_amd import _lib
    N, S, F = 64, 32, 16
    rays, img, rgbs = (t(a) for a in synth.make_rays(33, N))
    try:
        cas = dense_cascade(dtype=torch.float16, seed=171)
        assert cas.loss_scaler is not None and cas.coarse.loss_scaler is cas.fine.loss_scaler is cas.loss_scaler
        scales, losses = [], []
        for _ in range(4):
            losses.append(cas.train_step(rgbs, rays, img, S, N * S, 0.0, fine_samples=F)["loss"].item())
            scales.append(cas.loss_scaler.scale)
            assert cas.coarse.step_count == cas.fine.step_count
        print("fp16", losses, scales, cas.coarse.step_count)
        assert all(np.isfinite(losses))
        assert cas.coarse.step_count + round(np.log2(65536.0 / scales[-1])) == 4      # every step was taken or halved the one scale
    finally:
        _lib.use_half("bf16")


def test_cascade_refusals(g):
    from switch_nerf_amd import rendering
    from switch_nerf_amd.cascade import Cascade
    from switch_nerf_amd.dense import DenseNeRF
    from switch_nerf_amd.model import SwitchNeRF
    N, S, F = 8, 32, 16
    rays, img, rgbs = (t(a) for a in synth.make_rays(5, N))
    cas = dense_cascade(g)
    plain = cas.coarse
    with pytest.raises(NotImplementedError, match="Cascade"):
        rendering.render_rays(plain, None, rays, img, hparams(S, F), None, None)
    with pytest.raises(NotImplementedError, match="use_cascade is off"):
        rendering.render_rays(cas, None, rays, img, hparams(S, F, use_cascade=False), None, None)
    with pytest.raises(NotImplementedError, match="background model"):
        rendering.render_rays(cas, cas.fine, rays, img, hparams(S, F), None, None)
    with pytest.raises(NotImplementedError, match="device noise"):
        rendering.render_rays(cas, None, rays, img, hparams(S, F, device_noise_seed=3), None, None)
    with pytest.raises(NotImplementedError, match="mip path"):
        cas.forward_mip(rays, None, img, S, F, 1024)
    with pytest.raises(NotImplementedError, match="split=True"):
        cas.grad_step(rgbs, rays, img, S, N * S, fine_samples=F, split=True)
    with pytest.raises(NotImplementedError, match="routing_override"):
        cas.grad_step(rgbs, rays, img, S, N * S, fine_samples=F, routing_override=torch.zeros(1))
    with pytest.raises(NotImplementedError, match="parallelism"):
        cas.train_step(rgbs, rays, img, S, N * S, fine_samples=F, grad_allreduce=lambda v: 1.0)
    with pytest.raises(NotImplementedError, match="parallelism"):
        cas.set_expert_parallel(None)
    with pytest.raises(NotImplementedError, match="device noise"):
        cas.set_device_noise(1)
    cas.fine.set_device_noise(1)
    with pytest.raises(NotImplementedError, match="device noise"):
        cas.forward_cascade(rays, img, S, F, N * S)
    cas.fine.set_device_noise(None)
    for flag in ("graph_train", "graph_eval"):
        setattr(cas.coarse, flag, True)
        with pytest.raises(NotImplementedError, match="graph capture"):
            cas.forward_cascade(rays, img, S, F, N * S)
        setattr(cas.coarse, flag, False)
    from switch_nerf_amd.graph import GraphedRender, GraphedRenderTrain, GraphedTrainStep
    with pytest.raises(NotImplementedError, match="GraphedTrainStep: graph capture of a two-network Cascade"):
        GraphedTrainStep(cas, rgbs, rays, img, S, N * S)
    with pytest.raises(NotImplementedError, match="GraphedRender: graph capture of a two-network Cascade"):
        GraphedRender(cas, rays, img, S, N * S, F)
    with pytest.raises(NotImplementedError, match="GraphedRenderTrain: graph capture of a two-network Cascade"):
        GraphedRenderTrain(cas, rays, img, S, F, N * S, 0.0, 0.0)
    from types import SimpleNamespace
    with pytest.raises(NotImplementedError, match="Mega-NeRF"):
        Cascade(SimpleNamespace(is_mega_nerf=True), None)
    with pytest.raises(NotImplementedError, match="sh_deg"):
        Cascade(DenseNeRF(dict(synth.DENSE, sh_deg=2, pos_dir_dim=0), dtype=torch.float32), None)
    moe = SwitchNeRF(synth.BUILDING, dtype=torch.float32)
    with pytest.raises(NotImplementedError, match="MoE halves"):
        Cascade(moe, None)
    with pytest.raises(NotImplementedError, match="MoE halves"):
        Cascade(cas.coarse, moe)
    with pytest.raises(ValueError, match="same cfg"):
        Cascade(cas.coarse, DenseNeRF(dict(synth.DENSE, layers=6), dtype=torch.float32))
    with pytest.raises(ValueError, match="compute dtype"):
        Cascade(cas.coarse, DenseNeRF(synth.DENSE, dtype=torch.bfloat16))


def test_no_state_leaks_into_a_plain_model(g):
    """A plain model rendered with use_cascade = False before and after a cascade step that uses it as the coarse half (the optimizer
    step held back) gives the same bits."""
    from switch_nerf_amd import rendering
    N, S, F = int(g["N"]), int(g["S"]), int(g["F"])
    rays, img, rgbs = t(g["rays"]), t(g["image_indices"]), t(g["rgbs"])
    cas = dense_cascade(g)
    plain = cas.coarse.eval()
    h = hparams(S, F, use_cascade=False)
    before, _ = rendering.render_rays(plain, None, rays, img, h, None, None)
    before = {k: v.clone() for k, v in before.items()}
    cas.train()
    cas.train_step(rgbs, rays, img, S, N * S, 1.0, fine_samples=F, optimizer_step=False)
    res, _ = rendering.render_rays(cas.eval(), None, rays, img, hparams(S, F), None, None)
    after, _ = rendering.render_rays(plain.eval(), None, rays, img, h, None, None)
    assert sorted(after) == sorted(before) and all(torch.equal(after[k], before[k]) for k in before)
