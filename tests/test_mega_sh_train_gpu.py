"""Training a Mega-NeRF whose cells use spherical-harmonics colour (switch_nerf_amd/mega.py, joint_training + sh_training: forward_points /
backward_points / train_step) against the REFERENCE's own MegaNeRF(.., True).train() around NeRF(rgb_dim = 3 B), its eval_sh + sigmoid, its
autograd and torch.optim.Adam (tests/golden/mega_sh_train.npz, mega_sh_train_module_d{0,2,4}.npz; scripts/gen_golden_mega_sh_train.py).
Three two-layer cells of layer_dim 256, weights from tests/sh_weights.make_sh_weights.

Bounds are those tests/test_mega_train_gpu.py takes from tests/test_dense_gpu.py: rgb 1e-4 absolute, depth 1e-4 relative + 1e-5, loss 1e-5
relative, gradient checksums 1e-3 of scale, slices 2e-3 relative + 2e-4 max|ref| + 1e-7, Adam 2e-5 absolute wherever the step-1 gradient is
not below 1e-7 of its maximum, and the bf16-vs-fp32 bars 3e-2 rgb, 2e-2 loss, 0.15 relative gradient.  No point of the fixtures lies on a
membership decision (asserted by the generator and by tests/test_mega_sh_train_cpu.py), so every ray and every gradient is compared."""
import os

import numpy as np
import pytest
import torch

import sh_weights as SW
import synth

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
N_SLICE = 499


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _load(name):
    return np.load(os.path.join(G, name + ".npz"))


def _cfg(g):
    return {k[5:]: (tuple(int(v) for v in g[k]) if g[k].ndim else int(g[k])) for k in g.files if k.startswith("cfg__")}


def _mega(g, margin, dtype=torch.float32, n_cells=3, **kw):
    from switch_nerf_amd.mega import MegaNeRF
    cfg, deg = _cfg(g), int(g["deg"])
    sds = [SW.make_sh_weights(int(g["seed"]) + i, deg, cfg) for i in range(n_cells)]
    for sd, ref in zip(sds, g["sd_checksums"]):
        np.testing.assert_allclose(np.sum([synth.checksum(v) for v in sd.values()], 0), ref, rtol=1e-12)
    kw = dict(dict(joint_training=True, sh_training=True), **kw)
    return MegaNeRF.from_state_dicts(sds, g["centroids"][:n_cells], None, boundary_margin=margin, dtype=dtype, **kw)


def _sl(a):
    a = np.asarray(a).reshape(-1)
    return a[:: max(1, a.size // N_SLICE)][:N_SLICE]


def _check_grads(gd, ref_of, what, n=39):
    worst = 0.0
    assert len(gd) == n
    for k, t in gd.items():
        got = t.cpu().numpy()
        ref_sum, ref = ref_of(k)
        scale = max(1e-12, float(ref_sum[1]))
        assert abs(synth.checksum(got)[0] - ref_sum[0]) <= 1e-3 * scale + 1e-9, k
        assert abs(synth.checksum(got)[1] - ref_sum[1]) <= 1e-3 * scale + 1e-9, k
        sl = _sl(got)
        worst = max(worst, float(np.abs(sl - ref).max() / (np.abs(ref).max() + 1e-12)))
        np.testing.assert_allclose(sl, ref, rtol=2e-3, atol=1e-7 + 2e-4 * np.abs(ref).max(), err_msg=k)
    print(f"{what}: worst relative gradient-slice error {worst:.2e}")


@pytest.mark.parametrize("case", ["a", "b"])
def test_mega_sh_train_step_vs_reference_golden_fp32(case):
    """(a) 64 rays x 32 samples, (b) the same rays with 16 fine samples: rgb, depth, loss and every cell's gradient."""
    g = _load("mega_sh_train")
    m = _mega(g, float(g["margin"]))
    S, F = int(g["S"]), int(g["F"]) if case == "b" else 0
    st = m.train_step(_dev(g["rgbs"]), _dev(g["rays"]), _dev(g["image_indices"]), S, perturb=0.0, optimizer_step=False, fine_samples=F)
    print(f"({case}) members per cell {st['ctx']['counts']}" + (f", fine {st['ctx_fine']['counts']}" if F else "") + f"; reference {g[case + '_members'].tolist()}")
    print(f"({case}) rgb err {np.abs(st['rgb'].cpu().numpy() - g[case + '_rgb']).max():.3e}, loss {st['loss'].item():.8f} / {float(g[case + '_loss']):.8f}")
    assert st["ctx"]["counts"] == g[case + "_members"][0].tolist()
    np.testing.assert_allclose(st["rgb"].cpu().numpy(), g[case + "_rgb"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(st["depth"].cpu().numpy(), g[case + "_depth"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(st["loss"].item(), float(g[case + "_loss"]), rtol=1e-5)
    assert float(st["gate_loss"].item()) == 0.0
    assert set(st) >= {"loss", "photo_loss", "psnr", "rgb", "depth", "depth_variance", "gate_loss"}
    _check_grads(m.grad_dict(), lambda k: (g[f"{case}_gsum__{k}"], g[f"{case}_gslice__{k}"]), f"({case})")


@pytest.mark.parametrize("deg,tag,margin", [(2, "m100", 1.0), (2, "m115", 1.15), (0, "m115", 1.15), (4, "m115", 1.15)])
def test_mega_sh_forward_backward_points_vs_reference_golden_fp32(deg, tag, margin):
    """The module's own autograd through sigmoid(eval_sh(.)): one direction per point, sigma noise, a stored d_raw; hard and soft margin,
    the degree-0 double sigmoid, the widest rows."""
    g = _load(f"mega_sh_train_module_d{deg}")
    m = _mega(g, margin)
    for sub in m.sub_modules:
        sub.grad.zero_()
    ctx = m.forward_points(_dev(g["x"]), _dev(g["sigma_noise"]), "c", _dev(g["dirs"]), 1)
    out = ctx["out"].cpu().numpy()
    np.testing.assert_allclose(out[:, :3], g["raw_" + tag][:, :3], rtol=0, atol=1e-4)
    np.testing.assert_allclose(out[:, 3], g["raw_" + tag][:, 3], rtol=1e-4, atol=1e-4)
    m.backward_points(ctx, _dev(g["d_raw"]))
    names, off = [str(n) for n in g["param_names"]], g["offsets"]
    idx = {n: i for i, n in enumerate(names)}
    _check_grads(m.grad_dict(), lambda k: (g[tag + "_gsums"][idx[k]], g[tag + "_gslices"][off[idx[k]]:off[idx[k] + 1]]), f"d{deg} {tag}")


def test_mega_sh_adam_two_steps_and_empty_cells_vs_reference_golden():
    """(c) two Adam steps; the second on rays whose every sample lies in cell 0: cells 1 and 2 have a zero gradient, not a missing one,
    and still move (momentum), as under the reference's one torch.optim.Adam."""
    g = _load("mega_sh_train")
    m = _mega(g, float(g["margin"]))
    m.lr = m.base_lr = float(g["lr"])
    names, off = [str(n) for n in g["param_names"]], g["c_offsets"]
    rgbs, img = _dev(g["rgbs"]), _dev(g["image_indices"])
    after = {}
    for step, rays in ((1, g["rays"]), (2, g["rays_cell0"])):
        st = m.train_step(rgbs, _dev(rays), img, int(g["S"]), perturb=0.0, optimizer_step=True)
        if step == 2:
            assert st["ctx"]["counts"] == [int(g["N"]) * int(g["S"]), 0, 0]
            gd = m.grad_dict()
            assert len(gd) == 39
            for k, t in gd.items():
                if not k.startswith("sub_modules.0."):
                    assert not t.any(), k
        after[step] = {k: v.cpu().numpy() for k, v in m.named_parameters()}
        worst = 0.0
        for i, k in enumerate(names):
            ref = g[f"c_p{step}_slices"][off[i]:off[i + 1]]
            got = _sl(after[step][k])[::2]
            g1 = g["a_gslice__" + k][::2]
            small = np.abs(g1) < 1e-7 * max(1e-12, np.abs(g["a_gslice__" + k]).max())
            worst = max(worst, float(np.abs(np.where(small, ref, got) - ref).max()))
            np.testing.assert_allclose(np.where(small, ref, got), ref, rtol=0, atol=2e-5, err_msg=f"step {step} {k}")
        print(f"step {step}: worst parameter error {worst:.2e}")
    assert m.step_count == 2 and all(s.step_count == 2 for s in m.sub_modules)
    for k in names:
        if not k.startswith("sub_modules.0.") and np.abs(g["a_gslice__" + k]).max() > 0:
            assert not np.array_equal(after[1][k], after[2][k]), k      # moved without a point


def test_mega_sh_grad_step_is_deterministic_and_optimizer_step_false_changes_nothing():
    g = _load("mega_sh_train")
    m = _mega(g, 1.15)
    before = {k: v.clone() for k, v in m.named_parameters()}
    args = (_dev(g["rgbs"]), _dev(g["rays"]), _dev(g["image_indices"]), int(g["S"]))
    grads = []
    for _ in range(2):
        m.grad_step(*args, perturb=0.0, fine_samples=int(g["F"]))
        grads.append({k: v.clone() for k, v in m.grad_dict().items()})
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k
    for i in range(3):
        assert grads[0][f"sub_modules.{i}.rgb.weight"].any()
    m.train_step(*args, perturb=0.0, optimizer_step=False)
    for k, v in m.named_parameters():
        assert torch.equal(v, before[k]), k
    assert m.step_count == 0


def test_mega_sh_train_bf16_close_to_fp32():
    g = _load("mega_sh_train")
    outs = {}
    for dt in (torch.float32, torch.bfloat16):
        m = _mega(g, float(g["margin"]), dt)
        st = m.train_step(_dev(g["rgbs"]), _dev(g["rays"]), _dev(g["image_indices"]), int(g["S"]), perturb=0.0, optimizer_step=False,
                          fine_samples=int(g["F"]))
        outs[dt] = (st["rgb"].float().cpu().numpy(), st["loss"].item(), {k: v.cpu().numpy() for k, v in m.grad_dict().items()})
    a, b = outs[torch.float32], outs[torch.bfloat16]
    assert np.abs(a[0] - b[0]).max() < 3e-2
    assert abs(a[1] - b[1]) < 2e-2 * abs(a[1])
    for k in a[2]:
        den = np.abs(a[2][k]).max() + 1e-12
        assert np.abs(a[2][k] - b[2][k]).max() / den < 0.15, k


def test_mega_sh_eval_after_training_equals_the_inference_model():
    """One optimizer step, then eval(): render_rays with hparams.sh_deg = 2 is bit-equal to an inference MegaNeRF built from state_dicts()
    (and refuses the model while it is in training mode)."""
    from argparse import Namespace
    from switch_nerf_amd.mega import MegaNeRF
    from switch_nerf_amd.rendering import render_rays
    g = _load("mega_sh_train")
    m = _mega(g, 1.15)
    rays, img = _dev(g["rays"]), _dev(g["image_indices"])
    m.train_step(_dev(g["rgbs"]), rays, img, int(g["S"]), perturb=0.0)
    h = Namespace(coarse_samples=int(g["S"]), fine_samples=int(g["F"]), model_chunk_size=1000, perturb=1.0, use_sigma_noise=True,
                  sigma_noise_std=1.0, sh_deg=2)
    with pytest.raises(NotImplementedError, match="evaluation mode"):
        render_rays(m, None, rays, img, h, None, None, True, True, False)
    m.eval()
    assert not m.training and not any(s.training for s in m.sub_modules)
    twin = MegaNeRF.from_state_dicts([{k: v.cpu() for k, v in sd.items()} for sd in m.state_dicts()], g["centroids"], None, boundary_margin=1.15)
    assert not twin.joint_training and twin.sh_deg == 2
    a, _ = render_rays(m, None, rays, img, h, None, None, True, True, False)
    b, _ = render_rays(twin, None, rays, img, h, None, None, True, True, False)
    assert set(a) == set(b) == {"rgb_fine", "depth_fine", "depth_variance_fine"}
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_one_cell_mega_sh_agrees_with_the_dense_sh_model():
    """A one-cell MegaNeRF at degree 2 against DenseNeRF(sh_deg = 2).train_step on the same rays, coarse + fine: the per-row heads
    (swn_heads_coef_*, the basis behind the blend) and the folded heads (swn_heads_sh_*, the basis folded into the weights per ray) must
    give the same rgb, loss and gradients within the fp32 bounds above."""
    from switch_nerf_amd.dense import DenseNeRF
    g = _load("mega_sh_train")
    cfg, S, F = _cfg(g), int(g["S"]), int(g["F"])
    m = _mega(g, 1.0, n_cells=1)
    d = DenseNeRF(dict(cfg, sh_deg=2), dtype=torch.float32)
    d.load_state_dict(SW.make_sh_weights(int(g["seed"]), 2, cfg))
    rgbs, rays, img = _dev(g["rgbs"]), _dev(g["rays"]), _dev(g["image_indices"])
    a = m.train_step(rgbs, rays, img, S, perturb=0.0, optimizer_step=False, fine_samples=F)
    b = d.train_step(rgbs, rays, img, S, rays.shape[0] * S, perturb=0.0, optimizer_step=False, fine_samples=F)
    np.testing.assert_allclose(a["rgb"].cpu().numpy(), b["rgb"].cpu().numpy(), rtol=0, atol=1e-4)
    np.testing.assert_allclose(a["depth"].cpu().numpy(), b["depth"].cpu().numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(a["loss"].item(), b["loss"].item(), rtol=1e-5)
    ref = {"sub_modules.0." + k: v.cpu().numpy() for k, v in d.grad_dict().items()}
    _check_grads(m.grad_dict(), lambda k: (synth.checksum(ref[k]), _sl(ref[k])), "one cell vs dense", n=13)
