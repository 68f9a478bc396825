"""Training the Mega-NeRF spatial-cell model through its cells (switch_nerf_amd/mega.py, joint_training: forward_points / backward_points /
train_step) against the REFERENCE's own MegaNeRF under its own autograd and torch.optim.Adam (tests/golden/mega_train.npz,
mega_train_module.npz; scripts/gen_golden_mega_train.py).  Three two-layer cells of layer_dim 256, the weights of mega_fg.npz.

Bounds are those of tests/test_dense_gpu.py: its reference test (rgb 1e-4 absolute, depth 1e-4 relative + 1e-5, loss 1e-5 relative,
gradient checksums 1e-3 of scale, slices 2e-3 relative + 2e-4 max|ref| + 1e-7), its Adam rule (2e-5 absolute wherever the step-1
gradient is not below 1e-7 of its maximum) and its bf16-vs-fp32 bars (3e-2 rgb, 2e-2 loss, 0.15 relative gradient).  No point of the
fixtures lies on a membership decision (asserted by the generator and by tests/test_mega_train_cpu.py), so every ray and every gradient
is compared."""
import os

import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
N_SLICE = 499


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _load(name):
    return np.load(os.path.join(G, name + ".npz"))


def _mega(g, margin, dtype=torch.float32, joint=True):
    from switch_nerf_amd.mega import MegaNeRF
    cfg = {k[5:]: (tuple(int(v) for v in g[k]) if g[k].ndim else int(g[k])) for k in g.files if k.startswith("cfg__")}
    sds = [synth.make_dense_weights(int(g["seed"]) + i, cfg) for i in range(len(g["centroids"]))]
    for sd, ref in zip(sds, g["sd_checksums"]):
        np.testing.assert_allclose(np.sum([synth.checksum(v) for v in sd.values()], 0), ref, rtol=1e-12)
    return MegaNeRF.from_state_dicts(sds, g["centroids"], cfg, boundary_margin=margin, dtype=dtype, joint_training=joint)


def _sl(a):
    a = np.asarray(a).reshape(-1)
    return a[:: max(1, a.size // N_SLICE)][:N_SLICE]


def _check_grads(m, ref_of, what):
    """Every cell's gradient against (checksum, slice) = ref_of(key): checksums within 1e-3 of scale, slices rtol 2e-3 / atol 2e-4 max|ref| + 1e-7."""
    worst = 0.0
    gd = m.grad_dict()
    assert len(gd) == 3 * 13
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
def test_mega_train_step_vs_reference_golden_fp32(case):
    """(a) 64 rays x 32 samples, (b) the same rays with 16 fine samples: rgb, depth, loss and every cell's gradient."""
    g = _load("mega_train")
    m = _mega(g, float(g["margin"]))
    S, F = int(g["S"]), int(g["F"]) if case == "b" else 0
    st = m.train_step(_dev(g["rgbs"]), _dev(g["rays"]), _dev(g["image_indices"]), S, perturb=0.0, optimizer_step=False, fine_samples=F)
    print(f"({case}) members per cell {st['ctx']['counts']}" + (f", fine {st['ctx_fine']['counts']}" if F else "") + f"; reference {g[case + '_members'].tolist()}")
    print(f"({case}) rgb err {np.abs(st['rgb'].cpu().numpy() - g[case + '_rgb']).max():.3e}, loss {st['loss'].item():.8f} / {float(g[case + '_loss']):.8f}")
    np.testing.assert_allclose(st["rgb"].cpu().numpy(), g[case + "_rgb"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(st["depth"].cpu().numpy(), g[case + "_depth"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(st["loss"].item(), float(g[case + "_loss"]), rtol=1e-5)
    assert float(st["gate_loss"].item()) == 0.0
    assert set(st) >= {"loss", "photo_loss", "psnr", "rgb", "depth", "depth_variance", "gate_loss"}
    _check_grads(m, lambda k: (g[f"{case}_gsum__{k}"], g[f"{case}_gslice__{k}"]), f"({case})")


@pytest.mark.parametrize("tag,margin", [("m100", 1.0), ("m115", 1.15)])
def test_mega_forward_backward_points_vs_reference_golden_fp32(tag, margin):
    """The module's own autograd: 2048 points with sigma noise, out.backward(d_out), hard and soft margin."""
    g, fg = _load("mega_train_module"), _load("mega_fg")
    assert not fg["excluded_" + tag].any()          # (gradients are compared only when no point lies on a decision)
    m = _mega(g, margin)
    for sub in m.sub_modules:
        sub.grad.zero_()
    ctx = m.forward_points(_dev(fg["x"]), _dev(fg["sigma_noise"]))
    out = ctx["out"].cpu().numpy()
    np.testing.assert_allclose(out[:, :3], g["out_" + tag][:, :3], rtol=0, atol=1e-4)
    np.testing.assert_allclose(out[:, 3], g["out_" + tag][:, 3], rtol=1e-4, atol=1e-4)
    m.backward_points(ctx, _dev(g["d_out"]))
    names, off = [str(n) for n in g["param_names"]], g["offsets"]
    idx = {n: i for i, n in enumerate(names)}
    _check_grads(m, lambda k: (g[tag + "_gsums"][idx[k]], g[tag + "_gslices"][off[idx[k]]:off[idx[k] + 1]]), tag)


def test_mega_adam_two_steps_and_empty_cells_vs_reference_golden():
    """(c) two Adam steps; the second on rays whose every sample lies in cell 0: cells 1 and 2 have a zero gradient, not a missing one,
    and still move (momentum), as under the reference's one torch.optim.Adam."""
    g = _load("mega_train")
    m = _mega(g, float(g["margin"]))
    m.lr = m.base_lr = float(g["lr"])
    names, off = [str(n) for n in g["param_names"]], g["c_offsets"]
    rgbs, img = _dev(g["rgbs"]), _dev(g["image_indices"])
    after = {}
    for step, rays in ((1, g["rays"]), (2, g["rays_cell0"])):
        st = m.train_step(rgbs, _dev(rays), img, int(g["S"]), perturb=0.0, optimizer_step=True)
        if step == 2:
            assert st["ctx"]["counts"] == [int(g["N"]) * int(g["S"]), 0, 0]
            for k, t in m.grad_dict().items():
                if not k.startswith("sub_modules.0."):
                    assert not t.any(), k
        after[step] = {k: v.cpu().numpy() for k, v in m.named_parameters()}
        worst = 0.0
        for i, k in enumerate(names):
            ref = g[f"c_p{step}_slices"][off[i]:off[i + 1]]
            got = _sl(after[step][k])[::2]
            g1 = g["a_gslice__" + k][::2]                      # the step-1 gradient at the same positions
            small = np.abs(g1) < 1e-7 * max(1e-12, np.abs(g["a_gslice__" + k]).max())      # update direction ill-defined there
            worst = max(worst, float(np.abs(np.where(small, ref, got) - ref).max()))
            np.testing.assert_allclose(np.where(small, ref, got), ref, rtol=0, atol=2e-5, err_msg=f"step {step} {k}")
        print(f"step {step}: worst parameter error {worst:.2e}")
    assert m.step_count == 2 and all(s.step_count == 2 for s in m.sub_modules)
    for k in names:
        if not k.startswith("sub_modules.0.") and np.abs(g["a_gslice__" + k]).max() > 0:
            assert not np.array_equal(after[1][k], after[2][k]), k      # moved without a point


def test_mega_grad_step_is_deterministic_and_optimizer_step_false_changes_nothing():
    g = _load("mega_train")
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


def test_mega_train_bf16_close_to_fp32():
    g = _load("mega_train")
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


def test_mega_eval_after_training_equals_the_inference_model():
    """One optimizer step, then eval(): the trained model renders bit-equal to a joint_training = False model holding the same weights
    (and rendering.render_rays refuses it while it is in training mode)."""
    from argparse import Namespace
    from switch_nerf_amd.mega import MegaNeRF
    from switch_nerf_amd.rendering import render_rays
    g = _load("mega_train")
    m = _mega(g, 1.15)
    rays, img = _dev(g["rays"]), _dev(g["image_indices"])
    m.train_step(_dev(g["rgbs"]), rays, img, int(g["S"]), perturb=0.0)
    h = Namespace(coarse_samples=int(g["S"]), fine_samples=int(g["F"]), model_chunk_size=1000, perturb=1.0, use_sigma_noise=True, sigma_noise_std=1.0)
    with pytest.raises(NotImplementedError, match="evaluation mode"):
        render_rays(m, None, rays, img, h, None, None, True, True, False)
    m.eval()
    assert not m.training and not any(s.training for s in m.sub_modules)
    cfg = m.sub_modules[0].cfg
    twin = MegaNeRF.from_state_dicts([{k: v.cpu() for k, v in sd.items()} for sd in m.state_dicts()], g["centroids"], cfg, boundary_margin=1.15)
    assert not twin.joint_training
    a, _ = render_rays(m, None, rays, img, h, None, None, True, True, False)
    b, _ = render_rays(twin, None, rays, img, h, None, None, True, True, False)
    assert set(a) == set(b) == {"rgb_fine", "depth_fine", "depth_variance_fine"}
    for k in a:
        assert torch.equal(a[k], b[k]), k
