"""The padded form of Mega-NeRF joint training (switch_nerf_amd/mega.py: cell_capacity) and its captured step (graph.GraphedMegaStep) on
the reference's own run (tests/golden/mega_train.npz, mega_train_module.npz): 64 rays x 32 samples (+ 16 fine), three cells with
756 / 764 / 528 coarse and 378 / 380 / 266 fine members; rays_cell0 puts all 2048 points into cell 0.  Helpers, comparisons and bounds
are those of tests/test_mega_train_gpu.py (rgb 1e-4, depth 1e-4 relative + 1e-5, loss 1e-5 relative, gradient checksums and slices, the
2e-5 Adam rule)."""
import numpy as np
import pytest
import torch

from test_mega_train_gpu import _check_grads, _dev, _load, _mega, _sl

pytestmark = pytest.mark.gpu


def _batch(g, rays="rays"):
    return _dev(g["rgbs"]), _dev(g[rays]), _dev(g["image_indices"])


def _state(m):
    """Every parameter, moment and step count of the model, cloned."""
    return ([(s.flat.clone(), s.m.clone(), s.v.clone(), s.step_count) for s in m.sub_modules], m.step_count)


def _same_state(a, b):
    return a[1] == b[1] and all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and torch.equal(x[2], y[2]) and x[3] == y[3]
                                for x, y in zip(a[0], b[0]))


def _check_adam(m, g, step, after):
    """tests/test_mega_train_gpu.py's Adam rule against golden (c): 2e-5 wherever the step-1 gradient is not below 1e-7 of its maximum."""
    names, off = [str(n) for n in g["param_names"]], g["c_offsets"]
    worst = 0.0
    for i, k in enumerate(names):
        ref = g[f"c_p{step}_slices"][off[i]:off[i + 1]]
        got = _sl(after[k])[::2]
        g1 = g["a_gslice__" + k][::2]
        small = np.abs(g1) < 1e-7 * max(1e-12, np.abs(g["a_gslice__" + k]).max())
        worst = max(worst, float(np.abs(np.where(small, ref, got) - ref).max()))
        np.testing.assert_allclose(np.where(small, ref, got), ref, rtol=0, atol=2e-5, err_msg=f"step {step} {k}")
    print(f"step {step}: worst parameter error {worst:.2e}")


@pytest.mark.parametrize("cap", [(768, 384), (2048, 1024)])
@pytest.mark.parametrize("case", ["a", "b"])
def test_padded_step_vs_reference_golden_fp32(case, cap):
    g = _load("mega_train")
    m = _mega(g, float(g["margin"]))
    S, F = int(g["S"]), int(g["F"]) if case == "b" else 0
    st = m.train_step(*_batch(g), S, perturb=0.0, optimizer_step=False, fine_samples=F, cell_capacity=cap)
    print(f"({case}, C {cap}) rgb err {np.abs(st['rgb'].cpu().numpy() - g[case + '_rgb']).max():.3e}, loss {st['loss'].item():.8f} / "
          f"{float(g[case + '_loss']):.8f}")
    np.testing.assert_allclose(st["rgb"].cpu().numpy(), g[case + "_rgb"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(st["depth"].cpu().numpy(), g[case + "_depth"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(st["loss"].item(), float(g[case + "_loss"]), rtol=1e-5)
    _check_grads(m, lambda k: (g[f"{case}_gsum__{k}"], g[f"{case}_gslice__{k}"]), f"({case}, C {cap})")
    assert st["cell_overflow"].dtype == torch.int32 and st["cell_overflow"].tolist() == [0, 0]
    members = g[case + "_members"]
    assert torch.is_tensor(st["ctx"]["counts"]) and st["ctx"]["counts"].dtype == torch.int32 and st["ctx"]["counts"].is_cuda
    assert st["ctx"]["counts"].tolist() == members[0].tolist() and st["ctx"]["C"] == cap[0]
    assert st["ctx"]["overflow"].is_cuda and int(st["ctx"]["overflow"].item()) == 0
    if F:
        assert st["ctx_fine"]["counts"].tolist() == members[1].tolist() and st["ctx_fine"]["C"] == cap[1]


@pytest.mark.parametrize("F", [0, 16])
def test_padded_step_vs_compact_step_same_noise(F):
    """Same model, batch and supplied sigma noise: outputs and gradients within the fixture bounds of each other.  Bit equality is
    printed, not asserted: a cell's reduction geometry may depend on its row count."""
    g = _load("mega_train")
    m = _mega(g, float(g["margin"]))
    N, S = int(g["N"]), int(g["S"])
    gen = torch.Generator(device="cuda").manual_seed(11)
    noise, noise_f = torch.randn(N * S, device="cuda", generator=gen), torch.randn(N * 16, device="cuda", generator=gen)
    kw = dict(perturb=0.0, optimizer_step=False, sigma_noise=noise, fine_samples=F, sigma_noise_fine=noise_f if F else None)
    outs = []
    for cap in (None, (768, 384)):
        st = m.train_step(*_batch(g), S, cell_capacity=cap, **kw)
        outs.append(({k: st[k].clone() for k in ("rgb", "depth", "loss")}, {k: v.clone() for k, v in m.grad_dict().items()}))
    (a, ga), (b, gb) = outs
    equal = all(torch.equal(a[k], b[k]) for k in a) and all(torch.equal(ga[k], gb[k]) for k in ga)
    print(f"F {F}: padded step bit-equal to the compact step: {equal}")
    np.testing.assert_allclose(b["rgb"].cpu().numpy(), a["rgb"].cpu().numpy(), rtol=0, atol=1e-4)
    np.testing.assert_allclose(b["depth"].cpu().numpy(), a["depth"].cpu().numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(b["loss"].item(), a["loss"].item(), rtol=1e-5)
    for k in ga:
        ref = ga[k].cpu().numpy()
        np.testing.assert_allclose(gb[k].cpu().numpy(), ref, rtol=2e-3, atol=1e-7 + 2e-4 * np.abs(ref).max(), err_msg=k)


def test_padded_forward_backward_points_soft_margin_vs_reference_golden():
    """The margin-1.15 module case through forward_points / backward_points with a capacity that fits (every point may sit in every cell)."""
    g, fg = _load("mega_train_module"), _load("mega_fg")
    m = _mega(g, 1.15)
    for sub in m.sub_modules:
        sub.grad.zero_()
    P = fg["x"].shape[0]
    ctx = m.forward_points(_dev(fg["x"]), _dev(fg["sigma_noise"]), cell_capacity=P)
    assert int(ctx["overflow"].item()) == 0 and ctx["counts"].tolist() == (fg["weights_m115"] > 0).sum(0).tolist() and ctx["total"] == 3 * P
    out = ctx["out"].cpu().numpy()
    np.testing.assert_allclose(out[:, :3], g["out_m115"][:, :3], rtol=0, atol=1e-4)
    np.testing.assert_allclose(out[:, 3], g["out_m115"][:, 3], rtol=1e-4, atol=1e-4)
    m.backward_points(ctx, _dev(g["d_out"]))
    names, off = [str(n) for n in g["param_names"]], g["offsets"]
    idx = {n: i for i, n in enumerate(names)}
    _check_grads(m, lambda k: (g["m115_gsums"][idx[k]], g["m115_gslices"][off[idx[k]]:off[idx[k] + 1]]), "m115 padded")


def test_padded_adam_two_steps_and_empty_cells_vs_reference_golden():
    """Golden (c) with C = 2048: the second step has every point in cell 0; cells 1 and 2 run on padding rows only, have an all-zero
    gradient (not a missing one) and still move."""
    g = _load("mega_train")
    m = _mega(g, float(g["margin"]))
    m.lr = m.base_lr = float(g["lr"])
    rgbs, _, img = _batch(g)
    after = {}
    for step, rays in ((1, "rays"), (2, "rays_cell0")):
        st = m.train_step(rgbs, _dev(g[rays]), img, int(g["S"]), perturb=0.0, optimizer_step=True, cell_capacity=2048)
        if step == 2:
            assert st["ctx"]["counts"].tolist() == [2048, 0, 0]
            for k, t in m.grad_dict().items():
                if not k.startswith("sub_modules.0."):
                    assert not t.any(), k
        after[step] = {k: v.cpu().numpy() for k, v in m.named_parameters()}
        _check_adam(m, g, step, after[step])
    assert m.step_count == 2 and all(s.step_count == 2 for s in m.sub_modules)
    for k in after[1]:
        if not k.startswith("sub_modules.0.") and np.abs(g["a_gslice__" + k]).max() > 0:
            assert not np.array_equal(after[1][k], after[2][k]), k


def test_padded_overflow_raises_and_touches_nothing():
    g = _load("mega_train")
    m = _mega(g, float(g["margin"]))
    m.lr = m.base_lr = float(g["lr"])
    S = int(g["S"])
    m.train_step(*_batch(g), S, perturb=0.0, cell_capacity=768)                  # (moments and step count are no longer zero)
    before = _state(m)
    with pytest.raises(RuntimeError, match=r"cell capacity 768.*\[2048, 0, 0\]"):
        m.train_step(*_batch(g, "rays_cell0"), S, perturb=0.0, cell_capacity=768)
    assert _same_state(before, _state(m)) and m.step_count == 1
    st = m.train_step(*_batch(g), S, perturb=0.0, cell_capacity=768)
    assert st["cell_overflow"].tolist() == [0, 0] and m.step_count == 2 and not _same_state(before, _state(m))


@pytest.mark.parametrize("F", [0, 16])
def test_graphed_step_replays_equal_the_eager_padded_step(F):
    """One capture at C = (2048, 1024), replayed on rays, rays_cell0 and rays again: loss, rgb and every gradient bit for bit the eager
    padded step's on that batch."""
    from switch_nerf_amd.graph import GraphedMegaStep
    g = _load("mega_train")
    m, twin = _mega(g, float(g["margin"])), _mega(g, float(g["margin"]))
    S, cap = int(g["S"]), (2048, 1024)
    step = GraphedMegaStep(m, *_batch(g), S, cap, perturb=0.0, noise_std=0.0, fine_samples=F)
    for rays in ("rays", "rays_cell0", "rays"):
        res = step(*_batch(g, rays), optimizer_step=False)
        ref = twin.train_step(*_batch(g, rays), S, perturb=0.0, optimizer_step=False, fine_samples=F, cell_capacity=cap)
        assert torch.equal(res["loss"], ref["loss"]) and torch.equal(res["rgb"], ref["rgb"]) and torch.equal(res["depth"], ref["depth"]), rays
        assert res["ctx"]["counts"].tolist() == ref["ctx"]["counts"].tolist() and res["cell_overflow"].tolist() == [0, 0]
        gm, gt = m.grad_dict(), twin.grad_dict()
        for k in gm:
            assert torch.equal(gm[k], gt[k]), (rays, k)
    assert step.captures == 1 and m.step_count == 0


def test_graphed_step_adam_vs_reference_golden():
    from switch_nerf_amd.graph import GraphedMegaStep
    g = _load("mega_train")
    m = _mega(g, float(g["margin"]))
    m.lr = m.base_lr = float(g["lr"])
    step = GraphedMegaStep(m, *_batch(g), int(g["S"]), 2048, perturb=0.0, noise_std=0.0)
    for n, rays in ((1, "rays"), (2, "rays_cell0")):
        step(*_batch(g, rays))
        _check_adam(m, g, n, {k: v.cpu().numpy() for k, v in m.named_parameters()})
    assert m.step_count == 2 and all(s.step_count == 2 for s in m.sub_modules) and step.captures == 1


def test_graphed_step_overflow_raises_from_the_tail():
    from switch_nerf_amd.graph import GraphedMegaStep
    g = _load("mega_train")
    m, twin = _mega(g, float(g["margin"])), _mega(g, float(g["margin"]))
    S = int(g["S"])
    step = GraphedMegaStep(m, *_batch(g), S, 768, perturb=0.0, noise_std=0.0)
    before = _state(m)
    with pytest.raises(RuntimeError, match=r"cell capacity 768.*\[2048, 0, 0\]"):
        step(*_batch(g, "rays_cell0"))
    assert _same_state(before, _state(m))
    res = step(*_batch(g), optimizer_step=False)
    ref = twin.train_step(*_batch(g), S, perturb=0.0, optimizer_step=False, cell_capacity=768)
    assert torch.equal(res["loss"], ref["loss"]) and torch.equal(res["rgb"], ref["rgb"])
    gm, gt = m.grad_dict(), twin.grad_dict()
    for k in gm:
        assert torch.equal(gm[k], gt[k]), k
    assert step.captures == 1
