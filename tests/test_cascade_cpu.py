"""CPU-only: the internal consistency of tests/golden/cascade_dense.npz (scripts/gen_golden_cascade.py) and the argument checks of
cascade.Cascade that need no device."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import synth

G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(G, "cascade_dense.npz"))


@pytest.mark.parametrize("case", ["p0", "p1"])
def test_fixture_loss_and_union_are_consistent(g, case):
    N, S, F = int(g["N"]), int(g["S"]), int(g["F"])
    rays, img, rgbs = synth.make_rays(int(g["ray_seed"]), N, synth.DENSE["appearance_count"])
    assert np.array_equal(rays, g["rays"]) and np.array_equal(img, g["image_indices"]) and np.array_equal(rgbs, g["rgbs"])
    mse = lambda a: np.mean((a.astype(np.float64) - rgbs) ** 2)
    loss = (mse(g[case + "_rgb_fine"]) + mse(g[case + "_rgb_coarse"])) / 2          # runner.py:1195-1204
    np.testing.assert_allclose(loss, float(g[case + "_loss"]), rtol=1e-6)
    zu = g[case + "_z_union"]
    assert zu.shape == (N, S + F) and (np.diff(zu, axis=1) >= -1e-6).all()
    # the coarse depths (rendering.py:86, :573-584)
    tt = np.linspace(0, 1, S, dtype=np.float32)
    z = rays[:, 6:7] * (1 - tt) + rays[:, 7:8] * tt
    if case == "p1":
        mid = 0.5 * (z[:, :-1] + z[:, 1:])
        lo, hi = np.concatenate([z[:, :1], mid], 1), np.concatenate([mid, z[:, -1:]], 1)
        z = lo + (hi - lo) * g["p1_perturb_rand"]
    # the fine draws: _sample_pdf (rendering.py:587-637) restated in float64 on the stored coarse weights; the union is the sort of both
    z64, w = z.astype(np.float64), g[case + "_w_inner"].astype(np.float64) + 1e-8
    assert w.shape == (N, S - 2)
    bins = 0.5 * (z64[:, :-1] + z64[:, 1:])
    cdf = np.concatenate([np.zeros((N, 1)), np.cumsum(w / w.sum(1, keepdims=True), 1)], 1)
    u = g["p1_fine_u"].astype(np.float64) if case == "p1" else np.broadcast_to(np.linspace(0, 1, F), (N, F))
    union = np.empty((N, S + F))
    for i in range(N):
        inds = np.searchsorted(cdf[i], u[i], side="right")
        below, above = np.maximum(inds - 1, 0), np.minimum(inds, S - 2)
        denom = cdf[i][above] - cdf[i][below]
        denom = np.where(denom < 1e-8, 1.0, denom)
        fine = bins[i][below] + (u[i] - cdf[i][below]) / denom * (bins[i][above] - bins[i][below])
        union[i] = np.sort(np.concatenate([z64[i], fine]))
    np.testing.assert_allclose(zu, union, rtol=0, atol=1e-5)
    names = [str(k) for k in g["param_names"]]
    assert len(names) == 50 and all(n.startswith(("coarse.", "fine.")) for n in names)
    sums = np.stack([synth.checksum(v) for i in range(2) for v in synth.make_dense_weights(int(g["seed"]) + i, synth.DENSE).values()])
    assert np.array_equal(sums, g["sd_checksums"])


def test_cascade_argument_checks_without_a_device():
    from switch_nerf_amd.cascade import Cascade
    from switch_nerf_amd.dense import DenseNeRF
    from switch_nerf_amd.model import SwitchNeRF

    def fake(cls, **kw):
        m = cls.__new__(cls)
        m.__dict__.update(dict(cfg=dict(synth.DENSE), dtype="bf16", sh_deg=None, affine=False, loss_scaler=None), **kw)
        return m
    with pytest.raises(TypeError, match="must be a DenseNeRF"):
        Cascade(SimpleNamespace(), None)
    with pytest.raises(NotImplementedError, match="Mega-NeRF"):
        Cascade(SimpleNamespace(is_mega_nerf=True), None)
    with pytest.raises(NotImplementedError, match="sh_deg"):
        Cascade(fake(DenseNeRF, sh_deg=2), None)
    with pytest.raises(NotImplementedError, match="affine"):
        Cascade(fake(DenseNeRF), fake(DenseNeRF, affine=True))
    with pytest.raises(NotImplementedError, match="MoE halves"):
        Cascade(fake(SwitchNeRF), None)
    with pytest.raises(NotImplementedError, match="MoE halves"):
        Cascade(fake(DenseNeRF), fake(SwitchNeRF))
    with pytest.raises(ValueError, match="same cfg"):
        Cascade(fake(DenseNeRF), fake(DenseNeRF, cfg=dict(synth.DENSE, layers=6)))
    with pytest.raises(ValueError, match="compute dtype"):
        Cascade(fake(DenseNeRF), fake(DenseNeRF, dtype="f32"))
    a = fake(DenseNeRF)
    with pytest.raises(ValueError, match="two models"):
        Cascade(a, a)
    c = Cascade(fake(DenseNeRF), fake(DenseNeRF))
    assert c.is_cascade and len(c.halves()) == 2 and len(Cascade(a, None).halves()) == 1
    with pytest.raises(ValueError, match="no fine half"):
        Cascade(a, None)(False, None)
    for refused in (c.set_device_noise, c.set_expert_parallel, c.forward_mip, c.train_step_mip):
        with pytest.raises(NotImplementedError, match="Cascade"):
            refused()
    with pytest.raises(NotImplementedError, match="split=True"):
        c.grad_step(None, None, None, 32, 1024, fine_samples=16, split=True)


def test_render_rays_names_cascade_for_other_models():
    from switch_nerf_amd import rendering
    h = SimpleNamespace(use_cascade=True)
    with pytest.raises(NotImplementedError, match="Cascade"):
        rendering.render_rays(SimpleNamespace(), None, None, None, h)
    with pytest.raises(NotImplementedError, match="use_cascade is off"):
        rendering.render_rays(SimpleNamespace(is_cascade=True), None, None, None, SimpleNamespace(use_cascade=False))
