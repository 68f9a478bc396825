"""Gradient accumulation (SwitchNeRF.set_accumulation; the reference's --accumulation_steps, runner.py:589, 657, 677-690) on the native
step: the window rule, the fused and unfused last micro-step, one all-reduce per window on the buffer, the graph replay, the fp16 skipped
window, the background rule, the refusals, and parity with tests/golden/accum_train.npz (scripts/gen_golden_accum.py: the reference's
own loop on the CPU)."""
import os

import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
N, S, CHUNK = 64, 16, 1024


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _moe(dtype, seed=41, cfg=synth.BUILDING, **kw):
    from switch_nerf_amd.model import SwitchNeRF
    m = SwitchNeRF(cfg, dtype=dtype, **kw)
    m.load_state_dict(synth.make_weights(seed, cfg))
    return m


def _dense(dtype, seed=161, cfg=synth.DENSE):
    from switch_nerf_amd.dense import DenseNeRF
    m = DenseNeRF(cfg, dtype=dtype)
    m.load_state_dict(synth.make_dense_weights(seed, cfg))
    return m


def _batches(n, seed=900, rays=N):
    return [tuple(_dev(a) for a in synth.make_rays(seed + i, rays)) for i in range(n)]


def _step(m, batch, **kw):
    rays, img, rgbs = batch
    return m.train_step(rgbs, rays, img, S, CHUNK, perturb=0.0, **kw)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_one_accumulation_step_is_the_plain_step(dtype):
    a, b = _moe(dtype), _moe(dtype)
    a.set_accumulation(1)
    assert a.accum is None and a.accum_steps == 1
    for batch in _batches(2):
        ra, rb = _step(a, batch), _step(b, batch)
        assert "optimizer_stepped" not in ra and ra["loss"].item() == rb["loss"].item()
        assert torch.equal(a.flat, b.flat) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
    assert a.step_count == b.step_count == 2


class _CountingAllReduce:
    """A gradient all-reduce of one rank: counts its calls, records what it was given, returns the 1 / world factor 1.0."""

    def __init__(self):
        self.calls = []

    def __call__(self, view):
        self.calls.append((view.data_ptr(), view.numel()))
        return 1.0


@pytest.mark.parametrize("A", [2, 3])
def test_fused_and_unfused_last_steps_agree_and_window_bookkeeping(A):
    fused, unfused = _moe(torch.bfloat16), _moe(torch.bfloat16)
    for m in (fused, unfused):
        m.set_accumulation(A)
        assert m.accum.shape == m.grad.shape and m.accum.dtype == torch.float32 and not bool(m.accum.any())
    ar = _CountingAllReduce()
    batches = _batches(2 * A)
    before = fused.flat.clone()
    for it, batch in enumerate(batches):
        rf, ru = _step(fused, batch), _step(unfused, batch, grad_allreduce=ar)
        last = (it + 1) % A == 0
        assert rf["optimizer_stepped"] is last and ru["optimizer_stepped"] is last
        assert rf["loss"].item() == ru["loss"].item()                        # the micro-batch's own loss, undivided
        assert fused.step_count == unfused.step_count == (it + 1) // A       # one optimizer step per window
        assert len(ar.calls) == (it + 1) // A                                # one all-reduce per window (no_sync in between) ...
        assert torch.equal(fused.flat, unfused.flat) and torch.equal(fused.m, unfused.m) and torch.equal(fused.v, unfused.v), it
        if last:
            assert not bool(fused.accum.any()) and not bool(unfused.accum.any())         # cleared for the next window
        elif it < A:
            assert torch.equal(fused.flat, before)                           # no parameter moves inside the window
    assert all(c == (unfused.accum.data_ptr(), unfused.accum.numel()) for c in ar.calls)  # ... on the accumulation buffer
    assert not torch.equal(fused.flat, before)


def test_accumulated_step_equals_the_mean_gradient_step():
    """A = 2 on two micro-batches = Adam on (g0 + g1) / 2 (exact in fp32: halving is exact), against the kernels run by hand."""
    from switch_nerf_amd import ops
    m, ref = _moe(torch.float32), _moe(torch.float32)
    m.set_accumulation(2)
    b = _batches(2)
    grads = []
    for batch in b:
        _step(m, batch)
        _step(ref, batch, optimizer_step=False)
        grads.append(ref.grad.clone())
    assert torch.equal(m.grad, grads[1])
    mean = grads[0] * 0.5 + grads[1] * 0.5
    ref.step_count += 1
    ops.adam_step(ref.flat, mean, ref.m, ref.v, None, ref.step_count, ref.lr)
    assert torch.equal(m.flat, ref.flat) and torch.equal(m.m, ref.m) and torch.equal(m.v, ref.v) and m.step_count == 1


def test_explicit_should_accumulate_overrides_the_rule_and_restart():
    m = _moe(torch.bfloat16)
    m.set_accumulation(4)
    b = _batches(3)
    assert _step(m, b[0], should_accumulate=True)["optimizer_stepped"] is False
    assert _step(m, b[1], should_accumulate=False)["optimizer_stepped"] is True and m.step_count == 1      # a resumed run's own rule
    assert _step(m, b[2])["optimizer_stepped"] is False and bool(m.accum.any())     # the model's rule: micro-step index 2 of 4
    m.set_accumulation(4)                                                            # restarts the window
    assert m._micro == 0 and not bool(m.accum.any())
    with pytest.raises(ValueError):
        m.set_accumulation(0)
    m.set_accumulation(1)
    with pytest.raises(ValueError, match="should_accumulate"):
        _step(m, b[0], should_accumulate=True)


def test_graph_replay_with_device_noise_equals_eager_accumulated_steps():
    from switch_nerf_amd.graph import GraphedTrainStep
    A = 2
    b = _batches(4)
    ma, mb = _moe(torch.bfloat16), _moe(torch.bfloat16)
    for m in (ma, mb):
        m.set_device_noise(4321)
    rays0, img0, rgbs0 = b[0]
    step = GraphedTrainStep(ma, rgbs0, rays0, img0, S, CHUNK, perturb=1.0, noise_std=1.0)
    ma.load_state_dict(synth.make_weights(41, synth.BUILDING))
    ma.m.zero_(); ma.v.zero_(); ma.step_count = 0
    ma.refresh_compute_copies()
    for m in (ma, mb):
        m.set_accumulation(A)
    for it, (rays, img, rgbs) in enumerate(b):
        ra = step(rgbs, rays, img)
        la, sa = ra["loss"].item(), ra["optimizer_stepped"]
        rb = mb.train_step(rgbs, rays, img, S, CHUNK, perturb=1.0, sigma_noise_std=1.0)
        assert la == rb["loss"].item() and sa is rb["optimizer_stepped"] is ((it + 1) % A == 0)
        assert torch.equal(ra["ctx"]["z"], rb["ctx"]["z"])
        assert torch.equal(ma.flat, mb.flat) and torch.equal(ma.accum, mb.accum), it
    assert ma.step_count == mb.step_count == 2
    assert ma.noise_state_dict()["step"] == mb.noise_state_dict()["step"] == 4       # the noise advances once per micro-step


def test_fp16_inf_in_one_micro_gradient_skips_the_window():
    from switch_nerf_amd import _lib
    try:
        m = _moe(torch.float16)
        m.set_accumulation(2)
        b = _batches(4)
        scale0 = m.loss_scaler.scale
        rays, img, rgbs = b[0]
        m.grad_step(rgbs, rays, img, S, CHUNK, perturb=0.0)
        m.grad[12345] = float("inf")                                  # planted in the first micro-gradient of the window
        assert m.apply_step() is False
        assert m.loss_scaler.scale == scale0                          # the scale changes at the window's end only
        before = m.flat.clone()
        assert _step(m, b[1])["optimizer_stepped"] is False           # last micro-step: inf found in the buffer, window skipped
        assert m.loss_scaler.scale == scale0 * 0.5 and m.loss_scaler.skipped == 1 and m.step_count == 0
        assert torch.equal(m.flat, before) and not bool(m.accum.any()) and bool(torch.isfinite(m.accum).all())
        assert _step(m, b[2])["optimizer_stepped"] is False
        assert _step(m, b[3])["optimizer_stepped"] is True and m.step_count == 1 and not torch.equal(m.flat, before)
        assert bool(torch.isfinite(m.flat).all())
    finally:
        _lib.use_half("bf16")


def _scene(dtype=torch.float32):
    from switch_nerf_amd.background import BackgroundScene
    from switch_nerf_amd.dense import DenseNeRF
    from switch_nerf_amd.model import SwitchNeRF
    return BackgroundScene(SwitchNeRF(synth.BUILDING, dtype=dtype, seed=5), DenseNeRF(synth.DENSE_BG, dtype=dtype, seed=6),
                           synth.SPHERE_CENTER, synth.SPHERE_RADIUS)


def _bg_batch(seed, with_background):
    rays, img, rgbs = synth.make_bg_rays(seed, N)
    if not with_background:
        rays[:, 7] = 0.25                     # every ray stops inside the foreground bound
    return _dev(rays), _dev(img), _dev(rgbs)


@pytest.mark.parametrize("last_has_background", [False, True])
def test_background_scene_follows_the_last_micro_batch(last_has_background):
    scene = _scene()
    scene.set_accumulation(2)
    nerf, bg = scene.nerf, scene.bg
    assert nerf.accum_steps == bg.accum_steps == scene.accum_steps == 2
    state = [t.clone() for t in (bg.flat, bg.m, bg.v)]
    fg_before = nerf.flat.clone()
    rays, img, rgbs = _bg_batch(181, True)
    r0 = scene.train_step(rgbs, rays, img, S, CHUNK, perturb=0.0)
    assert r0["optimizer_stepped"] is False and r0["bg_nerf_rays_present"] is True
    assert bool(bg.accum.any()) and bool(nerf.accum.any()) and torch.equal(nerf.flat, fg_before)
    rays, img, rgbs = _bg_batch(182, last_has_background)
    r1 = scene.train_step(rgbs, rays, img, S, CHUNK, perturb=0.0)
    assert r1["optimizer_stepped"] is True and r1["bg_nerf_rays_present"] is last_has_background
    assert nerf.step_count == 1 and not torch.equal(nerf.flat, fg_before) and not bool(nerf.accum.any())
    assert not bool(bg.accum.any())                                   # stepped on, or discarded with the window (zero_grad)
    unchanged = all(torch.equal(a, b) for a, b in zip(state, (bg.flat, bg.m, bg.v)))
    if last_has_background:
        assert bg.step_count == 1 and not unchanged
    else:
        assert bg.step_count == 0 and unchanged


def test_refusals():
    from switch_nerf_amd.graph import GraphedBackgroundStep
    from switch_nerf_amd.mega import MegaNeRF
    from switch_nerf_amd.parallel import ExpertParallel
    # the padded background form and its graph
    scene = _scene()
    scene.set_accumulation(2)
    rays, img, rgbs = _bg_batch(181, True)
    with pytest.raises(NotImplementedError, match="accumulation"):
        scene.train_step(rgbs, rays, img, S, CHUNK, perturb=0.0, bg_capacity=N)
    with pytest.raises(NotImplementedError, match="accumulation"):
        GraphedBackgroundStep(scene, rgbs, rays, img, S, CHUNK, perturb=0.0, noise_std=0.0)
    # the mip step
    m = _moe(torch.float32)
    m.set_accumulation(2)
    rays, img, rgbs = _batches(1)[0]
    with pytest.raises(NotImplementedError, match="accumulation"):
        m.train_step_mip(rgbs, rays, torch.full((N, 1), 1e-3, device="cuda"), img, S, 8, CHUNK, perturb=0.0)
    # expert parallelism with the tail on the experts' ranks, in either order
    with pytest.raises(NotImplementedError, match="owner_tail"):
        m.set_expert_parallel(ExpertParallel(0, 1, m.E, owner_tail=True))
    m2 = _moe(torch.float32)
    m2.set_expert_parallel(ExpertParallel(0, 1, m2.E, owner_tail=True))
    with pytest.raises(NotImplementedError, match="owner_tail"):
        m2.set_accumulation(2)
    m2.set_accumulation(1)
    # Mega-NeRF joint training
    cells = [_dense(torch.float32, 161 + i) for i in range(2)]
    cen = np.array([[-0.05, 0.0, 0.0], [0.05, 0.0, 0.0]], np.float32)
    mega = MegaNeRF(cells, cen, 1.0, False, False, joint_training=True)
    with pytest.raises(NotImplementedError, match="accumulation"):
        mega.set_accumulation(2)
    mega.set_accumulation(1)
    with pytest.raises(ValueError):
        mega.set_accumulation(0)


def test_cascade_one_window_over_both_halves():
    from switch_nerf_amd.cascade import Cascade
    a = Cascade(_dense(torch.float32, 171), _dense(torch.float32, 172))
    b = Cascade(_dense(torch.float32, 171), _dense(torch.float32, 172))
    a.set_accumulation(2)
    batches = _batches(2)
    fu = torch.rand(N, 8, generator=torch.Generator().manual_seed(3)).cuda()
    kw = dict(perturb=0.0, fine_samples=8, fine_u=fu)
    for it, (rays, img, rgbs) in enumerate(batches):
        r = a.train_step(rgbs, rays, img, S, N * S, **kw)
        assert r["optimizer_stepped"] is (it == 1)
    for ha, hb in zip(a.halves(), b.halves()):
        assert ha.step_count == 1 and not bool(ha.accum.any()) and not torch.equal(ha.flat, hb.flat)
    # the same window by hand on the twin: the two micro-gradients of each half, halved and summed, then Adam
    from switch_nerf_amd import ops
    grads = []
    for rays, img, rgbs in batches:
        b.train_step(rgbs, rays, img, S, N * S, optimizer_step=False, **kw)
        grads.append([h.grad.clone() for h in b.halves()])
    for i, h in enumerate(b.halves()):
        h.step_count += 1
        ops.adam_step(h.flat, grads[0][i] * 0.5 + grads[1][i] * 0.5, h.m, h.v, None, h.step_count, h.lr)
    for ha, hb in zip(a.halves(), b.halves()):
        assert torch.equal(ha.flat, hb.flat) and torch.equal(ha.m, hb.m) and torch.equal(ha.v, hb.v)


# ------------------------------------------------------------------------------------------------------------ the reference's loop
def _unpack(g, key, offsets, names):
    packed = g[key]
    return {n: packed[offsets[i]: offsets[i + 1]] for i, n in enumerate(names)}


def _slice(t, every):
    a = t.detach().cpu().numpy().reshape(-1)
    return a[:: max(1, a.size // 499)][:499][::every]


@pytest.mark.parametrize("kind,A", [("moe", 2), ("moe", 3), ("dense", 2), ("dense", 3)])
def test_accumulated_training_vs_reference_golden_fp32(kind, A):
    """The runner.py:646-690 loop of the reference (fixture) against set_accumulation(A): per optimizer step the accumulated gradient
    with the tolerances tests/test_model_gpu.py / tests/test_dense_gpu.py apply to the one-step gradient of the same cfg (checksums
    1e-3 of the abs-sum; slices rtol 2e-3, atol 1e-7 + 2e-4 max|ref|), the parameters after Adam with test_dense_gpu.py's Adam bound
    (atol 2e-5 where the gradient is not negligible: |g| >= 1e-7 max|g|).
    Measured maxima (profiles/r20_accum.md): see there."""
    g = np.load(os.path.join(G, "accum_train.npz"))
    n_micro = {int(a): int(n) for a, n in g["cases"]}[A]
    tag, every, chunk, Sg = f"{kind}_a{A}_", int(g["every"]), int(g["chunk"]), int(g["S"])
    names = [str(n) for n in g[kind + "_param_names"]]
    offs = g[kind + "_offsets"]
    if kind == "moe":
        m = _moe(torch.float32, int(g["seed_moe"]))
    else:
        m = _dense(torch.float32, int(g["seed_dense"]))
        chunk = int(g["N"]) * Sg
    m.lr = m.base_lr = float(g["lr"])
    m.set_accumulation(A)
    inv = 1.0 / A
    step, worst_g, worst_p, worst_sum = 0, (0.0, ""), (0.0, ""), (0.0, "")
    for it in range(n_micro):
        rays, img, rgbs = (_dev(g[f"{kind}_mb{it}_{k}"]) for k in ("rays", "image_indices", "rgbs"))
        res = m.grad_step(rgbs, rays, img, Sg, chunk, perturb=0.0)
        np.testing.assert_allclose(res["loss"].item(), float(g[tag + f"m{it}_loss"]), rtol=1e-5)
        if kind == "moe":
            mis = int((res["ctx"]["idx"].cpu().numpy().reshape(-1) != g[tag + f"m{it}_moe_gates"].reshape(-1)).sum())
            print(f"{tag} micro {it}: routing mismatches vs reference {mis}")
        last = (it + 1) % A == 0
        total = m._to_ref_layout(m._views(m.accum + m.grad * inv)) if last else None     # what the fused step is about to consume
        assert m.apply_step() is last
        if not last:
            continue
        ref_sums = g[tag + f"s{step}_gsum__"]
        ref_g = _unpack(g, tag + f"s{step}_gslice__", offs, names)
        ref_p = _unpack(g, tag + f"s{step}_pslice__", offs, names)
        new = m.state_dict()
        for i, k in enumerate(names):
            got, scale = total[k].cpu().numpy(), max(1e-12, float(ref_sums[i][1]))
            cs = synth.checksum(got)
            worst_sum = max(worst_sum, (max(abs(cs[0] - ref_sums[i][0]), abs(cs[1] - ref_sums[i][1])) / scale, k))
            assert abs(cs[0] - ref_sums[i][0]) <= 1e-3 * scale + 1e-9, (k, step)
            assert abs(cs[1] - ref_sums[i][1]) <= 1e-3 * scale + 1e-9, (k, step)
            sl, ref = _slice(total[k], every), ref_g[k]
            worst_g = max(worst_g, (float(np.abs(sl - ref).max() / (np.abs(ref).max() + 1e-12)), k))
            np.testing.assert_allclose(sl, ref, rtol=2e-3, atol=1e-7 + 2e-4 * np.abs(ref).max(), err_msg=f"{k} step {step}")
            a, b = _slice(new[k], every), ref_p[k]
            small = np.abs(ref) < 1e-7 * max(1e-12, float(np.abs(ref).max()))           # update direction ill-defined there
            worst_p = max(worst_p, (float(np.abs(np.where(small, b, a) - b).max()), k))
            np.testing.assert_allclose(np.where(small, b, a), b, rtol=0, atol=2e-5, err_msg=f"{k} after step {step}")
        step += 1
    assert step == n_micro // A and m.step_count == step
    print(f"{tag}: worst gradient checksum error {worst_sum[0]:.2e} of the abs-sum ({worst_sum[1]}), worst gradient-slice error "
          f"{worst_g[0]:.2e} of max|ref| ({worst_g[1]}), worst parameter error after Adam {worst_p[0]:.2e} ({worst_p[1]})")
