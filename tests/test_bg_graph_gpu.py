"""The fixed-shape ("padded") background step and its hipGraph capture (csrc/bg_compact.hip, BackgroundScene(..., bg_capacity=C),
graph.GraphedBackgroundStep): the three kernels alone against torch, the padded eager step against the reference's own run
(tests/golden/bg_train_*.npz, N = 96 rays of which 64 leave the bound) and against the compact step, one capture replayed over batches
with no, some and only background rays, the refusals (overflow, cameras outside the bound) and the shared fp16 loss scaler.

Shapes: the kernels from 1 ray to 8193 (one slab of the 1024-thread scan, its wave boundary 63 / 64 / 65, nine slabs); the scene-level
tests on synth.BUILDING + synth.DENSE_BG with 64 rays x 16 samples (8 for the background)."""
import functools
import os

import numpy as np
import pytest
import torch

import synth
from test_background_gpu import CENTER, RADIUS, G, _check_grads, _dev, _models

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- kernels
def _masks(N, rng):
    last = np.zeros(N, np.int32)
    last[-1] = 1
    return dict(none=np.zeros(N, np.int32), all=np.ones(N, np.int32), alternating=(np.arange(N) % 2).astype(np.int32), last=last,
                random=(rng.uniform(size=N) < 0.4).astype(np.int32))


@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000, 8193])
def test_compaction_vs_nonzero_and_gathers(N):
    from switch_nerf_amd import ops
    rng = np.random.default_rng(900 + N)
    rays = _dev(rng.standard_normal((N, 8)).astype(np.float32))
    img = _dev(rng.integers(0, 1000, N).astype(np.int64))
    pad = ops.bg_pad_ray(CENTER, RADIUS)
    pad_t = torch.tensor(list(pad), dtype=torch.float32, device="cuda")
    for name, mask in _masks(N, rng).items():
        has_bg = _dev(mask)
        nz = has_bg.nonzero().view(-1)
        n = nz.numel()
        for C in sorted({1, max(1, N // 2), N}):
            idx_bg, n_bg, rays_b, img_b = ops.bg_compact(has_bg, rays, img, C, pad)
            k = min(n, C)
            what = (name, N, C)
            assert int(n_bg.item()) == n, what                                  # the TRUE count, also above C
            assert idx_bg.shape == (C,) and rays_b.shape == (C, 8) and img_b.shape == (C,) and img_b.dtype == torch.int64
            assert torch.equal(idx_bg[:k], nz[:k]), what
            assert torch.equal(rays_b[:k], rays[nz[:k]]), what
            assert torch.equal(img_b[:k], img[nz[:k]]), what
            assert (idx_bg[k:] == 0).all() and (img_b[k:] == 0).all(), what     # padding (k = C when n >= C: no padding rows)
            assert torch.equal(rays_b[k:], pad_t.expand(C - k, 8)), what
            again = ops.bg_compact(has_bg, rays, img, C, pad)
            for a, b in zip((idx_bg, n_bg, rays_b, img_b), again):
                assert torch.equal(a, b), what
    # int32 image indices take the kernel's other instantiation
    has_bg = _dev(_masks(N, rng)["random"])
    nz = has_bg.nonzero().view(-1)
    idx_bg, n_bg, _, img_b = ops.bg_compact(has_bg, rays, img.int(), N, pad)
    assert img_b.dtype == torch.int32 and torch.equal(img_b[: nz.numel()], img.int()[nz]) and (img_b[nz.numel():] == 0).all()
    with pytest.raises(ValueError, match="capacity"):
        ops.bg_compact(has_bg, rays, img, N + 1, pad)
    with pytest.raises(ValueError, match="capacity"):
        ops.bg_compact(has_bg, rays, img, 0, pad)


@pytest.mark.parametrize("bound", ["ellipsoid", "unit"])
def test_padding_ray_is_benign(bound):
    """Origin at the bound's centre, direction (0, 0, 1), near 0, far beyond the bound: the ray has a background segment, is inside the
    bound, and its background samples / points / metric depths are finite (so is everything computed from them)."""
    from switch_nerf_amd import ops
    center, radius = (CENTER, RADIUS) if bound == "ellipsoid" else (None, None)
    pad = np.array(list(ops.bg_pad_ray(center, radius)), np.float32)
    c = np.zeros(3, np.float32) if center is None else center
    np.testing.assert_array_equal(pad[:7], np.concatenate([c, [0, 0, 1, 0]]).astype(np.float32))
    r = _dev(pad[None])
    _, fg_far, _, has_bg, n_out = ops.fg_bounds(r, center, radius)
    assert int(has_bg.item()) == 1 and int(n_out.item()) == 0 and pad[7] > float(fg_far.item())
    for S in (8, 32):
        z, dreal, pe = ops.bg_sample_pe(r, center, radius, S, 12, torch.float32, 128)
        assert torch.isfinite(z).all() and torch.isfinite(dreal).all() and torch.isfinite(pe).all()


def _blend_case(n_bg, N=300, C=130, seed=77):
    rng = np.random.default_rng(seed + n_bg)
    f = lambda *s: _dev(rng.standard_normal(s).astype(np.float32))
    idx = np.zeros(C, np.int64)
    n_valid = min(n_bg, C)
    idx[:n_valid] = np.sort(rng.permutation(N)[:n_valid])
    return dict(N=N, C=C, n=n_valid, idx=_dev(idx), n_bg=torch.tensor([n_bg], dtype=torch.int32, device="cuda"), lam=f(N).abs(),
                rgb=f(N, 3), depth=f(N), rgb_b=f(C, 3), depth_b=f(C), d_rgb=f(N, 3))


@pytest.mark.parametrize("n_bg", [0, 1, 130, 131])      # 131 > C: an overflowing count blends the C rows there are
def test_blend_kernels_vs_torch(n_bg):
    from switch_nerf_amd import ops
    t = _blend_case(n_bg)
    n, sel = t["n"], t["idx"][: t["n"]]
    lam_b = t["lam"].index_select(0, sel)
    ref_rgb = t["rgb"].index_add(0, sel, t["rgb_b"][:n] * lam_b[:, None])
    ref_depth = t["depth"].index_add(0, sel, t["depth_b"][:n] * lam_b)
    rgb, depth = ops.bg_blend_fwd(t["rgb"].clone(), t["depth"].clone(), t["idx"], t["n_bg"], t["lam"], t["rgb_b"], t["depth_b"])
    assert torch.equal(rgb, ref_rgb) and torch.equal(depth, ref_depth)          # the valid prefix added, every other row untouched
    if n == 0:
        assert torch.equal(rgb, t["rgb"]) and torch.equal(depth, t["depth"])
    d_lam, d_rgb_b = ops.bg_blend_bwd(t["d_rgb"], t["idx"], t["n_bg"], t["lam"], t["rgb_b"])
    d_sel = t["d_rgb"].index_select(0, sel)
    assert torch.equal(d_rgb_b[:n], d_sel * lam_b[:, None])
    assert (d_rgb_b[n:] == 0).all() and not torch.signbit(d_rgb_b[n:]).any()    # padding: exactly +0
    ref_lam = (d_sel * t["rgb_b"][:n]).sum(-1).cpu().numpy()
    got = d_lam.cpu().numpy()
    off = np.ones(t["N"], bool)
    off[sel.cpu().numpy()] = False
    assert (got[off] == 0).all()
    err, ulp = np.abs(got[~off] - ref_lam), np.spacing(np.abs(ref_lam))
    print(f"n_bg {n_bg}: d_lam worst error {float((err / ulp).max()) if n else 0.0:.2f} ulp")
    assert (err <= ulp).all()


# ---------------------------------------------------------------------------------------------------------------- eager padded step
def _grad_ref(model, pre):
    """A model's gradients in the layout _check_grads reads from a golden file (oracle/gen_golden.py: checksum + strided slice)."""
    out = {}
    for k, t in model.grad_dict().items():
        a = t.cpu().numpy()
        out["gsum__" + pre + k] = synth.checksum(a)
        out["gslice__" + pre + k] = a.reshape(-1)[:: max(1, a.size // 499)][:499].copy()
    return out


@functools.lru_cache(maxsize=None)
def _golden_step(tag, C):
    """One fp32 training step (no Adam) on the fixture's batch; C = None: the compact form, else bg_capacity = C with the fixture's
    background noise padded to C rows.  Run once per (tag, C) and shared by the tests below."""
    from switch_nerf_amd.background import BackgroundScene
    g = np.load(os.path.join(G, f"bg_train_{tag}.npz"))
    N, S, Fn, chunk, n_bg = int(g["N"]), int(g["S"]), int(g["F"]), int(g["chunk"]), int(g["n_bg"])
    m, b = _models(torch.float32, int(g["seed"]), int(g["seed_bg"]), float(g["gate_scale"]))
    scene = BackgroundScene(m, b, CENTER, RADIUS)
    rays, img, rgbs = synth.make_bg_rays(83, N)
    rows = n_bg if C is None else C

    def padded(a):                       # the first n_bg rows are the fixture's, the padding rows' values are never used
        return _dev(np.concatenate([a, np.full((rows - n_bg,) + a.shape[1:], 0.5, np.float32)], 0))
    kw, perturb = {}, float(g["perturb"])
    if perturb > 0:
        kw = dict(perturb_rand=_dev(g["perturb_rand"]), perturb_rand_bg=padded(g["perturb_rand_bg"]))
        if Fn:
            kw.update(fine_u=_dev(g["fine_u"]), fine_u_bg=padded(g["fine_u_bg"]))
    st = scene.train_step(_dev(rgbs), _dev(rays), _dev(img), S, chunk, perturb=perturb, optimizer_step=False, fine_samples=Fn,
                          bg_capacity=C, **kw)
    ctx = st["ctx"]
    out = {k: ctx[k].cpu().numpy() for k in ("fg_far", "fg_rgb", "rgb", "depth", "depth_variance")}
    out.update(Nb=ctx["Nb"], loss=st["loss"].item(), loss_t=st["loss"].cpu(), m=m, b=b, grads={**_grad_ref(m, ""), **_grad_ref(b, "bg__")},
               present=st["bg_nerf_rays_present"])
    return out


@pytest.mark.parametrize("C", [96, 64])
@pytest.mark.parametrize("tag", ["coarse_det", "coarse", "fine"])
def test_padded_train_step_vs_reference_golden_fp32(tag, C):
    """The comparisons and tolerances of test_background_gpu.py::test_background_train_step_vs_reference_golden_fp32."""
    g = np.load(os.path.join(G, f"bg_train_{tag}.npz"))
    r = _golden_step(tag, C)
    assert r["Nb"] == int(g["n_bg"]) == 64 and r["present"]
    np.testing.assert_allclose(r["fg_far"], g["fg_far"], rtol=1e-6)
    np.testing.assert_allclose(r["fg_rgb"], g["fg_rgb"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(r["rgb"] - r["fg_rgb"], g["bg_rgb"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(r["rgb"], g["rgb"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(r["depth"], g["depth"], rtol=2e-3, atol=1e-4)
    np.testing.assert_allclose(r["depth_variance"], g["depth_variance"], rtol=2e-3, atol=1e-6)
    np.testing.assert_allclose(r["loss"], float(g["loss"]), rtol=1e-5)
    w1 = _check_grads(g, "", r["m"])
    w2 = _check_grads(g, "bg__", r["b"])
    print(f"{tag} C={C}: worst relative gradient-slice error fg {w1:.2e} bg {w2:.2e}")


@pytest.mark.parametrize("tag", ["coarse_det", "coarse", "fine"])
def test_no_padding_changes_nothing(tag):
    """bg_capacity = n_bg: the same rows in the same order as the compact form - rgb, depth and loss bit for bit, the gradients under
    _check_grads with the compact form's as the reference.  C = 96 against C = 64 under the same gradient rule (the weight-gradient split
    count follows the row count, so their sums associate differently); what a ray renders does not depend on the padding."""
    compact, exact, wide = _golden_step(tag, None), _golden_step(tag, 64), _golden_step(tag, 96)
    for k in ("rgb", "depth", "fg_rgb", "depth_variance"):
        np.testing.assert_array_equal(exact[k], compact[k], err_msg=k)
    assert torch.equal(exact["loss_t"], compact["loss_t"])
    w = [_check_grads(compact["grads"], pre, exact[mk]) for pre, mk in (("", "m"), ("bg__", "b"))]
    w += [_check_grads(exact["grads"], pre, wide[mk]) for pre, mk in (("", "m"), ("bg__", "b"))]
    print(f"{tag}: worst relative gradient-slice error C=n_bg vs compact fg {w[0]:.2e} bg {w[1]:.2e}; C=96 vs C=64 fg {w[2]:.2e} bg {w[3]:.2e}")


def test_render_rays_passes_bg_capacity_through():
    from argparse import Namespace
    from switch_nerf_amd import rendering
    m, b = _models(torch.float32, 101, 102)
    N, S = 64, 16
    rays, img, _ = synth.make_bg_rays(104, N)
    h = Namespace(coarse_samples=S, fine_samples=0, model_chunk_size=1024, perturb=0.0, use_sigma_noise=False, sigma_noise_std=0.0,
                  use_cascade=False, bg_capacity=48)
    m.eval()
    res, present = rendering.render_rays(m, b, _dev(rays), _dev(img), h, CENTER, RADIUS, True, False, False)
    scene = rendering.background_scene(m, b, CENTER, RADIUS)
    ctx = scene.forward(_dev(rays), _dev(img), S, 1024, training=False, bg_capacity=48)
    assert ctx["C"] == 48 and ctx["Nb"] is None and ctx["n_bg_dev"].shape == (1,) and ctx["n_out_dev"].shape == (1,)
    scene.read_counts(ctx)
    assert present and 0 < ctx["Nb"] <= 48
    assert torch.equal(res["rgb_coarse"], ctx["rgb"]) and torch.equal(res["depth_coarse"], ctx["depth"])
    h.bg_capacity = 4
    with pytest.raises(RuntimeError, match=rf"n_bg = {ctx['Nb']} .* bg_capacity = 4"):
        rendering.render_rays(m, b, _dev(rays), _dev(img), h, CENTER, RADIUS, True, False, False)
    bad = rays.copy()
    bad[:, :3] += 3.0
    h.bg_capacity = 64
    with pytest.raises(Exception, match="bounded by the unit sphere"):
        rendering.render_rays(m, b, _dev(bad), _dev(img), h, CENTER, RADIUS, True, False, False)


# ---------------------------------------------------------------------------------------------------------------- captured step
N_G, S_G, SEG_G = 64, 16, 1024


def _batches():
    """No ray, some rays, every ray leaves the bound (fg_far lies between ~0.45 and ~0.95 for these origins)."""
    return [synth.make_rays(301, N_G, far=0.3), synth.make_bg_rays(302, N_G), synth.make_rays(303, N_G, far=5.0)]


def _scene(dtype, seed=None):
    from switch_nerf_amd.background import BackgroundScene
    m, b = _models(dtype, 201, 202)
    scene = BackgroundScene(m, b, CENTER, RADIUS)
    if seed is not None:
        scene.set_device_noise(seed)
    return scene


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_one_capture_replayed_over_batches_equals_eager_padded(dtype):
    from switch_nerf_amd.graph import GraphedBackgroundStep
    batches = _batches()
    graphed, eager, compact = _scene(dtype, 5), _scene(dtype, 5), _scene(dtype, 5)
    rays0, img0, rgbs0 = batches[1]
    step = GraphedBackgroundStep(graphed, _dev(rgbs0), _dev(rays0), _dev(img0), S_G, SEG_G, perturb=1.0, noise_std=1.0)
    assert step.bg_capacity == N_G
    assert graphed.noise_state_dict()["step"] == 0                    # the warm-up's advances were put back
    seen = []
    for i, (rays, img, rgbs) in enumerate(batches):
        args = (_dev(rgbs), _dev(rays), _dev(img))
        bg_before, bg_steps = graphed.bg.flat.clone(), graphed.bg.step_count
        ra = step(*args)
        rb = eager.train_step(*args, S_G, SEG_G, perturb=1.0, noise_std=1.0, bg_capacity=N_G)
        n_bg = ra["ctx"]["Nb"]
        seen.append(n_bg)
        assert n_bg == rb["ctx"]["Nb"] and ra["bg_nerf_rays_present"] == rb["bg_nerf_rays_present"] == (n_bg > 0)
        assert torch.equal(graphed.nerf.flat, eager.nerf.flat), i
        assert torch.equal(graphed.bg.flat, eager.bg.flat), i
        assert torch.equal(ra["loss"], rb["loss"]) and torch.equal(ra["rgb"], rb["rgb"]), i
        assert graphed.noise_state_dict()["step"] == eager.noise_state_dict()["step"] == i + 1
        assert (graphed.nerf.step_count, graphed.bg.step_count) == (eager.nerf.step_count, eager.bg.step_count)
        if i == 0:                                                    # no background ray: the background model is left alone
            assert n_bg == 0
            assert float(graphed.bg.grad.abs().max()) == 0.0 and float(eager.bg.grad.abs().max()) == 0.0
            assert torch.equal(graphed.bg.flat, bg_before) and graphed.bg.step_count == bg_steps == 0
            rc = compact.train_step(*args, S_G, SEG_G, perturb=1.0, noise_std=1.0)
            assert rc["ctx"]["Nb"] == 0 and torch.equal(ra["rgb"], rc["rgb"])
        else:
            assert not torch.equal(graphed.bg.flat, bg_before) and graphed.bg.step_count == bg_steps + 1
    assert seen[0] == 0 and 0 < seen[1] < N_G and seen[2] == N_G, seen


def test_captured_step_refuses_overflow_and_unbounded_cameras():
    from switch_nerf_amd.graph import GraphedBackgroundStep
    scene = _scene(torch.float32, 5)
    rays, img, rgbs = synth.make_bg_rays(302, N_G)
    step = GraphedBackgroundStep(scene, _dev(rgbs), _dev(rays), _dev(img), S_G, SEG_G, bg_capacity=8)
    flats = lambda: (scene.nerf.flat.clone(), scene.bg.flat.clone())
    before = flats()
    with pytest.raises(RuntimeError, match=r"n_bg = \d+ .* bg_capacity = 8"):
        step(_dev(rgbs), _dev(rays), _dev(img))
    assert step.res["ctx"]["Nb"] > 8
    bad = rays.copy()
    bad[:, :3] += 3.0
    with pytest.raises(Exception, match="bounded by the unit sphere"):
        step(_dev(rgbs), _dev(bad), _dev(img))
    after = flats()
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert (scene.nerf.step_count, scene.bg.step_count) == (0, 0)
    few = rays.copy()                                                 # the same batch with all but its first 8 rays cut short
    few[8:, 7] = 0.3
    res = step(_dev(rgbs), _dev(few), _dev(img))
    assert 0 < res["ctx"]["Nb"] <= 8 and torch.isfinite(res["loss"])
    assert (scene.nerf.step_count, scene.bg.step_count) == (1, 1)
    assert not torch.equal(scene.nerf.flat, before[0]) and not torch.equal(scene.bg.flat, before[1])
    with pytest.raises(ValueError, match="bg_capacity"):
        GraphedBackgroundStep(scene, _dev(rgbs), _dev(rays), _dev(img), S_G, SEG_G, bg_capacity=N_G + 1)


def test_captured_step_fp16_one_shared_grad_scaler():
    """test_background_gpu.py::test_background_fp16_one_shared_grad_scaler on replayed steps: an overflow in the background gradient alone
    halves the shared scale, skips the background step only and resets the growth tracker.  The non-finite value is planted the same way
    (behind scene.backward), here while the second step is captured, so its replay carries it."""
    from switch_nerf_amd.graph import GraphedBackgroundStep
    rays, img, rgbs = synth.make_bg_rays(131, N_G)
    scene = _scene(torch.float16)
    m, b = scene.nerf, scene.bg
    assert m.loss_scaler is b.loss_scaler is scene.loss_scaler
    m.loss_scaler.scale = 1024.0
    m.loss_scaler._good = 7
    args = (_dev(rgbs), _dev(rays), _dev(img))
    clean = GraphedBackgroundStep(scene, *args, S_G, SEG_G, perturb=0.0, noise_std=0.0)
    st = clean(*args)
    assert st["ctx"]["Nb"] > 0 and m.step_count == 1 and b.step_count == 1
    assert m.loss_scaler.scale == 1024.0 and b.loss_scaler.scale == 1024.0 and m.loss_scaler._good == 8
    orig_backward = scene.backward

    def poisoned(*a, **k):
        orig_backward(*a, **k)
        b.grad[:1].fill_(float("inf"))                                  # (a fill launch: an element assignment copies from the host)
    scene.backward = poisoned
    bad = GraphedBackgroundStep(scene, *args, S_G, SEG_G, perturb=0.0, noise_std=0.0)
    scene.backward = orig_backward
    fg_before, bg_before = m.flat.clone(), b.flat.clone()
    bad(*args)
    assert m.step_count == 2 and b.step_count == 1                      # each optimizer skips on ITS OWN found_inf
    assert (m.flat != fg_before).any() and torch.equal(b.flat, bg_before)
    assert m.loss_scaler.scale == 512.0 and b.loss_scaler.scale == 512.0 and m.loss_scaler._good == 0
    assert b.loss_scaler.state_dict()["_growth_tracker"] == 0 and b.loss_scaler.skipped == 1
    clean(*args)                                                        # the replay reads the backed-off scale from the device
    assert m.step_count == 3 and b.step_count == 2 and m.loss_scaler.scale == 512.0 and m._applied_loss_scale == 512.0
