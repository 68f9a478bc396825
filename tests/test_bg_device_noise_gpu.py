"""Seeded device-side noise for scenes with a background model (csrc/rng.hip swn_rng_fill_rows, csrc/bounds.hip swn_bg_sample_pe_rng,
BackgroundScene.set_device_noise): the row-addressed generator against the plain-Python restatement (tests/philox_rows_restate.py), and
the scene-level properties the addressing exists for - a background ray's noise depends on (seed, step, global ray) only.

Scene-level shapes: synth.BUILDING + synth.DENSE_BG in bf16, 64 rays of synth.make_bg_rays(700) x 16 samples (8 for the background)."""
import types

import numpy as np
import pytest
import torch

import philox_rows_restate as RR
import synth

pytestmark = pytest.mark.gpu

SEED = 0x0123456789ABCDEF
CENTER, RADIUS = synth.SPHERE_CENTER, synth.SPHERE_RADIUS
N_ROWS = 37
# a fixed permutation-with-repeats of range(0, 200): unsorted, 37 entries, three values twice
ROW_INDEX = np.random.default_rng(4242).permutation(200)[:34].tolist() + [199, 0, 199]
ROW_INDEX[5], ROW_INDEX[20] = ROW_INDEX[11], ROW_INDEX[3]
assert len(ROW_INDEX) == N_ROWS and len(set(ROW_INDEX)) < N_ROWS and ROW_INDEX != sorted(ROW_INDEX)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _step(v):
    from switch_nerf_amd import ops
    return ops.rng_step_tensor(v, "cuda")


def _idx():
    return torch.tensor(ROW_INDEX, dtype=torch.int64, device="cuda")


# ---------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("step", [0, 3])
@pytest.mark.parametrize("row_base", [0, 5, (1 << 33) - 3])
@pytest.mark.parametrize("per_row", [1, 7, 13, 16])
def test_uniform_rows_equal_restatement(per_row, row_base, step):
    from switch_nerf_amd import ops
    st, idx = _step(step), _idx()
    got = {}
    for domain in (ops.RNG_DOMAIN_FG, ops.RNG_DOMAIN_BG):
        out = ops.rng_fill_rows(N_ROWS, per_row, row_base, idx, ops.RNG_UNIFORM, SEED, st, ops.RNG_FINE_U, domain, index_limit=200)
        assert out.shape == (N_ROWS, per_row)
        got[domain] = out.cpu().numpy()
        ref = RR.uniform_rows(SEED, step, ops.RNG_FINE_U, domain, row_base, ROW_INDEX, per_row)
        assert np.array_equal(got[domain].view(np.uint32), ref.view(np.uint32)), (domain, int((got[domain] != ref).sum()))
    assert not np.array_equal(got[0], got[1])                       # the domain is part of the key


@pytest.mark.parametrize("kind", [0, 1])
def test_identity_rows_equal_the_contiguous_fill(kind):
    """row_index None, domain 0: swn_rng_fill(n_rows * per_row, row_base * per_row) bit for bit (the aligned and the unaligned store path
    of either kernel; per_row 16 takes the 16-byte stores of the row kernel)."""
    from switch_nerf_amd import ops
    st = _step(2)
    for per_row in (13, 16):
        for row_base in (0, 5):
            rows = ops.rng_fill_rows(N_ROWS, per_row, row_base, None, kind, SEED, st, ops.RNG_SIGMA, ops.RNG_DOMAIN_FG, scale=0.5)
            flat = ops.rng_fill(N_ROWS * per_row, row_base * per_row, kind, SEED, st, ops.RNG_SIGMA, scale=0.5)
            assert torch.equal(rows.view(-1), flat), (per_row, row_base)


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("per_row", [7, 13])
def test_normal_rows_match_float64_restatement(per_row, scale):
    """Absolute tolerance 1e-5 * scale, the bound tests/test_device_noise_gpu.py derives for the same arithmetic (|r| <= 5.77, fp32 theta,
    logf / sqrtf / sincosf): the row kernel calls the same philox_normal_pair on the same words.  Row j drawn alone equals row j of the
    whole draw bit for bit: with an odd per_row a Box-Muller pair straddles two global rows and each row takes only its own half."""
    from switch_nerf_amd import ops
    st, idx = _step(1), _idx()
    for row_base in (0, 5):
        out = ops.rng_fill_rows(N_ROWS, per_row, row_base, idx, ops.RNG_NORMAL, SEED, st, ops.RNG_SIGMA, ops.RNG_DOMAIN_BG, scale, 200)
        ref = RR.normal_rows(SEED, 1, ops.RNG_SIGMA, ops.RNG_DOMAIN_BG, row_base, ROW_INDEX, per_row, scale=scale)
        err = np.abs(out.cpu().numpy().astype(np.float64) - ref).max()
        print(f"normal rows: per_row {per_row} scale {scale} row_base {row_base} max abs err {err:.3e} (bound {1e-5 * scale:.1e})")
        assert err <= 1e-5 * scale, err
        for j in (0, 1, 17, N_ROWS - 1):
            alone = ops.rng_fill_rows(1, per_row, row_base, idx[j:j + 1].clone(), ops.RNG_NORMAL, SEED, st, ops.RNG_SIGMA,
                                      ops.RNG_DOMAIN_BG, scale, 200)
            assert torch.equal(alone[0], out[j]), j


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("per_row", [7, 16])
def test_rows_write_nothing_outside_the_destination(per_row, kind):
    from switch_nerf_amd import ops
    st, idx = _step(0), _idx()
    n = N_ROWS * per_row
    whole = ops.rng_fill_rows(N_ROWS, per_row, 5, idx, kind, SEED, st, ops.RNG_JITTER, ops.RNG_DOMAIN_BG, index_limit=200)
    for off in (4, 3):                                              # a 16-byte aligned and an unaligned slice
        buf = torch.full((n + 16,), -7.0, device="cuda")
        ops.rng_fill_rows(N_ROWS, per_row, 5, idx, kind, SEED, st, ops.RNG_JITTER, ops.RNG_DOMAIN_BG, index_limit=200, out=buf[off:off + n])
        assert torch.equal(buf[off:off + n], whole.view(-1))
        assert bool((buf[:off] == -7.0).all()) and bool((buf[off + n:] == -7.0).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("ray_base", [0, 5])
def test_bg_sample_pe_rng_twin(ray_base, dtype):
    """The in-kernel jitter equals swn_rng_fill_rows (uniform, domain 1, stream 0) followed by swn_bg_sample_pe, bit for bit."""
    from switch_nerf_amd import _lib, ops
    _lib.use_half("bf16")
    N, S = N_ROWS, 13
    rays = _dev(synth.make_bg_rays(77, N)[0])
    st, idx = _step(3), _idx()
    u = ops.rng_fill_rows(N, S, ray_base, idx, ops.RNG_UNIFORM, SEED, st, ops.RNG_JITTER, ops.RNG_DOMAIN_BG, index_limit=200)
    z0, d0, pe0 = ops.bg_sample_pe(rays, CENTER, RADIUS, S, 12, dtype, 128, u, 1.0)
    z1, d1, pe1 = ops.bg_sample_pe_rng(rays, CENTER, RADIUS, S, 12, dtype, 128, SEED, st, ray_base, idx, 200, 1.0)
    assert torch.equal(z0, z1) and torch.equal(d0, d1) and torch.equal(pe0, pe1)
    zd, dd, ped = ops.bg_sample_pe(rays, CENTER, RADIUS, S, 12, dtype, 128, None, 0.0)
    assert not torch.equal(zd, z1) and not torch.equal(dd, d1) and not torch.equal(ped, pe1)     # (the jitter did move the samples)
    # the identity index is the plain ray number
    ui = ops.rng_fill_rows(N, S, ray_base, None, ops.RNG_UNIFORM, SEED, st, ops.RNG_JITTER, ops.RNG_DOMAIN_BG)
    z2 = ops.bg_sample_pe(rays, CENTER, RADIUS, S, 12, dtype, 128, ui, 1.0)[0]
    assert torch.equal(z2, ops.bg_sample_pe_rng(rays, CENTER, RADIUS, S, 12, dtype, 128, SEED, st, ray_base)[0])


# ---------------------------------------------------------------------------------------------------------------- scene level
N_RAYS, S_SAMPLES, CHUNK, STD = 64, 16, 1024, 1.0
RAY_SEED = 700            # synth.make_bg_rays(700, 64): 33 of the 64 rays leave the bound (17 of every second ray, 19 + 14 by halves)


def _scene(noise_seed=None, **kw):
    from switch_nerf_amd.background import BackgroundScene
    from switch_nerf_amd.dense import DenseNeRF
    from switch_nerf_amd.model import SwitchNeRF
    m = SwitchNeRF(synth.BUILDING, dtype=torch.bfloat16)
    m.load_state_dict(synth.make_weights(41, synth.BUILDING))
    b = DenseNeRF(synth.DENSE_BG, dtype=torch.bfloat16)
    b.load_state_dict(synth.make_dense_weights(43, synth.DENSE_BG))
    scene = BackgroundScene(m, b, CENTER, RADIUS)
    if noise_seed is not None:
        scene.set_device_noise(noise_seed, **kw)
    return scene


def _batch(seed=RAY_SEED, n=N_RAYS):
    rays, img, rgbs = (_dev(a) for a in synth.make_bg_rays(seed, n))
    return rays, img, rgbs


def _train(scene, batches, fine=0, **kw):
    losses = []
    for rays, img, rgbs in batches:
        st = scene.train_step(rgbs, rays, img, S_SAMPLES, CHUNK, perturb=1.0, fine_samples=fine, noise_std=STD, **kw)
        losses.append(st["loss"].item())
    return losses, st


def _bg_draws(ctx):
    """{global position in the batch -> (z row, sigma noise row, fine u row, fine sigma noise row)} of the background rays."""
    b, Nb = ctx["bg"], ctx["Nb"]
    per = lambda k: b[k].view(Nb, -1).cpu().numpy() if k in b else np.zeros((Nb, 0), np.float32)
    parts = [b["c"]["z"].cpu().numpy(), per("sigma_noise"), per("fine_u"), per("sigma_noise_fine")]
    return ctx["idx_bg"].cpu().numpy(), parts


@pytest.mark.parametrize("fine", [0, 8])
def test_same_seed_same_run(fine):
    batches = [_batch(RAY_SEED + i) for i in range(3)]
    runs = []
    for seed in (11, 11, 12):
        sc = _scene(seed)
        losses, st = _train(sc, batches, fine)
        assert 0 < st["ctx"]["Nb"] < N_RAYS
        assert sc.noise_state_dict() == dict(seed=seed, step=3, ray_base=0)
        runs.append((losses, sc.nerf.flat.clone(), sc.bg.flat.clone()))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
    assert runs[0][0] != runs[2][0]


@pytest.mark.parametrize("fine", [0, 8])
def test_subset_invariance(fine):
    """Every second ray of the batch, addressed by its position in the full batch (ray_index): each kept background ray's sample depths,
    sigma noise and fine u are those of the full batch's run.  (rgb is not compared: the foreground's routing capacity depends on the
    batch.)"""
    rays, img, _ = _batch()
    kw = dict(perturb=1.0, fine_samples=fine, noise_std=STD)
    full = _scene(11, ray_base=5).forward(rays, img, S_SAMPLES, CHUNK, **kw)
    keep = torch.arange(0, N_RAYS, 2, device="cuda")
    sub = _scene(11, ray_base=5).forward(rays[keep].contiguous(), img[keep].contiguous(), S_SAMPLES, CHUNK, ray_index=keep, **kw)
    assert 0 < sub["Nb"] < full["Nb"] < N_RAYS and full["Nb"] == 33 and sub["Nb"] == 17
    pos_f, parts_f = _bg_draws(full)
    pos_s, parts_s = _bg_draws(sub)
    pos_s = keep.cpu().numpy()[pos_s]                               # position in the full batch
    rows = [int(np.nonzero(pos_f == p)[0][0]) for p in pos_s]
    for a, b in zip(parts_f, parts_s):
        assert a.shape[1] == b.shape[1] and np.array_equal(a[rows].view(np.uint32), b.view(np.uint32))
    assert parts_f[1].shape[1] == S_SAMPLES // 2 and parts_f[2].shape[1] == fine // 2 == parts_f[3].shape[1]


@pytest.mark.parametrize("fine", [0, 8])
def test_rank_split(fine):
    """The two halves of the batch with ray_base 0 and 32 (parallel.shard_rays(..., model=scene)) reproduce the full batch's background
    draws row for row."""
    from switch_nerf_amd import parallel
    rays, img, _ = _batch()
    kw = dict(perturb=1.0, fine_samples=fine, noise_std=STD)
    pos_f, parts_f = _bg_draws(_scene(11).forward(rays, img, S_SAMPLES, CHUNK, **kw))
    pos, parts = [], []
    for rank in (0, 1):
        sc = _scene(11)
        lo, hi = parallel.shard_rays(N_RAYS, rank, 2, model=sc)
        assert (lo, hi) == (32 * rank, 32 * rank + 32) and sc.noise_state_dict()["ray_base"] == lo == sc.nerf.noise_state_dict()["ray_base"]
        ctx = sc.forward(rays[lo:hi].contiguous(), img[lo:hi].contiguous(), S_SAMPLES, CHUNK, **kw)
        assert ctx["Nb"] > 0
        p, q = _bg_draws(ctx)
        pos.append(p + lo)
        parts.append(q)
    assert np.array_equal(np.concatenate(pos), pos_f)
    for k, a in enumerate(parts_f):
        assert np.array_equal(np.concatenate([parts[0][k], parts[1][k]]).view(np.uint32), a.view(np.uint32)), k


def test_resume():
    """noise_state_dict() after step 2, loaded into a fresh scene with copied parameters and Adam state, reproduces steps 3-4."""
    batches = [_batch(RAY_SEED + i) for i in range(4)]
    a = _scene(11, ray_base=7)
    _train(a, batches[:2], fine=8)
    sd = a.noise_state_dict()
    assert sd == dict(seed=11, step=2, ray_base=7)
    b = _scene()
    for src, dst in ((a.nerf, b.nerf), (a.bg, b.bg)):
        dst.flat.copy_(src.flat)
        dst.m.copy_(src.m)
        dst.v.copy_(src.v)
        dst.step_count = src.step_count
        dst.refresh_compute_copies()
    b.load_noise_state_dict(sd)
    la, _ = _train(a, batches[2:], fine=8)
    lb, _ = _train(b, batches[2:], fine=8)
    assert la == lb and torch.equal(a.nerf.flat, b.nerf.flat) and torch.equal(a.bg.flat, b.bg.flat)
    assert a.noise_state_dict() == b.noise_state_dict() == dict(seed=11, step=4, ray_base=7)


def test_batch_without_background_rays_advances_once():
    sc = _scene(11, step=5)
    rays, img, rgbs = (_dev(a) for a in synth.make_rays(703, N_RAYS, far=0.3))      # every far below the bound
    st = sc.train_step(rgbs, rays, img, S_SAMPLES, CHUNK, perturb=1.0, noise_std=STD)
    assert st["ctx"]["Nb"] == 0 and sc.bg.step_count == 0 and sc.nerf.step_count == 1
    assert sc.noise_state_dict()["step"] == 6 and int(sc.nerf.noise.step.item()) == 6
    _train(sc, [_batch()])
    assert sc.noise_state_dict()["step"] == 7


def test_supplied_noise_wins():
    rays, img, _ = _batch()
    Nb, Sb, Fn = 33, S_SAMPLES // 2, 8
    g = torch.Generator(device="cuda").manual_seed(9)
    r = lambda *s: torch.rand(*s, device="cuda", generator=g)
    n = lambda *s: torch.randn(*s, device="cuda", generator=g)
    kw = dict(perturb_rand=r(N_RAYS, S_SAMPLES), perturb_rand_bg=r(Nb, Sb), sigma_noise=n(N_RAYS * S_SAMPLES), sigma_noise_bg=n(Nb * Sb),
              fine_u=r(N_RAYS, Fn), fine_u_bg=r(Nb, Fn // 2), sigma_noise_fine=n(N_RAYS * Fn), sigma_noise_bg_fine=n(Nb * (Fn // 2)))
    outs = []
    for seed in (11, None):
        ctx = _scene(seed).forward(rays, img, S_SAMPLES, CHUNK, perturb=1.0, fine_samples=Fn, noise_std=STD, **kw)
        assert ctx["Nb"] == Nb and "sigma_noise" not in ctx["bg"] and "fine_u" not in ctx["bg"]
        outs.append((ctx["rgb"].clone(), ctx["bg"]["z"].clone(), ctx["z"].clone()))
    for x, y in zip(*outs):
        assert torch.equal(x, y)


def test_no_framework_draw_left():
    sc = _scene(11)
    rays, img, rgbs = _batch()
    before = torch.cuda.get_rng_state()
    st = sc.train_step(rgbs, rays, img, S_SAMPLES, CHUNK, perturb=1.0, fine_samples=8, noise_std=STD)
    assert st["ctx"]["Nb"] == 33 and torch.equal(torch.cuda.get_rng_state(), before)
    b = st["ctx"]["bg"]
    assert b["sigma_noise"].numel() == 33 * 8 and b["fine_u"].shape == (33, 4) and b["sigma_noise_fine"].numel() == 33 * 4


def test_mixed_noise_sources_are_refused():
    rays, img, _ = _batch()
    sc = _scene()
    sc.nerf.set_device_noise(5)                                     # the model's own noise on, the scene's off
    with pytest.raises(RuntimeError, match="BackgroundScene.set_device_noise"):
        sc.forward(rays, img, S_SAMPLES, CHUNK, perturb=1.0)
    sc.nerf.set_device_noise(None)
    sc.bg.set_device_noise(5)
    with pytest.raises(RuntimeError, match="background model"):
        sc.forward(rays, img, S_SAMPLES, CHUNK, perturb=1.0)


def test_detach_hands_the_foreground_its_noise_state_back():
    sc = _scene()
    sc.nerf.set_device_noise(3, step=4, ray_base=9)
    own_step = sc.nerf.noise.step
    sc.set_device_noise(11)
    assert sc.nerf.noise.step is sc.noise.step and sc.nerf.noise_state_dict() == dict(seed=11, step=0, ray_base=0)
    assert not sc.bg.device_noise                                   # the background model never holds a counter
    sc.detach()
    assert not sc.device_noise and sc.nerf.noise.step is own_step
    assert sc.nerf.noise_state_dict() == dict(seed=3, step=4, ray_base=9)


def test_render_rays_route():
    from switch_nerf_amd import rendering
    rays, img, _ = _batch()
    hp = types.SimpleNamespace(coarse_samples=S_SAMPLES, fine_samples=8, model_chunk_size=CHUNK, perturb=1.0, use_sigma_noise=True,
                               sigma_noise_std=STD)
    c, r = _dev(CENTER), _dev(RADIUS)
    sc = _scene()
    with pytest.raises(NotImplementedError, match="BackgroundScene.set_device_noise"):
        rendering.render_rays(sc.nerf, sc.bg, rays, img, types.SimpleNamespace(**vars(hp), device_noise_seed=5), c, r)
    outs = []
    for _ in range(2):
        sc = _scene()
        scene = rendering.background_scene(sc.nerf, sc.bg, c, r)
        assert scene is rendering.background_scene(sc.nerf, sc.bg, c, r)            # cached on the foreground model
        scene.set_device_noise(5, ray_base=128)
        before = torch.cuda.get_rng_state()
        with torch.no_grad():
            res, present = rendering.render_rays(sc.nerf, sc.bg, rays, img, hp, c, r)
        assert present and torch.equal(torch.cuda.get_rng_state(), before)
        assert scene.noise_state_dict() == dict(seed=5, step=1, ray_base=128)
        outs.append({k: v.clone() for k, v in res.items() if k.startswith("rgb_")})
    assert outs[0].keys() == outs[1].keys() and "rgb_fine" in outs[0]
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k
