"""Seeded device-side noise (csrc/philox.hpp, csrc/rng.hip; SwitchNeRF.set_device_noise): the kernels against the plain-Python restatement
(tests/philox_restate.py), and the model-level properties the generator exists for - same seed same run, eager == graph with noise ON,
batch-split invariance, resume, caller-supplied noise wins, no framework draw left in the step.

The model-level tests run synth.BUILDING (M = 256, E = 8) at 64 rays x 16 samples: SwitchNeRF's router and chain kernels take 128 / 256 /
512 features, so the M = 64 layer config of synth.small_cfg (a moe.MoELayer config) does not build a SwitchNeRF."""
import types

import numpy as np
import pytest
import torch

import philox_restate as R
import synth

pytestmark = pytest.mark.gpu

SEED = 0x0123456789ABCDEF


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _step(v):
    from switch_nerf_amd import ops
    return ops.rng_step_tensor(v, "cuda")


# ---------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("stream", [0, 4])
@pytest.mark.parametrize("step", [0, 3])
@pytest.mark.parametrize("base", [0, 3, (1 << 34) - 6])
def test_uniform_fill_equals_restatement(base, step, stream):
    from switch_nerf_amd import ops
    n = 1027
    out = ops.rng_fill(n, base, ops.RNG_UNIFORM, SEED, _step(step), stream).cpu().numpy()
    ref = R.uniform(SEED, step, stream, base, n)
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32)), int((out != ref).sum())


@pytest.mark.parametrize("kind", [0, 1])
def test_fill_split_invariance(kind):
    from switch_nerf_amd import ops
    st = _step(2)
    whole = ops.rng_fill(4096, 0, kind, SEED, st, 1)
    parts = torch.cat([ops.rng_fill(1001, 0, kind, SEED, st, 1), ops.rng_fill(3095, 1001, kind, SEED, st, 1)])
    assert torch.equal(whole, parts)
    # an unaligned destination (the plain-store path) holds the same values, and nothing is written outside [0, n)
    buf = torch.full((4096 + 8,), -7.0, device="cuda")
    ops.rng_fill(4096, 0, kind, SEED, st, 1, out=buf[3:3 + 4096])
    assert torch.equal(buf[3:3 + 4096], whole) and bool((buf[:3] == -7.0).all()) and bool((buf[3 + 4096:] == -7.0).all())


@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_normal_fill_matches_float64_restatement(scale):
    """Absolute tolerance 1e-5 * scale: |r| <= sqrt(48 ln 2) = 5.77; theta < 2 pi carries <= 4e-7 of fp32 rounding -> <= 2.4e-6 on the
    result; logf / sqrtf / sincosf add a few ulp of a value <= 5.77 (< 2e-6).  Measured maximum: profiles/r08_device_noise.md."""
    from switch_nerf_amd import ops
    n = 4099
    for base in (0, 5):
        out = ops.rng_fill(n, base, ops.RNG_NORMAL, SEED, _step(1), 3, scale=scale).cpu().numpy().astype(np.float64)
        ref = R.normal(SEED, 1, 3, base, n, scale=scale)
        err = np.abs(out - ref).max()
        print(f"normal fill: scale {scale} base {base} max abs err {err:.3e} (bound {1e-5 * scale:.1e})")
        assert err <= 1e-5 * scale, err


def test_normal_moments():
    """n = 2^20: every value finite, |mean| < 0.005 (5 sigma of the mean, sigma = 2^-10), |var - 1| < 0.007 (5 sigma, sigma = sqrt(2/n))."""
    from switch_nerf_amd import ops
    x = ops.rng_fill(1 << 20, 0, ops.RNG_NORMAL, SEED, _step(0), 1).double()
    assert bool(torch.isfinite(x).all())
    mean, var = x.mean().item(), x.var(unbiased=False).item()
    print(f"moments: mean {mean:.3e} var {var:.6f}")
    assert abs(mean) < 0.005 and abs(var - 1.0) < 0.007, (mean, var)


def test_step_lives_on_the_device():
    from switch_nerf_amd import ops
    n, stream = 515, 2
    st = _step(5)
    a = ops.rng_fill(n, 0, ops.RNG_UNIFORM, SEED, st, stream)
    ops.rng_advance(st)
    b = ops.rng_fill(n, 0, ops.RNG_UNIFORM, SEED, st, stream)
    assert np.array_equal(a.cpu().numpy(), R.uniform(SEED, 5, stream, 0, n))
    assert np.array_equal(b.cpu().numpy(), R.uniform(SEED, 6, stream, 0, n)) and int(st.item()) == 6
    # [fill; advance] captured once on one stream (no parallel branches): replay k draws at step k
    st.fill_(0)
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ops.rng_fill(n, 0, ops.RNG_UNIFORM, SEED, st, stream, out=out)
        ops.rng_advance(st)
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), R.uniform(SEED, k, stream, 0, n)), k
    assert int(st.item()) == 3


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("ray_base", [0, 5])
def test_sample_pe_rng_twin(ray_base, dtype):
    """The in-kernel jitter equals the fill (stream 0, base ray_base * S) followed by swn_sample_pe, bit for bit."""
    from switch_nerf_amd import _lib, ops
    _lib.use_half("bf16")
    N, S = 37, 13
    rays = _dev(synth.make_rays(77, N)[0])
    t = torch.linspace(0, 1, S, dtype=torch.float32).cuda()
    st = _step(3)
    u = ops.rng_fill(N * S, ray_base * S, ops.RNG_UNIFORM, SEED, st, ops.RNG_JITTER).view(N, S)
    z0, pe0, pd0 = ops.sample_pe(rays, t, u, 1.0, S, 12, 4, dtype, 128, 32)
    z1, pe1, pd1 = ops.sample_pe_rng(rays, t, SEED, st, ray_base, 1.0, S, 12, 4, dtype, 128, 32)
    assert torch.equal(z0, z1) and torch.equal(pe0, pe1) and torch.equal(pd0, pd1)
    zd, _, _ = ops.sample_pe(rays, t, None, 0.0, S, 12, 4, dtype, 128, 32)
    assert not torch.equal(zd, z1)                                   # (the jitter did move the samples)


# ---------------------------------------------------------------------------------------------------------------- model level
N_RAYS, S_SAMPLES, CHUNK, STD = 64, 16, 1024, 1.0


def _model(noise_seed=None, weights=41, dtype=torch.bfloat16, **kw):
    from switch_nerf_amd.model import SwitchNeRF
    m = SwitchNeRF(synth.BUILDING, dtype=dtype, **kw)
    m.load_state_dict(synth.make_weights(weights, synth.BUILDING))
    if noise_seed is not None:
        m.set_device_noise(noise_seed)
    return m


def _batches(n=3, rays=N_RAYS):
    return [tuple(_dev(a) for a in synth.make_rays(500 + i, rays)) for i in range(n)]


def _train(m, batches, **kw):
    out = []
    for rays, img, rgbs in batches:
        r = m.train_step(rgbs, rays, img, S_SAMPLES, CHUNK, perturb=1.0, sigma_noise_std=STD, **kw)
        out.append((r["loss"].item(), r["ctx"]["z"].clone()))
    return out


def test_same_seed_same_run():
    b = _batches()
    ma, mb, mc = _model(1234), _model(1234), _model(99)
    ra, rb, rc = _train(ma, b), _train(mb, b), _train(mc, b[:1])
    assert [l for l, _ in ra] == [l for l, _ in rb]
    assert torch.equal(ma.flat, mb.flat)
    assert ma.noise_state_dict() == dict(seed=1234, step=3, ray_base=0)
    assert not torch.equal(ra[0][1], rc[0][1])                       # another seed: another jitter


def test_graphed_step_equals_eager_with_noise_on():
    """GraphedTrainStep over 3 steps == 3 eager steps, bit for bit in loss and parameters, with jitter and sigma noise ON (device noise):
    with the framework generator this only held with supplied noise."""
    from switch_nerf_amd.graph import GraphedTrainStep
    b = _batches()
    ma, mb = _model(4321), _model(4321)
    rays0, img0, rgbs0 = b[0]
    step = GraphedTrainStep(ma, rgbs0, rays0, img0, S_SAMPLES, CHUNK, perturb=1.0, noise_std=STD)
    assert ma.noise_state_dict()["step"] == 0                        # the warm-up steps' advances were taken back
    ma.m.zero_(); ma.v.zero_(); ma.step_count = 0
    for rays, img, rgbs in b:
        ra = step(rgbs, rays, img)
        la = ra["loss"].item()
        rb = mb.train_step(rgbs, rays, img, S_SAMPLES, CHUNK, perturb=1.0, sigma_noise_std=STD)
        assert la == rb["loss"].item()
        assert torch.equal(ra["ctx"]["z"], rb["ctx"]["z"])
    assert torch.equal(ma.flat, mb.flat), (ma.flat - mb.flat).abs().max().item()
    assert ma.noise_state_dict()["step"] == mb.noise_state_dict()["step"] == 3


def test_reseed_behind_a_capture_fills_the_captured_counter():
    """set_device_noise after a GraphedTrainStep was captured (same seed and ray_base, step 5) must FILL the counter tensor the graph
    holds by address, never replace it: the replay then equals an eager step of a model seeded at step 5 bit for bit (rgb, loss, the
    flat gradient), and both counters read 6."""
    from switch_nerf_amd.graph import GraphedTrainStep
    rays, img, rgbs = _batches(1)[0]
    ma, mb = _model(4321), _model(None)
    step = GraphedTrainStep(ma, rgbs, rays, img, S_SAMPLES, CHUNK, perturb=1.0, noise_std=STD)
    for m in (ma, mb):
        m.set_device_noise(4321, step=5, ray_base=0)
    ra = step(rgbs, rays, img, optimizer_step=False)
    rb = mb.train_step(rgbs, rays, img, S_SAMPLES, CHUNK, perturb=1.0, sigma_noise_std=STD, optimizer_step=False)
    assert torch.equal(ra["rgb"], rb["rgb"]) and torch.equal(ra["loss"], rb["loss"]) and torch.equal(ma.grad, mb.grad)
    assert ma.noise_state_dict()["step"] == mb.noise_state_dict()["step"] == 6


def test_batch_split_invariance():
    """forward_rays on 2N rays draws, for ray i, what the two halves run with ray_base 0 and N draw (z and the sigma noise; rgb is not
    compared: routing is per chunk)."""
    m = _model(777)
    rays, img, _ = _batches(1, 2 * N_RAYS)[0]
    N = N_RAYS
    run = lambda r, i: m.forward_rays(r.contiguous(), i.contiguous(), S_SAMPLES, CHUNK, 1.0, None, None, True, sigma_noise_std=STD)
    c = run(rays, img)
    z, sn = c["z"].clone(), c["sigma_noise"].clone()
    halves = []
    for h in range(2):
        m.set_ray_base(h * N)
        ch = run(rays[h * N:(h + 1) * N], img[h * N:(h + 1) * N])
        halves.append((ch["z"].clone(), ch["sigma_noise"].clone()))
    assert torch.equal(z, torch.cat([halves[0][0], halves[1][0]]))
    assert torch.equal(sn, torch.cat([halves[0][1], halves[1][1]]))
    assert sn.std().item() > 0.5 and not torch.equal(halves[0][1], halves[1][1])


def test_resume_from_noise_state():
    b = _batches()
    m = _model(2024)
    _train(m, b[:2])
    saved = dict(noise=m.noise_state_dict(), flat=m.flat.clone(), m=m.m.clone(), v=m.v.clone(), step_count=m.step_count)
    assert saved["noise"]["step"] == 2
    loss_a = _train(m, b[2:])[0][0]
    m2 = _model(None, weights=7)
    m2.flat.copy_(saved["flat"]); m2.m.copy_(saved["m"]); m2.v.copy_(saved["v"]); m2.step_count = saved["step_count"]
    m2.refresh_compute_copies()
    m2.load_noise_state_dict(saved["noise"])
    loss_b = _train(m2, b[2:])[0][0]
    assert loss_a == loss_b and torch.equal(m.flat, m2.flat)


def test_supplied_noise_wins():
    rays, img, rgbs = _batches(1)[0]
    g = torch.Generator().manual_seed(5)
    pr = torch.rand(N_RAYS, S_SAMPLES, generator=g).cuda()
    sn = torch.randn(N_RAYS * S_SAMPLES, generator=g).cuda()
    on, off = _model(31), _model(None)
    ra = on.train_step(rgbs, rays, img, S_SAMPLES, CHUNK, perturb=1.0, perturb_rand=pr, sigma_noise=sn, sigma_noise_std=STD)
    rb = off.train_step(rgbs, rays, img, S_SAMPLES, CHUNK, perturb=1.0, perturb_rand=pr, sigma_noise=sn)
    assert torch.equal(ra["ctx"]["z"], rb["ctx"]["z"]) and torch.equal(ra["rgb"], rb["rgb"])
    assert ra["loss"].item() == rb["loss"].item() and torch.equal(on.flat, off.flat)


def test_background_model_is_refused():
    from switch_nerf_amd.dense import DenseNeRF
    from switch_nerf_amd.rendering import render_rays
    m = _model(None)
    bg = DenseNeRF(synth.DENSE_BG, dtype=torch.bfloat16)
    rays, img, _ = _batches(1)[0]
    hp = types.SimpleNamespace(coarse_samples=S_SAMPLES, fine_samples=0, model_chunk_size=CHUNK, perturb=1.0, use_sigma_noise=True,
                               sigma_noise_std=STD, device_noise_seed=5)
    with pytest.raises(NotImplementedError, match="device_noise_seed"):
        render_rays(m, bg, rays, img, hp, _dev(synth.SPHERE_CENTER), _dev(synth.SPHERE_RADIUS))


def test_render_rays_switches_device_noise_on():
    """hparams.device_noise_seed switches the model's device noise on once; hparams.ray_base is honoured; a training render advances
    the step and two models with the same seed render the same jittered, noised batch."""
    from switch_nerf_amd.rendering import render_rays
    rays, img, _ = _batches(1)[0]
    hp = types.SimpleNamespace(coarse_samples=S_SAMPLES, fine_samples=0, model_chunk_size=CHUNK, perturb=1.0, use_sigma_noise=True,
                               sigma_noise_std=STD, device_noise_seed=5, ray_base=128)
    outs = []
    for _ in range(2):
        m = _model(None)
        with torch.no_grad():
            res, _ = render_rays(m, None, rays, img, hp)
        assert m.noise_state_dict() == dict(seed=5, step=1, ray_base=128)
        outs.append(res["rgb_coarse"].clone())
    assert torch.equal(outs[0], outs[1])


def test_no_framework_draw_in_the_step():
    """With device noise on the step calls no torch.rand / randn: a differently seeded default CUDA generator changes nothing - with the
    hierarchical pass (fine u, fine sigma noise) and the gate noise on, so that every stream is drawn."""
    rays, img, rgbs = _batches(1)[0]
    res = []
    for gen_seed in (1, 2):
        m = _model(555, gate_noise=1.0)
        torch.cuda.manual_seed(gen_seed)
        r = m.train_step(rgbs, rays, img, S_SAMPLES, CHUNK, perturb=1.0, sigma_noise_std=STD, fine_samples=8)
        res.append((r["loss"].item(), r["rgb"].clone(), m.flat.clone()))
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])


def test_moe_layer_gate_noise_switch():
    """moe.MoELayer.set_device_noise: the layer's gate-noise draw comes from the seeded generator (stream 4, restated here), not from
    the framework generator."""
    from switch_nerf_amd import ops
    from switch_nerf_amd.moe import moe_layer
    cfg = synth.BUILDING
    P, E = 512, cfg["num_experts"]
    moe = moe_layer(gate_type=dict(type="top", k=1, fp32_gate=True, capacity_factor=1.0, batch_prioritized_routing=True, gate_noise=1.0,
                                   gate_dim=cfg["gate_hidden"]), model_dim=cfg["model_dim"],
                    experts=dict(type="expertmlp", count_per_node=E, hidden_size_per_expert=cfg["model_dim"],
                                 layer_num=cfg["expert_layers"], skips=list(cfg["skips"])), seeds=(1, 1, 1), return_gates=True,
                    dtype=torch.float32).cuda()
    moe.train()
    rng = np.random.default_rng(3)
    x = _dev(rng.standard_normal((P, 256)).astype(np.float32))
    gi = _dev(rng.standard_normal((P, 256)).astype(np.float32))
    moe.set_device_noise(99, step=4, row_base=10)
    torch.cuda.manual_seed(1)
    ya = moe(x, gate_input=gi)
    assert moe.noise_state_dict() == dict(seed=99, step=5, row_base=10)
    moe.set_device_noise(99, step=4, row_base=10)
    torch.cuda.manual_seed(2)
    yb = moe(x, gate_input=gi)
    draw = ops.rng_fill(P * E, 10 * E, ops.RNG_NORMAL, 99, ops.rng_step_tensor(4, "cuda"), ops.RNG_GATE).view(P, E)
    moe.set_device_noise(None)
    yc = moe(x, gate_input=gi, gate_noise_draw=draw)
    assert torch.equal(ya, yb) and torch.equal(ya, yc)
    assert torch.equal(ya.gate_extras["gates"], yc.gate_extras["gates"])


# ---------------------------------------------------------------------------------------------------------------- the other paths
def _hp(**kw):
    d = dict(coarse_samples=S_SAMPLES, fine_samples=0, model_chunk_size=CHUNK, perturb=1.0, use_sigma_noise=True, sigma_noise_std=STD,
             use_cascade=False, device_noise_seed=5)
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_render_rays_keeps_the_shards_ray_base():
    """parallel.shard_rays(..., model=m) sets the rank's first global ray; render_rays with hparams.device_noise_seed and NO
    hparams.ray_base keeps it, on the switch-on call and on every later one - rank 1's render of its half equals the second half of the
    one-GPU draw; an hparams.ray_base, when present, is honoured."""
    from switch_nerf_amd import parallel
    from switch_nerf_amd.rendering import render_rays
    rays, img, _ = _batches(1, 2 * N_RAYS)[0]
    whole = _model(None)
    with torch.no_grad():
        render_rays(whole, None, rays, img, _hp())
    z_whole = whole.forward_rays(rays, img, S_SAMPLES, CHUNK, 1.0, None, None, True)["z"]          # (step 1 now)
    m = _model(None)
    b, e = parallel.shard_rays(2 * N_RAYS, 1, 2, model=m)
    assert (b, e) == (N_RAYS, 2 * N_RAYS)
    with torch.no_grad():
        render_rays(m, None, rays[b:e].contiguous(), img[b:e].contiguous(), _hp())
        assert m.noise_state_dict() == dict(seed=5, step=1, ray_base=N_RAYS)
        z = m.forward_rays(rays[b:e].contiguous(), img[b:e].contiguous(), S_SAMPLES, CHUNK, 1.0, None, None, True)["z"]
        assert torch.equal(z, z_whole[b:e])
        render_rays(m, None, rays[b:e].contiguous(), img[b:e].contiguous(), _hp())
        assert m.noise_state_dict()["ray_base"] == N_RAYS
        render_rays(m, None, rays[b:e].contiguous(), img[b:e].contiguous(), _hp(ray_base=7))
        assert m.noise_state_dict()["ray_base"] == 7
    on = _model(11)                                                  # switched on by the caller: the shard helper moves it, too
    parallel.shard_rays(2 * N_RAYS, 1, 2, model=on)
    assert on.noise_state_dict()["ray_base"] == N_RAYS


def test_mip_step_draws_from_the_seeded_generator():
    """train_step_mip with device noise on (jitter through the fill, sigma noise per interval on streams 1 / 3, fine u on stream 2): the
    framework generator's seed changes nothing, the step counter advances, another noise seed gives other depths."""
    N, S, Fn = 32, 17, 17
    rays, img, rgbs = _batches(1, N)[0]
    radii = torch.full((N, 1), 1e-3, device="cuda")
    res = []
    for gen_seed, noise_seed in ((1, 21), (2, 21), (2, 22)):
        m = _model(noise_seed)
        torch.cuda.manual_seed(gen_seed)
        st = m.train_step_mip(rgbs, rays, radii, img, S, Fn, CHUNK, perturb=1.0, sigma_noise_std=STD)
        assert m.noise_state_dict()["step"] == 1
        assert st["ctx"]["sigma_noise"].numel() == N * (S - 1) and st["ctx_fine"]["sigma_noise"].numel() == N * (Fn - 1)
        res.append((st["loss"].item(), st["ctx"]["z_edges"].clone(), st["ctx_fine"]["z_edges"].clone(), m.flat.clone()))
    assert res[0][0] == res[1][0] and all(torch.equal(a, b) for a, b in zip(res[0][1:], res[1][1:]))
    assert not torch.equal(res[0][1], res[2][1]) and not torch.equal(res[0][2], res[2][2])


def test_hash_model_jitter_through_the_fill():
    """The hash-grid model samples with swn_sample_z: its jitter is stream 0 through the fill - the same depths the plain model draws
    in-kernel for the same (seed, step, rays)."""
    from switch_nerf_amd.model import SwitchNeRF
    hc = dict(n_levels=8, log2_table=12, base_res=4, per_level_scale=1.6, aabb_lo=(-1.2, -1.2, -1.2), aabb_hi=(1.2, 1.2, 1.2))
    rays, img, rgbs = _batches(1)[0]
    zs = []
    for gen_seed in (1, 2):
        m = SwitchNeRF(dict(synth.BUILDING, hash=hc), dtype=torch.float32, seed=3)
        m.set_device_noise(77)
        torch.cuda.manual_seed(gen_seed)
        st = m.train_step(rgbs, rays, img, S_SAMPLES, CHUNK, perturb=1.0, sigma_noise_std=STD)
        zs.append((st["ctx"]["z"].clone(), st["loss"].item(), m.flat.clone()))
    assert torch.equal(zs[0][0], zs[1][0]) and zs[0][1] == zs[1][1] and torch.equal(zs[0][2], zs[1][2])
    plain = _model(77, dtype=torch.float32)
    zp = plain.forward_rays(rays, img, S_SAMPLES, CHUNK, 1.0, None, None, True)["z"]
    assert torch.equal(zs[0][0], zp)


@pytest.mark.parametrize("fine", [0, 8])
def test_autograd_render_eager_and_graphed_agree_with_noise_on(fine):
    """render_rays under autograd (RenderRaysFunction) with device noise on, eager and with nerf.graph_train = True
    (graph.GraphedRenderTrain: draws and the counter's advance inside the forward graph): over 3 iterations both give the same
    rendering bit for bit (the parameters do not move: equal iff the noise is equal) and the same flat gradient, whatever the framework
    generator holds; the counter ends at 3 in both."""
    from switch_nerf_amd.rendering import render_rays
    batches = _batches(3)
    models = [_model(None), _model(None)]
    models[1].graph_train = True
    key = "rgb_fine" if fine else "rgb_coarse"
    out = [[], []]
    for i, m in enumerate(models):
        for it, (rays, img, rgbs) in enumerate(batches):
            torch.cuda.manual_seed(100 * i + it)
            res, _ = render_rays(m, None, rays, img, _hp(fine_samples=fine), None, None, True, True, False)
            assert res[key].requires_grad
            m.flat_param.grad = None
            (torch.nn.functional.mse_loss(res[key], rgbs) + m.wt * res["gate_loss_coarse"].mean()).backward()
            out[i].append((res[key].detach().clone(), m.flat_param.grad.clone()))
        assert m.noise_state_dict() == dict(seed=5, step=3, ray_base=0)
    for (rgb_a, g_a), (rgb_b, g_b) in zip(*out):
        assert torch.equal(rgb_a, rgb_b)                             # same parameters, same rays: equal iff the noise is equal
        err = (g_a - g_b).abs().max().item() / g_a.abs().max().item()
        print(f"eager vs graphed autograd gradient (fine={fine}): relative max difference {err:.2e}")
        assert err <= 2e-3, err          # (the bound tests/test_autograd_gpu.py gives the bf16 bridge: atomically accumulated weight gradients)
    assert not torch.equal(out[0][0][0], out[0][1][0])


def test_autograd_float_std_needs_device_noise():
    from switch_nerf_amd.autograd import RenderRaysFunction
    m = _model(None)
    rays, img, _ = _batches(1)[0]
    with pytest.raises(ValueError, match="device noise"):
        RenderRaysFunction.apply(m.flat_param, m, rays, img, S_SAMPLES, 0, CHUNK, 1.0, None, 1.0, None)
