"""Seeded device noise for Mega-NeRF joint training (switch_nerf_amd/mega.py: MegaNeRF.set_device_noise; graph.GraphedMegaStep) on the
fixture of tests/test_mega_train_gpu.py (tests/golden/mega_train.npz: 64 rays x 32 samples + 16 fine, three cells, margin 1).  Every
comparison is bit equality: a step that draws its noise runs the same packed rows through the same launches as a step that is handed the
same values from ops.rng_fill, eagerly and in a graph replay, in the compact and the padded form, before and after a resume."""
import numpy as np
import pytest
import torch

from test_mega_train_gpu import _dev, _load, _mega

pytestmark = pytest.mark.gpu
# The fixture's own rays fill (768, 384) to 764 and 380 rows, and the jitter moves a few points between the cells: the seed is one of
# those under which the drawn steps at STEP0 .. STEP0 + 2 stay inside that capacity (a batch that does not is refused by the step's tail
# with nothing touched: tests/test_mega_graph_gpu.py).
SEED, STEP0, BASE = 0x5EEDC0FFEE12345F, 5, 3
CAP = (768, 384)


def _batch(g, rays="rays"):
    return _dev(g["rgbs"]), _dev(g[rays]), _dev(g["image_indices"])


def _state(m):
    """Every parameter, moment and step count of the model, cloned."""
    return ([(s.flat.clone(), s.m.clone(), s.v.clone(), s.step_count) for s in m.sub_modules], m.step_count)


def _same_state(a, b):
    return a[1] == b[1] and all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and torch.equal(x[2], y[2]) and x[3] == y[3]
                                for x, y in zip(a[0], b[0]))


def _grads(m):
    return {k: v.clone() for k, v in m.grad_dict().items()}


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


def _noisy(g, margin=None, dtype=torch.float32, seed=SEED, step=STEP0, base=BASE):
    m = _mega(g, float(g["margin"]) if margin is None else margin, dtype)
    m.lr = m.base_lr = float(g["lr"])
    m.set_device_noise(seed, step, base)
    return m


def test_switch_and_state_dict():
    g = _load("mega_train")
    inf = _mega(g, 1.0, joint=False)
    with pytest.raises(NotImplementedError, match="joint_training=True"):
        inf.set_device_noise(3)
    m = _mega(g, float(g["margin"]))
    assert not m.device_noise and m.noise_state_dict() == {"seed": None, "step": 0, "ray_base": 0}
    m.set_device_noise(SEED, STEP0, BASE)
    assert m.device_noise and m.noise_state_dict() == {"seed": SEED, "step": STEP0, "ray_base": BASE}
    assert m.noise.step.is_cuda and not any(s.device_noise for s in m.sub_modules)
    m.train_step(*_batch(g), int(g["S"]), sigma_noise_std=1.0)
    assert m.noise_state_dict() == {"seed": SEED, "step": STEP0 + 1, "ray_base": BASE} and m.step_count == 1
    m.train_step(*_batch(g), int(g["S"]), optimizer_step=False, fine_samples=int(g["F"]), cell_capacity=(2048, 1024))
    assert m.noise_state_dict()["step"] == STEP0 + 2 and m.step_count == 1          # optimizer_step=False still advances the noise
    twin = _mega(g, float(g["margin"]))
    twin.load_noise_state_dict(m.noise_state_dict())
    assert twin.noise_state_dict() == m.noise_state_dict()
    counter = twin.noise.step
    twin.set_ray_base(128)
    twin.load_noise_state_dict({"seed": 9, "step": 2, "ray_base": 3})
    assert twin.noise.step is counter and twin.noise_state_dict() == {"seed": 9, "step": 2, "ray_base": 3}      # (the same counter tensor)
    for bad in (dict(seed=-1), dict(seed=1 << 64), dict(seed=1, step=1 << 32), dict(seed=1, ray_base=-1)):
        with pytest.raises(ValueError, match="device noise"):
            twin.set_device_noise(**bad)
    assert twin.noise_state_dict() == {"seed": 9, "step": 2, "ray_base": 3}
    # off: no launch differs - the counter stays where it is
    m.set_device_noise(None)
    step = m.noise.step.clone()
    m.train_step(*_batch(g), int(g["S"]), perturb=0.0, optimizer_step=False, sigma_noise_std=1.0)
    assert torch.equal(m.noise.step, step) and m.noise_state_dict()["seed"] is None


CASES = [("compact", None, None, torch.float32), ("padded", CAP, None, torch.float32), ("compact-soft", None, 1.15, torch.float32),
         ("padded-soft", (2048, 1024), 1.15, torch.float32), ("compact-bf16", None, None, torch.bfloat16),
         ("padded-bf16", CAP, None, torch.bfloat16)]


@pytest.mark.parametrize("F", [0, 16])
@pytest.mark.parametrize("name,cap,margin,dtype", CASES, ids=[c[0] for c in CASES])
def test_drawn_step_equals_the_step_supplied_the_same_draws(name, cap, margin, dtype, F):
    """A: noise on, sigma_noise_std 1, perturb 1.  B: a second identical model, noise off, handed perturb_rand / sigma_noise / fine_u /
    sigma_noise_fine from ops.rng_fill at the same (seed, step, ray_base, stream).  rgb, depth, loss and every cell's gradient bit for
    bit.  The fixture's margin is 1 (hard); the soft cases run at 1.15 with a capacity that holds every membership."""
    from switch_nerf_amd import ops
    g = _load("mega_train")
    N, S = int(g["N"]), int(g["S"])
    a = _noisy(g, margin, dtype)
    b = _mega(g, float(g["margin"]) if margin is None else margin, dtype)
    ra = a.grad_step(*_batch(g), S, perturb=1.0, fine_samples=F, cell_capacity=cap, sigma_noise_std=1.0)
    ga = _grads(a)
    step = ops.rng_step_tensor(STEP0, "cuda")
    fill = lambda stream_id, R, kind: ops.rng_fill(N * R, BASE * R, kind, SEED, step, stream_id, 1.0)
    kw = dict(perturb_rand=fill(ops.RNG_JITTER, S, ops.RNG_UNIFORM).view(N, S), sigma_noise=fill(ops.RNG_SIGMA, S, ops.RNG_NORMAL))
    if F:
        kw.update(fine_u=fill(ops.RNG_FINE_U, F, ops.RNG_UNIFORM).view(N, F), sigma_noise_fine=fill(ops.RNG_SIGMA_FINE, F, ops.RNG_NORMAL))
    outs = []
    for _ in range(2):              # (twice: what B reproduces of itself is what A must reproduce of B)
        rb = b.grad_step(*_batch(g), S, perturb=1.0, fine_samples=F, cell_capacity=cap, **kw)
        outs.append(({k: rb[k].clone() for k in ("rgb", "depth", "loss")}, _grads(b)))
    for k in ("rgb", "depth", "loss"):
        assert torch.equal(ra[k], outs[0][0][k]), k
    counts = lambda r: r["ctx"]["counts"].tolist() if torch.is_tensor(r["ctx"]["counts"]) else r["ctx"]["counts"]
    assert counts(ra) == counts(rb)
    if cap is not None:             # (a jittered batch may put more than C points into a cell: the same memberships are dropped in both)
        print(f"{name} F {F}: members {counts(ra)}, dropped {ra['cell_overflow'].tolist()}")
        assert ra["cell_overflow"].tolist() == rb["cell_overflow"].tolist()
    reproducible = _same(outs[0][1], outs[1][1])
    print(f"{name} F {F}: supplied-noise gradients reproduce themselves: {reproducible}")
    assert reproducible or dtype != torch.float32          # (fp32: tests/test_mega_train_gpu.py pins the determinism)
    if reproducible:
        for k in ga:
            assert torch.equal(ga[k], outs[0][1][k]), k
    assert any(v.any() for v in ga.values())
    # the draws are not the undrawn step's: perturb 1 with sigma noise differs from the deterministic pass
    rc = b.grad_step(*_batch(g), S, perturb=0.0, fine_samples=F, cell_capacity=cap)
    assert not torch.equal(rc["rgb"], ra["rgb"])
    assert b.noise_state_dict()["seed"] is None and a.noise_state_dict()["step"] == STEP0 + 1


def test_sh_cells_draw_in_the_compact_form():
    """sh_training cells use the same gather: the drawn step equals the step supplied the same draws (golden mega_sh_train.npz)."""
    from switch_nerf_amd import ops
    from test_mega_sh_train_gpu import _mega as _mega_sh
    g = _load("mega_sh_train")
    N, S = int(g["N"]), int(g["S"])
    a, b = _mega_sh(g, float(g["margin"])), _mega_sh(g, float(g["margin"]))
    a.set_device_noise(SEED, STEP0, BASE)
    args = (_dev(g["rgbs"]), _dev(g["rays"]), _dev(g["image_indices"]), S)
    ra = a.grad_step(*args, perturb=1.0, sigma_noise_std=0.5)
    ga = _grads(a)
    step = ops.rng_step_tensor(STEP0, "cuda")
    rb = b.grad_step(*args, perturb=1.0, perturb_rand=ops.rng_fill(N * S, BASE * S, ops.RNG_UNIFORM, SEED, step, ops.RNG_JITTER).view(N, S),
                     sigma_noise=ops.rng_fill(N * S, BASE * S, ops.RNG_NORMAL, SEED, step, ops.RNG_SIGMA, 0.5))
    for k in ("rgb", "depth", "loss"):
        assert torch.equal(ra[k], rb[k]), k
    gb = _grads(b)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k


def test_reproducible_and_resumable():
    g = _load("mega_train")
    S, F = int(g["S"]), int(g["F"])
    kw = dict(perturb=1.0, fine_samples=F, sigma_noise_std=1.0)

    def two_steps(seed):
        m = _noisy(g, seed=seed)
        rgb = [m.train_step(*_batch(g, rays), S, **kw)["rgb"].clone() for rays in ("rays", "rays_cell0")]
        return m, rgb

    (m1, rgb1), (m2, rgb2), (m3, rgb3) = two_steps(SEED), two_steps(SEED), two_steps(SEED + 1)
    assert _same_state(_state(m1), _state(m2)) and torch.equal(rgb1[0], rgb2[0]) and torch.equal(rgb1[1], rgb2[1])
    assert not torch.equal(rgb1[0], rgb3[0]) and not _same_state(_state(m1), _state(m3))
    assert m1.noise_state_dict() == {"seed": SEED, "step": STEP0 + 2, "ray_base": BASE}
    # one step, save, rebuild, second step: bit-equal to the uninterrupted run
    first = _noisy(g)
    first.train_step(*_batch(g), S, **kw)
    saved = (first.noise_state_dict(), _state(first))
    assert saved[0]["step"] == STEP0 + 1
    resumed = _mega(g, float(g["margin"]))
    resumed.lr = resumed.base_lr = float(g["lr"])
    for s, (flat, mom, var, count) in zip(resumed.sub_modules, saved[1][0]):
        s.flat.copy_(flat), s.m.copy_(mom), s.v.copy_(var)
        s.step_count = count
        s.refresh_compute_copies()
    resumed.step_count = saved[1][1]
    resumed.load_noise_state_dict(saved[0])
    rgb = resumed.train_step(*_batch(g, "rays_cell0"), S, **kw)["rgb"]
    assert torch.equal(rgb, rgb1[1]) and _same_state(_state(resumed), _state(m1))
    assert resumed.noise_state_dict() == m1.noise_state_dict()


def test_graphed_replays_equal_the_eager_padded_steps():
    """One capture at C = (2048, 1024) - rays_cell0 puts all 2048 coarse points into cell 0 - with 16 fine samples, replayed on rays, a
    permutation of rays and rays_cell0 with the optimizer on: results and end states bit for bit three eager padded train_steps of a twin
    with the same seed.  A second capture at (768, 384), the capacity the fixture's own rays fit, replays rays, the permutation and rays
    again on the initial parameters (optimizer_step=False: the fine pass's memberships then are those the seed was chosen for)."""
    from switch_nerf_amd.graph import GraphedMegaStep
    g = _load("mega_train")
    S, F = int(g["S"]), int(g["F"])
    perm = torch.randperm(int(g["N"]), generator=torch.Generator().manual_seed(3)).cuda()
    rgbs, rays, img = _batch(g)
    batches = {"rays": (rgbs, rays, img), "perm": (rgbs[perm].contiguous(), rays[perm].contiguous(), img[perm].contiguous()),
               "rays_cell0": _batch(g, "rays_cell0")}
    for cap, order, opt in (((2048, 1024), ("rays", "perm", "rays_cell0"), True), (CAP, ("rays", "perm", "rays"), False)):
        m, twin = _noisy(g), _noisy(g)
        step = GraphedMegaStep(m, *batches["rays"], S, cap, perturb=1.0, noise_std=1.0, fine_samples=F)
        assert m.noise_state_dict()["step"] == STEP0 and m.step_count == 0      # the counter is back behind warm-up and capture
        assert _same_state(_state(m), _state(twin))
        for i, name in enumerate(order):
            res = step(*batches[name], optimizer_step=opt)
            ref = twin.train_step(*batches[name], S, perturb=1.0, fine_samples=F, cell_capacity=cap, sigma_noise_std=1.0, optimizer_step=opt)
            for k in ("loss", "rgb", "depth"):
                assert torch.equal(res[k], ref[k]), (cap, name, k)
            assert res["ctx"]["counts"].tolist() == ref["ctx"]["counts"].tolist() and res["cell_overflow"].tolist() == [0, 0]
            gm, gt = m.grad_dict(), twin.grad_dict()
            for k in gm:
                assert torch.equal(gm[k], gt[k]), (cap, name, k)
            assert _same_state(_state(m), _state(twin)), (cap, name)
            assert m.noise_state_dict()["step"] == twin.noise_state_dict()["step"] == STEP0 + i + 1
        assert step.captures == 1 and m.step_count == twin.step_count == (3 if opt else 0)
    # a replay is a function of the counter, not of the warm-up: the same step again after putting the counter back
    m.set_device_noise(SEED, STEP0, BASE)
    again = step(*batches["rays"], optimizer_step=False)["rgb"].clone()
    m.set_device_noise(SEED, STEP0, BASE)
    assert torch.equal(step(*batches["rays"], optimizer_step=False)["rgb"], again)


def test_refusals_leave_the_counter_alone():
    from argparse import Namespace
    from switch_nerf_amd import mega
    from switch_nerf_amd.graph import GraphedMegaStep
    from test_mega_sh_train_gpu import _mega as _mega_sh
    g = _load("mega_train")
    S = int(g["S"])
    m = _noisy(g)
    with pytest.raises(NotImplementedError, match="accumulation"):
        m.set_accumulation(2)
    with pytest.raises(NotImplementedError, match="finite guard"):
        m.set_check_finite(True)
    with pytest.raises(NotImplementedError, match="data parallelism"):
        m.apply_step(lambda flat: 1.0)
    with pytest.raises(ValueError, match="exclude each other"):
        m.forward_points(torch.zeros(4, 7, device="cuda"), torch.zeros(4, device="cuda"), sigma_rng=(1, 2, 1.0))
    with pytest.raises(ValueError, match="cell_capacity is required"):
        GraphedMegaStep(m, *_batch(g), S, None)
    m.eval()
    h = Namespace(coarse_samples=S, fine_samples=0, model_chunk_size=1000, device_noise_seed=3)
    with pytest.raises(NotImplementedError, match="device_noise_seed"):
        mega.render_rays(m, None, _dev(g["rays"]), _dev(g["image_indices"]), h)
    m.train()
    assert m.noise_state_dict() == {"seed": SEED, "step": STEP0, "ray_base": BASE}
    gs = _load("mega_sh_train")
    sh = _mega_sh(gs, float(gs["margin"]))
    sh.set_device_noise(SEED, STEP0, BASE)
    args = (_dev(gs["rgbs"]), _dev(gs["rays"]), _dev(gs["image_indices"]), int(gs["S"]))
    with pytest.raises(NotImplementedError, match="cell_capacity.*spherical-harmonics"):
        sh.train_step(*args, cell_capacity=CAP, sigma_noise_std=1.0)
    with pytest.raises(NotImplementedError, match="cell_capacity.*spherical-harmonics"):
        GraphedMegaStep(sh, *args, CAP)
    assert sh.noise_state_dict()["step"] == STEP0      # (fp16 cells and xyz_real are refused at construction: tests/test_mega_device_noise_cpu.py)
