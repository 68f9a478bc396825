"""The finite guard at the level of the training step (set_check_finite; the reference's check_finite, runner.py:620-673): a step on a
poisoned batch - a NaN target pixel, an infinite far bound - is dropped on the device and the model then trains exactly like a twin
that never saw the batch; for every model kind, with accumulation, the fp16 loss scaler, the captured step and RCCL underneath."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, S = 64, 8
CHUNK = N * S
NAN, INF = float("nan"), float("inf")
DTYPES = [torch.float32, torch.bfloat16]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _moe(dtype, seed=41):
    from switch_nerf_amd.model import SwitchNeRF
    m = SwitchNeRF(synth.BUILDING, dtype=dtype)
    m.load_state_dict(synth.make_weights(seed, synth.BUILDING))
    return m


def _dense(dtype, seed=161):
    from switch_nerf_amd.dense import DenseNeRF
    m = DenseNeRF(synth.DENSE, dtype=dtype)
    m.load_state_dict(synth.make_dense_weights(seed, synth.DENSE))
    return m


def _batch(seed):
    return tuple(_dev(a) for a in synth.make_rays(seed, N))          # rays, image indices, targets


def _poisoned(batch, how):
    rays, img, rgbs = (t.clone() for t in batch)
    if how == "nan_target":
        rgbs[17, 1] = NAN                                            # one target pixel
    else:
        rays[17, 7] = INF                                            # one ray's far bound
    return rays, img, rgbs


def _step(m, batch, **kw):
    rays, img, rgbs = batch
    return m.train_step(rgbs, rays, img, S, CHUNK, perturb=0.0, **kw)


def _models(owner):
    if hasattr(owner, "halves"):
        return owner.halves()
    return [owner.nerf, owner.bg] if hasattr(owner, "bg") else [owner]


def _assert_twins(a, b, what=""):
    """Parameters, both moments and the step count of every model, bit for bit."""
    for ma, mb in zip(_models(a), _models(b)):
        for k in ("flat", "m", "v"):
            assert torch.equal(getattr(ma, k).view(torch.int32), getattr(mb, k).view(torch.int32)), (what, k)
        assert ma.step_count == mb.step_count, what
        assert bool(torch.isfinite(ma.flat).all()), what


def _poison_then_clean(a, b, step, poison, clean):
    """a (guard on): the poisoned batch, then the clean one; b (the twin, no guard): the clean one only."""
    a.set_check_finite(True)
    r0 = step(a, poison)
    assert int(r0["step_ok"].item()) == 0 and a.skipped_steps() == 1
    assert all(m.step_count == 0 for m in _models(a))
    r1 = step(a, clean)
    rb = step(b, clean)
    assert int(r1["step_ok"].item()) == 1 and a.skipped_steps() == 1 and "step_ok" not in rb and b.skipped_steps() == 0
    assert r1["loss"].item() == rb["loss"].item()
    _assert_twins(a, b)
    assert all(m.step_count == 1 for m in _models(a))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("how", ["nan_target", "inf_far"])
def test_twin_poisoned_step_is_dropped(dtype, how):
    """Without the guard the poisoned step turns every parameter into NaN (checked on a third model: the poison is real)."""
    clean = _batch(900)
    poison = _poisoned(_batch(901), how)
    _poison_then_clean(_moe(dtype), _moe(dtype), _step, poison, clean)
    c = _moe(dtype)
    _step(c, poison)
    assert not bool(torch.isfinite(c.flat).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_perfect_reproduction_is_a_step(dtype):
    m = _moe(dtype)
    m.set_check_finite(True)
    rays, img, _ = _batch(902)
    rgb = m.train_step(torch.zeros(N, 3, device="cuda"), rays, img, S, CHUNK, perturb=0.0, optimizer_step=False)["rgb"].clone()
    before = m.flat.clone()
    r = m.train_step(rgb, rays, img, S, CHUNK, perturb=0.0)
    assert r["photo_loss"].item() == 0.0 and r["psnr"].item() == INF
    assert int(r["step_ok"].item()) == 1 and m.skipped_steps() == 0 and m.step_count == 1
    assert bool(torch.isfinite(m.flat).all())
    moved = not torch.equal(m.flat, before)
    assert moved == bool(m.grad.any())               # by the gate-loss gradient, or not at all


@pytest.mark.parametrize("dtype", DTYPES)
def test_guard_on_clean_batches_equals_guard_off(dtype):
    a, b = _moe(dtype), _moe(dtype)
    a.set_check_finite(True)
    for i in range(3):
        ra, rb = _step(a, _batch(910 + i)), _step(b, _batch(910 + i))
        assert int(ra["step_ok"].item()) == 1 and ra["loss"].item() == rb["loss"].item()
        _assert_twins(a, b, i)
        for k in a.wf:
            assert torch.equal(a.wf[k].view(torch.uint8), b.wf[k].view(torch.uint8)), k      # the compute copies
    assert a.step_count == 3 and a.skipped_steps() == 0
    a.set_check_finite(False)                        # the count returns to the host
    assert a.step_count == 3 and "step_ok" not in _step(a, _batch(913)) and a.step_count == 4


@pytest.mark.parametrize("dtype", DTYPES)
def test_dense_nerf(dtype):
    _poison_then_clean(_dense(dtype), _dense(dtype), _step, _poisoned(_batch(921), "nan_target"), _batch(920))


def test_cascade_poison_in_the_coarse_loss_only():
    """A NaN in the coarse pass's sigma noise at a ray's LAST sample: that ray's coarse colour is NaN, its resampled depths are not
    (the resampling leaves out the first and the last weight), so the fine loss is finite and only the coarse loss carries the poison.
    One flag drops the step of both halves."""
    from switch_nerf_amd.cascade import Cascade
    mk = lambda: Cascade(_dense(torch.float32, 171), _dense(torch.float32, 172))
    fu = torch.rand(N, 8, generator=torch.Generator().manual_seed(3)).cuda()
    noise = torch.zeros(N * S, device="cuda")
    bad = noise.clone()
    bad[17 * S + S - 1] = NAN
    seen = []

    def step(m, batch):
        rays, img, rgbs = batch
        r = m.train_step(rgbs, rays, img, S, CHUNK, perturb=0.0, fine_samples=8, fine_u=fu, sigma_noise=bad if batch is poison else noise,
                         sigma_noise_fine=torch.zeros(N * (S + 8), device="cuda"))
        seen.append((r["coarse_loss"].item(), r["photo_loss"].item()))
        return r
    poison, clean = _batch(931), _batch(930)
    _poison_then_clean(mk(), mk(), step, poison, clean)
    coarse, fine = seen[0]
    assert not np.isfinite(coarse) and np.isfinite(fine), seen[0]


def test_background_scene_poison_in_a_background_ray():
    from switch_nerf_amd.background import BackgroundScene
    from switch_nerf_amd.dense import DenseNeRF
    from switch_nerf_amd.model import SwitchNeRF
    mk = lambda: BackgroundScene(SwitchNeRF(synth.BUILDING, dtype=torch.float32, seed=5), DenseNeRF(synth.DENSE_BG, dtype=torch.float32, seed=6),
                                 synth.SPHERE_CENTER, synth.SPHERE_RADIUS)
    def bg_batch(seed, poison):
        rays, img, rgbs = synth.make_bg_rays(seed, N)
        k = int(np.argmax(rays[:, 7]))               # the ray that reaches farthest: it leaves the bound (far > 1.4, the bound ends by 0.9)
        assert rays[k, 7] > 1.4
        if poison:
            rgbs[k, 2] = NAN
        return _dev(rays), _dev(img), _dev(rgbs)
    step = lambda m, b: m.train_step(b[2], b[0], b[1], S, CHUNK, perturb=0.0)
    a, b = mk(), mk()
    _poison_then_clean(a, b, step, bg_batch(941, True), bg_batch(940, False))
    assert a.bg.step_count == 1                      # the clean batch had background rays: both models stepped, on one flag
    with pytest.raises(NotImplementedError, match="check_finite"):
        bb = bg_batch(940, False)
        a.train_step(bb[2], bb[0], bb[1], S, CHUNK, perturb=0.0, bg_capacity=N)
    from switch_nerf_amd.graph import GraphedBackgroundStep
    with pytest.raises(NotImplementedError, match="check_finite"):
        GraphedBackgroundStep(a, bb[2], bb[0], bb[1], S, CHUNK, perturb=0.0, noise_std=0.0)


def test_accumulation_flagged_micro_step_clears_the_window():
    """A = 2, micro-steps (poison, clean1, clean2, clean3).  The rule: a flagged micro-step contributes nothing and clears the buffer;
    it does not change which call is the A-th.  So call 2 is a last micro-step and steps on 0 + g(clean1) / 2, and calls 3 and 4 are an
    ordinary window: Adam on g(clean2) / 2 + g(clean3) / 2.  The twin is told exactly that: clean1 with should_accumulate=False on its
    zero buffer, then clean2 (accumulate) and clean3 (step)."""
    a, b = _moe(torch.float32), _moe(torch.float32)
    for m in (a, b):
        m.set_accumulation(2)
    a.set_check_finite(True)
    clean = [_batch(950 + i) for i in range(3)]
    flags, stepped = [], []
    for batch in [_poisoned(_batch(959), "nan_target")] + clean:
        r = _step(a, batch)
        flags.append(int(r["step_ok"].item()))       # (the flag is ONE device tensor: read before the next step overwrites it)
        stepped.append(r["optimizer_stepped"])
    assert flags == [0, 1, 1, 1]
    assert stepped == [False, True, False, True]     # (the launches issued: the window rule)
    for c, acc in zip(clean, (False, True, False)):
        _step(b, c, should_accumulate=acc)
    _assert_twins(a, b)
    assert a.step_count == 2 and a.skipped_steps() == 1 and not bool(a.accum.any())
    # a flagged LAST micro-step: the window's partial sum is discarded with it
    before = a.flat.clone()
    _step(a, clean[0])
    assert bool(a.accum.any())
    r = _step(a, _poisoned(_batch(959), "inf_far"))
    assert int(r["step_ok"].item()) == 0 and not bool(a.accum.any()) and torch.equal(a.flat, before) and a.step_count == 2


def test_fp16_guard_sits_in_front_of_the_loss_scaler():
    from switch_nerf_amd import _lib
    try:
        m = _moe(torch.float16)
        m.set_check_finite(True)
        sc = m.loss_scaler
        state0 = dict(sc.state_dict())
        before = m.flat.clone()
        r = _step(m, _poisoned(_batch(961), "nan_target"))
        assert int(r["step_ok"].item()) == 0 and m.skipped_steps() == 1
        assert sc.state_dict() == state0 and sc.skipped == 0         # scale and growth tracker: the scaler's update never ran
        assert torch.equal(m.flat, before) and m.step_count == 0
        r = _step(m, _batch(960))
        assert int(r["step_ok"].item()) == 1 and m.step_count == 1 and sc.state_dict()["_growth_tracker"] == state0["_growth_tracker"] + 1
        assert bool(torch.isfinite(m.flat).all()) and not torch.equal(m.flat, before)
    finally:
        _lib.use_half("bf16")


@pytest.mark.parametrize("dtype", DTYPES)
def test_graphed_step_one_capture_skips_and_steps(dtype):
    from switch_nerf_amd.graph import GraphedTrainStep
    a, b = _moe(dtype), _moe(dtype)
    for m in (a, b):
        m.set_check_finite(True)
    clean = [_batch(970), _batch(971)]
    poison = [_poisoned(_batch(972), "nan_target"), _poisoned(_batch(973), "inf_far")]
    rays, img, rgbs = poison[0]                      # captured on a bad batch: the warm-up is not counted as skipped steps
    step = GraphedTrainStep(a, rgbs, rays, img, S, CHUNK, perturb=0.0, noise_std=0.0)
    assert a.skipped_steps() == 0 and step.captures == 1
    graph = step.graph
    for i, (batch, want) in enumerate(((poison[0], 0), (clean[0], 1), (poison[1], 0), (clean[1], 1))):
        rays, img, rgbs = batch
        ra = step(rgbs, rays, img)
        rb = _step(b, batch)
        assert int(ra["step_ok"].item()) == int(rb["step_ok"].item()) == want, i
        _assert_twins(a, b, i)
    assert a.step_count == 2 and a.skipped_steps() == b.skipped_steps() == 2
    assert step.captures == 1 and step.graph is graph


def test_graphed_split_backward_reduces_the_flag_over_ranks(monkeypatch):
    """GraphedTrainStep with the backward cut in two hands apply_step a closure in place of the all-reduce object; the flag's MIN over
    the ranks must still be issued (once per step, on the model's flag, between the early part and the rest of the gradient) and decide
    the step: here the stand-in for the other rank reports a bad batch on the second step, and this rank drops its clean step."""
    from switch_nerf_amd import optim
    from switch_nerf_amd.graph import GraphedTrainStep
    calls = []

    class TwoRanks:
        other_ok = 1

        def __call__(self, view):
            calls.append("all")
            return 1.0

        def begin(self, part, stream=None):
            calls.append("begin")

        def finish(self, rest):
            calls.append("finish")
            return 1.0

        def all_ranks_ok(self, flag):
            calls.append(("flag", flag.data_ptr()))
            flag.clamp_(max=self.other_ok)           # MIN with the other rank's flag
            return flag

    monkeypatch.setattr(optim, "distributed", lambda: True)       # (the tail counts skipped steps, behind the reduction)
    m = _moe(torch.bfloat16)
    m.set_check_finite(True)
    rays, img, rgbs = _batch(975)
    step = GraphedTrainStep(m, rgbs, rays, img, S, CHUNK, perturb=0.0, noise_std=0.0, split_backward=True)
    assert step.graph_b is not None
    ar = TwoRanks()
    before = m.flat.clone()
    r = step(rgbs, rays, img, grad_allreduce=ar)
    assert calls == ["begin", ("flag", m._guard["ok"].data_ptr()), "finish"]
    assert int(r["step_ok"].item()) == 1 and m.step_count == 1 and m.skipped_steps() == 0 and not torch.equal(m.flat, before)
    ar.other_ok, before = 0, m.flat.clone()
    r = step(rgbs, rays, img, grad_allreduce=ar)
    assert calls[3:] == ["begin", ("flag", m._guard["ok"].data_ptr()), "finish"]
    assert int(r["step_ok"].item()) == 0 and m.step_count == 1 and m.skipped_steps() == 1 and torch.equal(m.flat, before)


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_rccl_world1_loopback_equals_single_process():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "SWN_DIST_BACKEND", "SWN_FORCE_DEVICE")}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "finite_guard_rccl_worker.py")], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-2500:], out.stderr[-2500:])
    assert "FINITE_GUARD_RCCL: OK" in out.stdout
