"""CPU-only side of the finite guard (set_check_finite): the reduction rule over ranks, the refusals, the round trip of the counters,
and the argument checks of the new entry points (they run before any launch)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import synth

SMALL = dict(layer_dim=64, layers=2, skip_layers=(1,), pos_xyz_dim=3, pos_dir_dim=2, appearance_dim=8, appearance_count=10, xyz_dim=3)


def _dense(cfg=SMALL, seed=0):
    from switch_nerf_amd.dense import DenseNeRF
    return DenseNeRF(cfg, dtype=torch.float32, device="cpu", seed=seed)


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_min_over_ranks_is_all_ranks_ok(world):
    """The reference sums the per-rank flags and compares with world_size (runner.py:660-666); the step here takes their MIN."""
    from switch_nerf_amd.parallel import combine_ok
    cases = itertools.product((0, 1), repeat=world) if world <= 3 else [(1,) * 8, (0,) * 8, (1,) * 7 + (0,), (0,) + (1,) * 7]
    for flags in cases:
        t = torch.tensor(flags, dtype=torch.int32)
        assert int(combine_ok(t)) == int(all(flags)) == int(int(t.sum()) == world)


def test_switch_state_round_trip_and_step_count():
    m = _dense()
    assert m.check_finite is False and m.skipped_steps() == 0
    m.step_count = 7
    m.set_check_finite(True)
    assert m.check_finite and m.step_count == 7 and m._guard["step"].tolist() == [7, 0] and m._guard["ok"].dtype == torch.int32
    m._guard["skipped"].fill_(3)
    m.step_count = 9
    sd = m.finite_guard_state_dict()
    assert sd == dict(check_finite=True, skipped_steps=3, step_count=9)
    r = _dense()
    r.load_finite_guard_state_dict(sd)
    assert r.check_finite and r.skipped_steps() == 3 and r.step_count == 9 and r._guard["step"].tolist() == [9, 0]
    r.set_check_finite(False)                        # off: the count returns to the host, the counter is gone
    assert r.step_count == 9 and r._guard is None and r.skipped_steps() == 0
    # Adam's checkpoint state reads the same count
    from switch_nerf_amd import checkpoint
    assert float(checkpoint.adam_state_dict(m)["state"][0]["step"]) == 9.0
    checkpoint.load_adam_state_dict(m, {"state": {}, "param_groups": []})
    assert m.step_count == 0 and m._guard["step"].tolist() == [0, 0]


def test_owners_share_one_flag_and_round_trip():
    from switch_nerf_amd.background import BackgroundScene
    from switch_nerf_amd.cascade import Cascade
    c = Cascade(_dense(seed=0), _dense(seed=1))
    s = BackgroundScene(_dense(), _dense(dict(SMALL, xyz_dim=4)), synth.SPHERE_CENTER, synth.SPHERE_RADIUS)
    for owner, (x, y) in ((c, (c.coarse, c.fine)), (s, (s.nerf, s.bg))):
        owner.set_check_finite(True)
        assert owner.check_finite and x._guard["ok"] is y._guard["ok"] and x._guard["skipped"] is y._guard["skipped"]
        assert x._guard["step"] is not y._guard["step"]
        x.step_count, y.step_count = 4, 2
        x._guard["skipped"].fill_(5)
        sd = owner.finite_guard_state_dict()
        owner.set_check_finite(False)
        assert not owner.check_finite and owner.skipped_steps() == 0 and (x.step_count, y.step_count) == (4, 2)
        x.step_count = y.step_count = 0
        owner.load_finite_guard_state_dict(sd)
        assert owner.skipped_steps() == 5 and (x.step_count, y.step_count) == (4, 2) and x._guard["ok"] is y._guard["ok"]


def test_refusals_name_check_finite():
    from switch_nerf_amd import optim
    from switch_nerf_amd.background import BackgroundScene
    from switch_nerf_amd.mega import MegaNeRF
    from switch_nerf_amd.model import SwitchNeRF
    from switch_nerf_amd.parallel import ExpertParallel
    # expert parallelism with the tail on the experts' ranks, in either order
    m = SwitchNeRF(synth.BUILDING, dtype=torch.float32, device="cpu")
    m.set_check_finite(True)
    with pytest.raises(NotImplementedError, match="check_finite.*owner_tail"):
        m.set_expert_parallel(ExpertParallel(0, 1, m.E, owner_tail=True))
    m2 = SwitchNeRF(synth.BUILDING, dtype=torch.float32, device="cpu")
    m2.set_expert_parallel(ExpertParallel(0, 1, m2.E, owner_tail=True))
    with pytest.raises(NotImplementedError, match="check_finite.*owner_tail"):
        m2.set_check_finite(True)
    m2.set_check_finite(False)
    # the mip step
    with pytest.raises(NotImplementedError, match="check_finite"):
        m.train_step_mip(None, None, None, None, 8, 8, 64)
    # Mega-NeRF joint training: the switch, and a cell switched on by hand
    cells = [_dense(seed=i) for i in range(2)]
    mega = MegaNeRF(cells, np.array([[-0.05, 0.0, 0.0], [0.05, 0.0, 0.0]], np.float32), 1.0, False, False, joint_training=True)
    with pytest.raises(NotImplementedError, match="check_finite"):
        mega.set_check_finite(True)
    mega.set_check_finite(False)
    cells[0].set_check_finite(True)
    with pytest.raises(NotImplementedError, match="check_finite"):
        mega.apply_step()
    # the padded background step
    s = BackgroundScene(_dense(), _dense(dict(SMALL, xyz_dim=4)), synth.SPHERE_CENTER, synth.SPHERE_RADIUS)
    s.set_check_finite(True)
    with pytest.raises(NotImplementedError, match="check_finite"):
        s.train_step(None, None, None, 8, 64, bg_capacity=4)
    with pytest.raises(NotImplementedError, match="check_finite"):
        s.apply_step(dict(ctx=dict(Nb=1, C=4, N=8, n_out=0)))
    # a group whose models do not share one flag
    x, y = _dense(seed=0), _dense(seed=1)
    x.set_check_finite(True)
    with pytest.raises(ValueError, match="check_finite"):
        optim.apply_tail([x, y])
    y.set_check_finite(True)
    with pytest.raises(ValueError, match="check_finite"):
        optim.apply_tail([x, y])


def test_entry_points_validate_before_launch():
    from switch_nerf_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(0x1000)                           # any aligned non-null address: validation only
    odd = C.c_void_p(0x1002)
    err = lambda: lib.swn_last_error().decode()
    assert lib.swn_finite_guard(None, 4, 3, p, p, None) != 0 and "null pointer" in err()
    assert lib.swn_finite_guard(p, 0, -1, p, p, None) != 0 and "1 to 64" in err()
    assert lib.swn_finite_guard(p, 4, 4, p, p, None) != 0 and "psnr slot" in err()
    assert lib.swn_finite_guard(p, 4, 3, odd, p, None) != 0 and "misaligned" in err()
    adam = [p, p, p, p, None, _lib.F32, 100, 1e-3, 0.9, 0.999, 1e-8]
    assert lib.swn_adam_step_guarded(*adam, p, 10, p, 1.0, None, None) != 0 and "flag are required" in err()
    assert lib.swn_adam_step_guarded(*adam, None, 10, p, 1.0, p, None) != 0 and "flag are required" in err()
    assert lib.swn_adam_step_guarded(*adam, p, 0, p, 1.0, p, None) != 0 and "flag are required" in err()
    assert lib.swn_adam_step_guarded(*adam, p, 10, odd, 1.0, p, None) != 0 and "misaligned" in err()
    adam[6] = 0
    assert lib.swn_adam_step_guarded(*adam, p, 10, p, 1.0, p, None) != 0 and "bad arguments" in err()
    assert lib.swn_grad_accum_guarded(p, p, 100, 0.5, None, None) != 0 and "bad arguments" in err()
    assert lib.swn_grad_accum_guarded(p, odd, 100, 0.5, p, None) != 0 and "aligned" in err()
    acc = [p, p, p, p, p, None, _lib.F32, 100, 1e-3, 0.9, 0.999, 1e-8]
    assert lib.swn_adam_accum_step_guarded(*acc, p, 10, None, 0.5, 1.0, p, None) != 0 and "flag are required" in err()
    assert lib.swn_adam_accum_step_guarded(*acc, p, 10, p, 0.5, 1.0, odd, None) != 0 and "misaligned" in err()
    acc[1] = None
    assert lib.swn_adam_accum_step_guarded(*acc, p, 10, p, 0.5, 1.0, p, None) != 0 and "bad arguments" in err()
    # the bias table (host only): the expressions of the unguarded entry point, the end row, the refusals
    tab = (C.c_float * (2 * 20000))()
    rows = C.c_long(0)
    assert lib.swn_adam_bias_table(0.9, 0.999, tab, 20000, C.byref(rows)) == 0 and 17000 < rows.value < 18000
    assert (tab[2 * rows.value - 2], tab[2 * rows.value - 1]) == (1.0, 1.0)
    assert (tab[2 * rows.value - 4], tab[2 * rows.value - 3]) != (1.0, 1.0)
    assert abs(tab[0] - 0.1) < 1e-7 and abs(tab[1] - np.sqrt(np.float32(1.0) - np.float32(0.999))) < 1e-7
    assert lib.swn_adam_bias_table(0.9, 0.999, tab, 100, C.byref(rows)) != 0 and "larger table" in err()
    assert lib.swn_adam_bias_table(0.9, 1.0, tab, 100, C.byref(rows)) != 0 and "betas" in err()


def test_tail_combines_the_flag_over_ranks_or_raises(monkeypatch):
    """In a torch.distributed run the tail reduces the flag with what it is given - the all-reduce object's all_ranks_ok, or an explicit
    flag_allreduce where the caller wrapped the all-reduce in a closure (the graphed split backward) - counts the skipped step behind
    the reduction, and raises on several ranks with neither."""
    import torch.distributed as dist
    from switch_nerf_amd import optim
    m = _dense()
    m.set_check_finite(True)
    ok = m._guard["ok"]
    seen = []

    class AllReduce:
        def __call__(self, view):
            return 1.0

        def all_ranks_ok(self, flag):
            seen.append(("object", flag))
            flag.zero_()                             # another rank's batch was bad

    monkeypatch.setattr(optim, "distributed", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    assert optim._guard_flag([m], AllReduce()) is ok and seen == [("object", ok)] and int(ok) == 0 and m.skipped_steps() == 1
    ok.fill_(1)
    closure = lambda view: 1.0                       # what GraphedTrainStep's split backward passes on: no all_ranks_ok on it
    assert optim._guard_flag([m], closure, lambda flag: seen.append(("explicit", flag))) is ok
    assert seen[-1] == ("explicit", ok) and m.skipped_steps() == 1
    for ar in (closure, None):
        with pytest.raises(RuntimeError, match="check_finite"):
            optim._guard_flag([m], ar)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 1)          # one rank: nothing to combine
    assert optim._guard_flag([m], None) is ok and m.skipped_steps() == 1
