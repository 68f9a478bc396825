"""CPU-only: the host state of the training step's tail (SwitchNeRF.apply_step; optim.apply_tail behind Cascade / BackgroundScene /
MegaNeRF.apply_step) that a launch trace cannot see - return values, step counts, window indices, the loss scaler, the recorded scale, which
buffers are left cleared - and the order of the optimizer launches, on host-resident fp32 models with the three library calls and
refresh_compute_copies replaced by recorders.  A loss scaler is attached by hand (fp32 models have none).

EXPECTED holds literal values, written down from a run of this file on the commit BEFORE the tail was factored into optim.py (every
owner with hand-written copies); they are not to be regenerated from the code under test.

One record per case: ret = what each apply_step call returned (a scene: its result keys without "ctx"); step / micro / applied / zero =
per model step_count, _micro, _applied_loss_scale, "accum is all zero" (None: no buffer); scale / skipped = the group's LossScaler;
calls = the launches in order - allreduce(buffer), accum(model, scale), adam(model, step, grad_scale),
adam_accum(model, +g = the gradient was passed, step, accum_scale, grad_scale), refresh(model) or refresh(*) for the replacement."""
import numpy as np
import pytest
import torch

import synth

SMALL = dict(layer_dim=64, layers=2, skip_layers=(1,), pos_xyz_dim=3, pos_dir_dim=2, appearance_dim=8, appearance_count=10, xyz_dim=3)
INF = float("inf")


def _build(group, kind, scaler):
    from switch_nerf_amd.background import BackgroundScene
    from switch_nerf_amd.cascade import Cascade
    from switch_nerf_amd.dense import DenseNeRF
    from switch_nerf_amd.mega import MegaNeRF
    from switch_nerf_amd.model import LossScaler, SwitchNeRF

    def dense(cfg=SMALL, seed=0):
        return DenseNeRF(cfg, dtype=torch.float32, device="cpu", seed=seed)
    if group == "model":
        models = [dense() if kind == "dense" else SwitchNeRF(synth.BUILDING, dtype=torch.float32, device="cpu")]
    elif group == "scene":
        models = [dense(), dense(dict(SMALL, xyz_dim=4))]
    else:
        models = [dense(seed=i) for i in range(2 if group == "cascade" else 3)]
    if scaler:
        ls = LossScaler(1024.0)
        for m in models:
            m.loss_scaler = ls
    if group == "model":
        return models[0], models
    if group == "cascade":
        return Cascade(*models), models
    if group == "scene":
        return BackgroundScene(models[0], models[1], synth.SPHERE_CENTER, synth.SPHERE_RADIUS), models
    cen = np.array([[-0.5, -0.4, 0.1], [0.5, -0.3, -0.2], [0.0, 0.5, 0.3]], np.float32)
    return MegaNeRF(models, cen, 1.15, False, False, joint_training=True), models


def _f(x):
    return "%.10g" % x


def drive(group, owner, models, A, scaler, calls, allreduce, refresh):
    """The apply_step calls of one case on an owner from _build -> what each returned (scripts/step_launch_trace.py drives its tail
    cases through this too).  Every call starts from a gradient of ones; with a scaler each model records the current scale as the one
    its backward used, as grad_step does."""
    if A > 1:
        owner.set_accumulation(A)
    ret = []
    for c in calls:
        c = dict(c)
        for m in models:
            m.grad.fill_(1.0)
            if scaler:
                m._loss_scale_tensor()
        if "inf" in c:
            what, i = c.pop("inf")
            getattr(models[i], what)[0] = INF
        kw = dict(grad_allreduce=allreduce) if c.pop("allreduce", False) else {}
        if group == "scene":
            ctx = dict(Nb=c.pop("Nb"))
            if c.pop("padded", False):
                ctx.update(C=4, N=8, n_out=0)
            if "refresh" in c:
                c["refresh"] = refresh
            res = owner.apply_step(dict(ctx=ctx), **kw, **c)
            ret.append({k: v for k, v in res.items() if k != "ctx"})
        else:
            ret.append(owner.apply_step(**kw, **c))
    return ret


def run_case(monkeypatch, group, kind="dense", A=1, scaler=False, calls=()):
    """calls: one dict per apply_step call - allreduce (bool: the stub returning 0.5), inf (("grad" | "accum", model index) planted
    before the call), Nb / padded / advance / refresh (scene), and apply_step's own optimizer_step / should_accumulate."""
    from switch_nerf_amd import ops
    from switch_nerf_amd.model import SwitchNeRF
    owner, models = _build(group, kind, scaler)
    log = []

    def who(t):
        for i, m in enumerate(models):
            for name in ("flat", "grad", "accum"):
                b = getattr(m, name, None)
                if b is not None and b.data_ptr() == t.data_ptr():
                    return "m%d" % i + ("" if name == "flat" else "." + name)
        raise AssertionError("a tensor of no model")

    def adam_step(param, grad, m, v, shadow, step, lr, grad_scale=1.0):
        assert who(grad) == who(param) + ".grad"
        log.append("adam(%s,%d,%s)" % (who(param), step, _f(grad_scale)))

    def grad_accum(acc, grad, scale):
        assert who(acc) == who(grad)[:2] + ".accum"
        acc.add_(grad * scale)
        log.append("accum(%s,%s)" % (who(grad)[:2], _f(scale)))

    def adam_accum_step(param, acc, grad, m, v, shadow, step, lr, accum_scale=1.0, grad_scale=1.0):
        assert who(acc) == who(param) + ".accum" and (grad is None or who(grad) == who(param) + ".grad")
        acc.zero_()                        # (the kernel leaves the buffer cleared)
        log.append("adam_accum(%s,%s,%d,%s,%s)" % (who(param), "+g" if grad is not None else "-g", step, _f(accum_scale), _f(grad_scale)))

    monkeypatch.setattr(ops, "adam_step", adam_step)
    monkeypatch.setattr(ops, "grad_accum", grad_accum)
    monkeypatch.setattr(ops, "adam_accum_step", adam_accum_step)
    monkeypatch.setattr(SwitchNeRF, "refresh_compute_copies", lambda self: log.append("refresh(%s)" % who(self.flat)))

    def allreduce(view):
        log.append("allreduce(%s)" % who(view))
        return 0.5

    ret = drive(group, owner, models, A, scaler, calls, allreduce, lambda: log.append("refresh(*)"))
    ls = models[0].loss_scaler
    got = dict(ret=ret, step=[m.step_count for m in models], micro=[m._micro for m in models],
               scale=None if ls is None else ls.scale, skipped=None if ls is None else ls.skipped,
               applied=[getattr(m, "_applied_loss_scale", None) for m in models],
               zero=[None if m.accum is None else not bool(m.accum.any()) for m in models], calls=log)
    if group == "mega":
        got["owner_step"] = owner.step_count
    return got


AR = dict(allreduce=True)
CASES = {}
for _k in ("moe", "dense"):
    for _name, _kw in {
        "a1": dict(calls=[{}, {}]),
        "a1_scaler": dict(scaler=True, calls=[{}]),
        "a1_allreduce": dict(calls=[AR]),
        "a1_scaler_allreduce": dict(scaler=True, calls=[AR]),
        "a1_nostep": dict(scaler=True, calls=[dict(AR, optimizer_step=False)]),
        "a1_scaler_inf": dict(scaler=True, calls=[dict(inf=("grad", 0)), {}]),
        "a3": dict(A=3, calls=[{}] * 4),
        "a3_scaler": dict(A=3, scaler=True, calls=[{}] * 3),
        "a3_allreduce": dict(A=3, calls=[AR] * 3),
        "a3_scaler_allreduce": dict(A=3, scaler=True, calls=[AR] * 3),
        "a3_nostep": dict(A=3, calls=[{}, {}, dict(optimizer_step=False), {}]),
        "a3_explicit": dict(A=3, calls=[dict(should_accumulate=False), {}, dict(should_accumulate=True), dict(should_accumulate=False)]),
        "a3_scaler_inf_grad": dict(A=3, scaler=True, calls=[{}, {}, dict(inf=("grad", 0)), {}]),
        "a3_scaler_inf_buffer": dict(A=3, scaler=True, calls=[{}, dict(inf=("accum", 0)), {}]),
        "a3_allreduce_scaler_inf_grad": dict(A=3, scaler=True, calls=[AR, AR, dict(AR, inf=("grad", 0))]),
    }.items():
        CASES["%s_%s" % (_k, _name)] = dict(group="model", kind=_k, **_kw)
CASES.update({
    "cascade_a1": dict(group="cascade", calls=[{}, dict(optimizer_step=False)]),
    "cascade_a1_scaler": dict(group="cascade", scaler=True, calls=[{}]),
    "cascade_a1_scaler_inf_fine": dict(group="cascade", scaler=True, calls=[dict(inf=("grad", 1)), {}]),
    "cascade_a2": dict(group="cascade", A=2, calls=[{}, {}, dict(should_accumulate=False)]),
    "cascade_a2_nostep": dict(group="cascade", A=2, calls=[{}, dict(optimizer_step=False)]),
    "cascade_a2_scaler": dict(group="cascade", A=2, scaler=True, calls=[{}, {}]),
    "cascade_a2_scaler_inf_fine": dict(group="cascade", A=2, scaler=True, calls=[{}, dict(inf=("grad", 1)), {}, {}]),
    "cascade_a2_scaler_inf_fine_buffer": dict(group="cascade", A=2, scaler=True, calls=[dict(inf=("accum", 1)), {}]),
    "scene_a1": dict(group="scene", calls=[dict(Nb=3), dict(Nb=0), dict(Nb=3, optimizer_step=False)]),
    "scene_a1_scaler": dict(group="scene", scaler=True, calls=[dict(Nb=3), dict(Nb=0)]),
    "scene_a1_scaler_inf_bg": dict(group="scene", scaler=True, calls=[dict(Nb=3, inf=("grad", 1)), dict(Nb=3)]),
    "scene_a1_scaler_inf_bg_absent": dict(group="scene", scaler=True, calls=[dict(Nb=0, inf=("grad", 1))]),
    "scene_a1_scaler_inf_fg": dict(group="scene", scaler=True, calls=[dict(Nb=3, inf=("grad", 0))]),
    "scene_a1_allreduce": dict(group="scene", calls=[dict(AR, Nb=0), dict(AR, Nb=0, optimizer_step=False)]),
    "scene_a1_padded_refresh": dict(group="scene", scaler=True, calls=[dict(Nb=2, padded=True, refresh=True, advance=False),
                                                                       dict(Nb=0, padded=True, refresh=True, advance=False),
                                                                       dict(Nb=2, padded=True, refresh=True, advance=False, inf=("grad", 0)),
                                                                       dict(Nb=2, padded=True, refresh=True, advance=False, optimizer_step=False)]),
    "scene_a2_bg_bg": dict(group="scene", A=2, calls=[dict(Nb=3), dict(Nb=3)]),
    "scene_a2_nobg_bg": dict(group="scene", A=2, calls=[dict(Nb=0), dict(Nb=3)]),
    "scene_a2_bg_nobg": dict(group="scene", A=2, calls=[dict(Nb=3), dict(Nb=0)]),
    "scene_a2_nobg_nobg": dict(group="scene", A=2, calls=[dict(Nb=0), dict(Nb=0)]),
    "scene_a2_nostep": dict(group="scene", A=2, calls=[dict(Nb=3), dict(Nb=3, optimizer_step=False), dict(Nb=3, should_accumulate=False)]),
    "scene_a2_scaler": dict(group="scene", A=2, scaler=True, calls=[dict(Nb=3), dict(Nb=3)]),
    "scene_a2_scaler_bg_nobg": dict(group="scene", A=2, scaler=True, calls=[dict(Nb=3), dict(Nb=0)]),
    "scene_a2_scaler_inf_bg": dict(group="scene", A=2, scaler=True, calls=[dict(Nb=3), dict(Nb=3, inf=("grad", 1)), dict(Nb=3), dict(Nb=3)]),
    "scene_a2_scaler_inf_bg_buffer": dict(group="scene", A=2, scaler=True, calls=[dict(Nb=3, inf=("accum", 1)), dict(Nb=3)]),
    "scene_a2_allreduce": dict(group="scene", A=2, calls=[dict(AR, Nb=0), dict(AR, Nb=0)]),
    "scene_a2_allreduce_scaler_inf_fg": dict(group="scene", A=2, scaler=True, calls=[dict(AR, Nb=3), dict(AR, Nb=3, inf=("grad", 0))]),
    "mega_two_steps": dict(group="mega", calls=[{}, dict(optimizer_step=False), {}]),
})

# written down from the parent of the commit that added switch_nerf_amd/optim.py (see the module doc)
EXPECTED = {
    "moe_a1": dict(ret=[None, None], step=[2], micro=[0], scale=None, skipped=None, applied=[None], zero=[None],
        calls=["adam(m0,1,1)", "refresh(m0)", "adam(m0,2,1)", "refresh(m0)"]),
    "moe_a1_scaler": dict(ret=[None], step=[1], micro=[0], scale=1024.0, skipped=0, applied=[1024.0], zero=[None],
        calls=["adam(m0,1,0.0009765625)", "refresh(m0)"]),
    "moe_a1_allreduce": dict(ret=[None], step=[1], micro=[0], scale=None, skipped=None, applied=[None], zero=[None],
        calls=["allreduce(m0.grad)", "adam(m0,1,0.5)", "refresh(m0)"]),
    "moe_a1_scaler_allreduce": dict(ret=[None], step=[1], micro=[0], scale=1024.0, skipped=0, applied=[1024.0], zero=[None],
        calls=["allreduce(m0.grad)", "adam(m0,1,0.00048828125)", "refresh(m0)"]),
    "moe_a1_nostep": dict(ret=[None], step=[0], micro=[0], scale=1024.0, skipped=0, applied=[None], zero=[None],
        calls=["allreduce(m0.grad)"]),
    "moe_a1_scaler_inf": dict(ret=[None, None], step=[1], micro=[0], scale=512.0, skipped=1, applied=[512.0], zero=[None],
        calls=["adam(m0,1,0.001953125)", "refresh(m0)"]),
    "moe_a3": dict(ret=[False, False, True, False], step=[1], micro=[4], scale=None, skipped=None, applied=[None], zero=[False],
        calls=["accum(m0,0.3333333333)", "accum(m0,0.3333333333)", "adam_accum(m0,+g,1,0.3333333333,1)", "refresh(m0)", "accum(m0,0.3333333333)"]),
    "moe_a3_scaler": dict(ret=[False, False, True], step=[1], micro=[3], scale=1024.0, skipped=0, applied=[1024.0], zero=[True],
        calls=["accum(m0,0.3333333333)", "accum(m0,0.3333333333)", "accum(m0,0.3333333333)", "adam_accum(m0,-g,1,1,0.0009765625)", "refresh(m0)"]),
    "moe_a3_allreduce": dict(ret=[False, False, True], step=[1], micro=[3], scale=None, skipped=None, applied=[None], zero=[True],
        calls=["accum(m0,0.3333333333)", "accum(m0,0.3333333333)", "accum(m0,0.3333333333)", "allreduce(m0.accum)", "adam_accum(m0,-g,1,1,0.5)",
               "refresh(m0)"]),
    "moe_a3_scaler_allreduce": dict(ret=[False, False, True], step=[1], micro=[3], scale=1024.0, skipped=0, applied=[1024.0], zero=[True],
        calls=["accum(m0,0.3333333333)", "accum(m0,0.3333333333)", "accum(m0,0.3333333333)", "allreduce(m0.accum)",
               "adam_accum(m0,-g,1,1,0.00048828125)", "refresh(m0)"]),
    "moe_a3_nostep": dict(ret=[False, False, False, False], step=[0], micro=[4], scale=None, skipped=None, applied=[None], zero=[False],
        calls=["accum(m0,0.3333333333)", "accum(m0,0.3333333333)", "accum(m0,0.3333333333)", "accum(m0,0.3333333333)"]),
    "moe_a3_explicit": dict(ret=[True, False, False, True], step=[2], micro=[4], scale=None, skipped=None, applied=[None], zero=[True],
        calls=["adam_accum(m0,+g,1,0.3333333333,1)", "refresh(m0)", "accum(m0,0.3333333333)", "accum(m0,0.3333333333)",
               "adam_accum(m0,+g,2,0.3333333333,1)", "refresh(m0)"]),
    "moe_a3_scaler_inf_grad": dict(ret=[False, False, False, False], step=[0], micro=[4], scale=512.0, skipped=1, applied=[1024.0], zero=[False],
        calls=["accum(m0,0.3333333333)", "accum(m0,0.3333333333)", "accum(m0,0.3333333333)", "accum(m0,0.3333333333)"]),
    "moe_a3_scaler_inf_buffer": dict(ret=[False, False, False], step=[0], micro=[3], scale=512.0, skipped=1, applied=[1024.0], zero=[True],
        calls=["accum(m0,0.3333333333)", "accum(m0,0.3333333333)", "accum(m0,0.3333333333)"]),
    "moe_a3_allreduce_scaler_inf_grad": dict(ret=[False, False, False], step=[0], micro=[3], scale=512.0, skipped=1, applied=[1024.0], zero=[True],
        calls=["accum(m0,0.3333333333)", "accum(m0,0.3333333333)", "accum(m0,0.3333333333)", "allreduce(m0.accum)"]),
    "dense_a1": dict(ret=[None, None], step=[2], micro=[0], scale=None, skipped=None, applied=[None], zero=[None],
        calls=["adam(m0,1,1)", "refresh(m0)", "adam(m0,2,1)", "refresh(m0)"]),
    "dense_a1_scaler": dict(ret=[None], step=[1], micro=[0], scale=1024.0, skipped=0, applied=[1024.0], zero=[None],
        calls=["adam(m0,1,0.0009765625)", "refresh(m0)"]),
    "dense_a1_allreduce": dict(ret=[None], step=[1], micro=[0], scale=None, skipped=None, applied=[None], zero=[None],
        calls=["allreduce(m0.grad)", "adam(m0,1,0.5)", "refresh(m0)"]),
    "dense_a1_scaler_allreduce": dict(ret=[None], step=[1], micro=[0], scale=1024.0, skipped=0, applied=[1024.0], zero=[None],
        calls=["allreduce(m0.grad)", "adam(m0,1,0.00048828125)", "refresh(m0)"]),
    "dense_a1_nostep": dict(ret=[None], step=[0], micro=[0], scale=1024.0, skipped=0, applied=[None], zero=[None],
        calls=["allreduce(m0.grad)"]),
    "dense_a1_scaler_inf": dict(ret=[None, None], step=[1], micro=[0], scale=512.0, skipped=1, applied=[512.0], zero=[None],
        calls=["adam(m0,1,0.001953125)", "refresh(m0)"]),
    "dense_a3": dict(ret=[False, False, True, False], step=[1], micro=[4], scale=None, skipped=None, applied=[None], zero=[False],
        calls=["accum(m0,0.3333333333)", "accum(m0,0.3333333333)", "adam_accum(m0,+g,1,0.3333333333,1)", "refresh(m0)", "accum(m0,0.3333333333)"]),
    "dense_a3_scaler": dict(ret=[False, False, True], step=[1], micro=[3], scale=1024.0, skipped=0, applied=[1024.0], zero=[True],
        calls=["accum(m0,0.3333333333)", "accum(m0,0.3333333333)", "accum(m0,0.3333333333)", "adam_accum(m0,-g,1,1,0.0009765625)", "refresh(m0)"]),
    "dense_a3_allreduce": dict(ret=[False, False, True], step=[1], micro=[3], scale=None, skipped=None, applied=[None], zero=[True],
        calls=["accum(m0,0.3333333333)", "accum(m0,0.3333333333)", "accum(m0,0.3333333333)", "allreduce(m0.accum)", "adam_accum(m0,-g,1,1,0.5)",
               "refresh(m0)"]),
    "dense_a3_scaler_allreduce": dict(ret=[False, False, True], step=[1], micro=[3], scale=1024.0, skipped=0, applied=[1024.0], zero=[True],
        calls=["accum(m0,0.3333333333)", "accum(m0,0.3333333333)", "accum(m0,0.3333333333)", "allreduce(m0.accum)",
               "adam_accum(m0,-g,1,1,0.00048828125)", "refresh(m0)"]),
    "dense_a3_nostep": dict(ret=[False, False, False, False], step=[0], micro=[4], scale=None, skipped=None, applied=[None], zero=[False],
        calls=["accum(m0,0.3333333333)", "accum(m0,0.3333333333)", "accum(m0,0.3333333333)", "accum(m0,0.3333333333)"]),
    "dense_a3_explicit": dict(ret=[True, False, False, True], step=[2], micro=[4], scale=None, skipped=None, applied=[None], zero=[True],
        calls=["adam_accum(m0,+g,1,0.3333333333,1)", "refresh(m0)", "accum(m0,0.3333333333)", "accum(m0,0.3333333333)",
               "adam_accum(m0,+g,2,0.3333333333,1)", "refresh(m0)"]),
    "dense_a3_scaler_inf_grad": dict(ret=[False, False, False, False], step=[0], micro=[4], scale=512.0, skipped=1, applied=[1024.0], zero=[False],
        calls=["accum(m0,0.3333333333)", "accum(m0,0.3333333333)", "accum(m0,0.3333333333)", "accum(m0,0.3333333333)"]),
    "dense_a3_scaler_inf_buffer": dict(ret=[False, False, False], step=[0], micro=[3], scale=512.0, skipped=1, applied=[1024.0], zero=[True],
        calls=["accum(m0,0.3333333333)", "accum(m0,0.3333333333)", "accum(m0,0.3333333333)"]),
    "dense_a3_allreduce_scaler_inf_grad": dict(ret=[False, False, False], step=[0], micro=[3], scale=512.0, skipped=1, applied=[1024.0], zero=[True],
        calls=["accum(m0,0.3333333333)", "accum(m0,0.3333333333)", "accum(m0,0.3333333333)", "allreduce(m0.accum)"]),
    "cascade_a1": dict(ret=[None, None], step=[1, 1], micro=[0, 0], scale=None, skipped=None, applied=[None, None], zero=[None, None],
        calls=["adam(m0,1,1)", "refresh(m0)", "adam(m1,1,1)", "refresh(m1)"]),
    "cascade_a1_scaler": dict(ret=[None], step=[1, 1], micro=[0, 0], scale=1024.0, skipped=0, applied=[1024.0, 1024.0], zero=[None, None],
        calls=["adam(m0,1,0.0009765625)", "refresh(m0)", "adam(m1,1,0.0009765625)", "refresh(m1)"]),
    "cascade_a1_scaler_inf_fine": dict(ret=[None, None], step=[1, 1], micro=[0, 0], scale=512.0, skipped=1, applied=[512.0, 512.0], zero=[None, None],
        calls=["adam(m0,1,0.001953125)", "refresh(m0)", "adam(m1,1,0.001953125)", "refresh(m1)"]),
    "cascade_a2": dict(ret=[False, True, True], step=[2, 2], micro=[3, 3], scale=None, skipped=None, applied=[None, None], zero=[True, True],
        calls=["accum(m0,0.5)", "accum(m1,0.5)", "adam_accum(m0,+g,1,0.5,1)", "refresh(m0)", "adam_accum(m1,+g,1,0.5,1)", "refresh(m1)",
               "adam_accum(m0,+g,2,0.5,1)", "refresh(m0)", "adam_accum(m1,+g,2,0.5,1)", "refresh(m1)"]),
    "cascade_a2_nostep": dict(ret=[False, False], step=[0, 0], micro=[2, 2], scale=None, skipped=None, applied=[None, None], zero=[False, False],
        calls=["accum(m0,0.5)", "accum(m1,0.5)", "accum(m0,0.5)", "accum(m1,0.5)"]),
    "cascade_a2_scaler": dict(ret=[False, True], step=[1, 1], micro=[2, 2], scale=1024.0, skipped=0, applied=[1024.0, 1024.0], zero=[True, True],
        calls=["accum(m0,0.5)", "accum(m1,0.5)", "accum(m0,0.5)", "accum(m1,0.5)", "adam_accum(m0,-g,1,1,0.0009765625)", "refresh(m0)",
               "adam_accum(m1,-g,1,1,0.0009765625)", "refresh(m1)"]),
    "cascade_a2_scaler_inf_fine": dict(ret=[False, False, False, True], step=[1, 1], micro=[4, 4], scale=512.0, skipped=1, applied=[512.0, 512.0], zero=[True, True],
        calls=["accum(m0,0.5)", "accum(m1,0.5)", "accum(m0,0.5)", "accum(m1,0.5)", "accum(m0,0.5)", "accum(m1,0.5)", "accum(m0,0.5)",
               "accum(m1,0.5)", "adam_accum(m0,-g,1,1,0.001953125)", "refresh(m0)", "adam_accum(m1,-g,1,1,0.001953125)", "refresh(m1)"]),
    "cascade_a2_scaler_inf_fine_buffer": dict(ret=[False, False], step=[0, 0], micro=[2, 2], scale=512.0, skipped=1, applied=[1024.0, 1024.0], zero=[True, True],
        calls=["accum(m0,0.5)", "accum(m1,0.5)", "accum(m0,0.5)", "accum(m1,0.5)"]),
    "scene_a1": dict(
        ret=[{'bg_nerf_rays_present': True},
             {'bg_nerf_rays_present': False},
             {'bg_nerf_rays_present': True}],
        step=[2, 1], micro=[0, 0], scale=None, skipped=None, applied=[None, None], zero=[None, None],
        calls=["adam(m0,1,1)", "refresh(m0)", "adam(m1,1,1)", "refresh(m1)", "adam(m0,2,1)", "refresh(m0)"]),
    "scene_a1_scaler": dict(
        ret=[{'bg_nerf_rays_present': True},
             {'bg_nerf_rays_present': False}],
        step=[2, 1], micro=[0, 0], scale=1024.0, skipped=0, applied=[1024.0, 1024.0], zero=[None, None],
        calls=["adam(m0,1,0.0009765625)", "refresh(m0)", "adam(m1,1,0.0009765625)", "refresh(m1)", "adam(m0,2,0.0009765625)", "refresh(m0)"]),
    "scene_a1_scaler_inf_bg": dict(
        ret=[{'bg_nerf_rays_present': True},
             {'bg_nerf_rays_present': True}],
        step=[2, 1], micro=[0, 0], scale=512.0, skipped=1, applied=[512.0, 512.0], zero=[None, None],
        calls=["adam(m0,1,0.0009765625)", "refresh(m0)", "adam(m0,2,0.001953125)", "refresh(m0)", "adam(m1,1,0.001953125)", "refresh(m1)"]),
    "scene_a1_scaler_inf_bg_absent": dict(
        ret=[{'bg_nerf_rays_present': False}],
        step=[1, 0], micro=[0, 0], scale=1024.0, skipped=0, applied=[1024.0, None], zero=[None, None],
        calls=["adam(m0,1,0.0009765625)", "refresh(m0)"]),
    "scene_a1_scaler_inf_fg": dict(
        ret=[{'bg_nerf_rays_present': True}],
        step=[0, 1], micro=[0, 0], scale=512.0, skipped=1, applied=[1024.0, 1024.0], zero=[None, None],
        calls=["adam(m1,1,0.0009765625)", "refresh(m1)"]),
    "scene_a1_allreduce": dict(
        ret=[{'bg_nerf_rays_present': True},
             {'bg_nerf_rays_present': True}],
        step=[1, 1], micro=[0, 0], scale=None, skipped=None, applied=[None, None], zero=[None, None],
        calls=["allreduce(m0.grad)", "allreduce(m1.grad)", "adam(m0,1,0.5)", "refresh(m0)", "adam(m1,1,0.5)", "refresh(m1)", "allreduce(m0.grad)",
               "allreduce(m1.grad)"]),
    "scene_a1_padded_refresh": dict(
        ret=[{'bg_nerf_rays_present': True},
             {'bg_nerf_rays_present': False},
             {'bg_nerf_rays_present': True},
             {'bg_nerf_rays_present': True}],
        step=[2, 2], micro=[0, 0], scale=512.0, skipped=1, applied=[1024.0, 1024.0], zero=[None, None],
        calls=["adam(m0,1,0.0009765625)", "adam(m1,1,0.0009765625)", "refresh(*)", "adam(m0,2,0.0009765625)", "refresh(*)",
               "adam(m1,2,0.0009765625)", "refresh(*)"]),
    "scene_a2_bg_bg": dict(
        ret=[{'bg_nerf_rays_present': True, 'optimizer_stepped': False},
             {'bg_nerf_rays_present': True, 'optimizer_stepped': True}],
        step=[1, 1], micro=[2, 2], scale=None, skipped=None, applied=[None, None], zero=[True, True],
        calls=["accum(m0,0.5)", "accum(m1,0.5)", "adam_accum(m0,+g,1,0.5,1)", "refresh(m0)", "adam_accum(m1,+g,1,0.5,1)", "refresh(m1)"]),
    "scene_a2_nobg_bg": dict(
        ret=[{'bg_nerf_rays_present': False, 'optimizer_stepped': False},
             {'bg_nerf_rays_present': True, 'optimizer_stepped': True}],
        step=[1, 1], micro=[2, 2], scale=None, skipped=None, applied=[None, None], zero=[True, True],
        calls=["accum(m0,0.5)", "adam_accum(m0,+g,1,0.5,1)", "refresh(m0)", "adam_accum(m1,+g,1,0.5,1)", "refresh(m1)"]),
    "scene_a2_bg_nobg": dict(
        ret=[{'bg_nerf_rays_present': True, 'optimizer_stepped': False},
             {'bg_nerf_rays_present': False, 'optimizer_stepped': True}],
        step=[1, 0], micro=[2, 2], scale=None, skipped=None, applied=[None, None], zero=[True, True],
        calls=["accum(m0,0.5)", "accum(m1,0.5)", "adam_accum(m0,+g,1,0.5,1)", "refresh(m0)"]),
    "scene_a2_nobg_nobg": dict(
        ret=[{'bg_nerf_rays_present': False, 'optimizer_stepped': False},
             {'bg_nerf_rays_present': False, 'optimizer_stepped': True}],
        step=[1, 0], micro=[2, 2], scale=None, skipped=None, applied=[None, None], zero=[True, True],
        calls=["accum(m0,0.5)", "adam_accum(m0,+g,1,0.5,1)", "refresh(m0)"]),
    "scene_a2_nostep": dict(
        ret=[{'bg_nerf_rays_present': True, 'optimizer_stepped': False},
             {'bg_nerf_rays_present': True, 'optimizer_stepped': False},
             {'bg_nerf_rays_present': True, 'optimizer_stepped': True}],
        step=[1, 1], micro=[3, 3], scale=None, skipped=None, applied=[None, None], zero=[True, True],
        calls=["accum(m0,0.5)", "accum(m1,0.5)", "accum(m0,0.5)", "accum(m1,0.5)", "adam_accum(m0,+g,1,0.5,1)", "refresh(m0)",
               "adam_accum(m1,+g,1,0.5,1)", "refresh(m1)"]),
    "scene_a2_scaler": dict(
        ret=[{'bg_nerf_rays_present': True, 'optimizer_stepped': False},
             {'bg_nerf_rays_present': True, 'optimizer_stepped': True}],
        step=[1, 1], micro=[2, 2], scale=1024.0, skipped=0, applied=[1024.0, 1024.0], zero=[True, True],
        calls=["accum(m0,0.5)", "accum(m1,0.5)", "accum(m0,0.5)", "accum(m1,0.5)", "adam_accum(m0,-g,1,1,0.0009765625)", "refresh(m0)",
               "adam_accum(m1,-g,1,1,0.0009765625)", "refresh(m1)"]),
    "scene_a2_scaler_bg_nobg": dict(
        ret=[{'bg_nerf_rays_present': True, 'optimizer_stepped': False},
             {'bg_nerf_rays_present': False, 'optimizer_stepped': True}],
        step=[1, 0], micro=[2, 2], scale=1024.0, skipped=0, applied=[1024.0, None], zero=[True, True],
        calls=["accum(m0,0.5)", "accum(m1,0.5)", "accum(m0,0.5)", "accum(m1,0.5)", "adam_accum(m0,-g,1,1,0.0009765625)", "refresh(m0)"]),
    "scene_a2_scaler_inf_bg": dict(
        ret=[{'bg_nerf_rays_present': True, 'optimizer_stepped': False},
             {'bg_nerf_rays_present': True, 'optimizer_stepped': True},
             {'bg_nerf_rays_present': True, 'optimizer_stepped': False},
             {'bg_nerf_rays_present': True, 'optimizer_stepped': True}],
        step=[2, 1], micro=[4, 4], scale=512.0, skipped=1, applied=[512.0, 512.0], zero=[True, True],
        calls=["accum(m0,0.5)", "accum(m1,0.5)", "accum(m0,0.5)", "accum(m1,0.5)", "adam_accum(m0,-g,1,1,0.0009765625)", "refresh(m0)",
               "accum(m0,0.5)", "accum(m1,0.5)", "accum(m0,0.5)", "accum(m1,0.5)", "adam_accum(m0,-g,2,1,0.001953125)", "refresh(m0)",
               "adam_accum(m1,-g,1,1,0.001953125)", "refresh(m1)"]),
    "scene_a2_scaler_inf_bg_buffer": dict(
        ret=[{'bg_nerf_rays_present': True, 'optimizer_stepped': False},
             {'bg_nerf_rays_present': True, 'optimizer_stepped': True}],
        step=[1, 0], micro=[2, 2], scale=512.0, skipped=1, applied=[1024.0, 1024.0], zero=[True, True],
        calls=["accum(m0,0.5)", "accum(m1,0.5)", "accum(m0,0.5)", "accum(m1,0.5)", "adam_accum(m0,-g,1,1,0.0009765625)", "refresh(m0)"]),
    "scene_a2_allreduce": dict(
        ret=[{'bg_nerf_rays_present': True, 'optimizer_stepped': False},
             {'bg_nerf_rays_present': True, 'optimizer_stepped': True}],
        step=[1, 1], micro=[2, 2], scale=None, skipped=None, applied=[None, None], zero=[True, True],
        calls=["accum(m0,0.5)", "accum(m0,0.5)", "allreduce(m0.accum)", "accum(m1,0.5)", "allreduce(m1.accum)", "adam_accum(m0,-g,1,1,0.5)",
               "refresh(m0)", "adam_accum(m1,-g,1,1,0.5)", "refresh(m1)"]),
    "scene_a2_allreduce_scaler_inf_fg": dict(
        ret=[{'bg_nerf_rays_present': True, 'optimizer_stepped': False},
             {'bg_nerf_rays_present': True, 'optimizer_stepped': True}],
        step=[0, 1], micro=[2, 2], scale=512.0, skipped=1, applied=[1024.0, 1024.0], zero=[True, True],
        calls=["accum(m0,0.5)", "accum(m1,0.5)", "accum(m0,0.5)", "allreduce(m0.accum)", "accum(m1,0.5)", "allreduce(m1.accum)",
               "adam_accum(m1,-g,1,1,0.00048828125)", "refresh(m1)"]),
    "mega_two_steps": dict(ret=[None, None, None], step=[2, 2, 2], micro=[0, 0, 0], scale=None, skipped=None, applied=[None, None, None], zero=[None, None, None], owner_step=2,
        calls=["adam(m0,1,1)", "refresh(m0)", "adam(m1,1,1)", "refresh(m1)", "adam(m2,1,1)", "refresh(m2)", "adam(m0,2,1)", "refresh(m0)",
               "adam(m1,2,1)", "refresh(m1)", "adam(m2,2,1)", "refresh(m2)"]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_tail_host_state(name, monkeypatch):
    got = run_case(monkeypatch, **CASES[name])
    assert got == EXPECTED[name]
