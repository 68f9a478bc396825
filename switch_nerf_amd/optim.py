"""The host-side tail of a training step, written once for the owners of several models (Cascade, BackgroundScene, MegaNeRF): gradient
all-reduce -> fp16 found-inf check with the update of the shared loss scaler -> the gradient-accumulation window -> Adam -> refresh of
the compute copies (runner.py:486, 589, 677-690).  The owners differ in three things only - which models form the group, which of them
step this time, and whether a non-finite gradient skips the one model or the whole group - and pass exactly those.  It is
SwitchNeRF.apply_step / _apply_step_accum over a group: a group of one model takes the same steps as that model's own apply_step
(tests/test_optim_tail_cpu.py pins both on the same expectations), which still has its own text."""
from __future__ import annotations

from . import ops


def sync_loss_scale(models):
    """Bring every model's device copy of the loss scale up to the scaler's host value (each also records it as the scale its next
    backward uses) -> the first model's device scalar; None, and nothing done, without a loss scaler."""
    if models[0].loss_scaler is None:
        return None
    return [m._loss_scale_tensor() for m in models][0]


def distributed() -> bool:
    import torch.distributed as dist
    return dist.is_available() and dist.is_initialized()


def _guard_flag(models, grad_allreduce, flag_allreduce=None):
    """The finite guard's device flag for this step (None: the guard is off).  The group shares ONE flag, written behind the loss
    kernel (SwitchNeRF._finite_guard).  In a torch.distributed run the ranks agree on it here - MIN over the ranks, the reference's
    `sum == world_size` (runner.py:660-666), on every step, accumulating ones included - and the skipped step is counted behind that.
    The reduction is flag_allreduce(flag), or grad_allreduce.all_ranks_ok where the caller passes a GradAllReduce itself; a caller
    that wraps its all-reduce (GraphedTrainStep's split backward hands over a closure) passes flag_allreduce.  With more than one
    rank and neither, the step raises: ranks that judged their own batches alone would take different steps on one summed gradient."""
    first = models[0]
    if not first.check_finite:
        if any(m.check_finite for m in models):
            raise ValueError("check_finite is on for some models of the group only: switch it on through their owner's set_check_finite")
        return None
    ok = first._guard["ok"]
    if any(not m.check_finite or m._guard["ok"] is not ok for m in models):
        raise ValueError("check_finite: the models of one step must share one flag: switch it on through their owner's set_check_finite")
    if distributed():
        import torch.distributed as dist
        reduce = flag_allreduce if flag_allreduce is not None else getattr(grad_allreduce, "all_ranks_ok", None)
        if reduce is not None:
            reduce(ok)
        elif dist.get_world_size() > 1:
            raise RuntimeError("check_finite: this step runs on several ranks but was given nothing that combines their flags: pass "
                               "grad_allreduce=parallel.make_grad_allreduce(...) or flag_allreduce=its all_ranks_ok")
        first._guard["skipped"].add_(1 - ok)
    return ok


def apply_tail(models, stepping=None, zero_grad=(), skip_together=False, grad_allreduce=None, optimizer_step=True, refresh=None,
               should_accumulate=None, flag_allreduce=None) -> bool:
    """The tail over a group of models -> whether any optimizer stepped.
    models: the group, in order; the first one owns the accumulation window (accum_steps, the micro-step index the others follow) and
    its loss scaler is the group's.  stepping: the models that may take an optimizer step this time (default: all).  zero_grad: models
    whose gradient is known to be zero - an accumulating micro-step does not add them.  skip_together: a non-finite gradient in any
    stepping model skips all of them; otherwise each skips on its own gradient.  Either way the one scaler is updated once, with the OR.
    grad_allreduce(view) -> the scale that turns the summed gradient into the mean; refresh: a replacement for every model's
    refresh_compute_copies (the replay of their captured graph), run once behind the last Adam.

    Accumulation off (A = 1): all-reduce of every model's gradient (stepping or not, before optimizer_step is looked at), inf check,
    one adam_step per model that steps.
    Accumulation on: an accumulating micro-step (the window rule, should_accumulate, or optimizer_step=False) adds grad / A into the
    buffers and does nothing else: no all-reduce (DDP's no_sync), no inf check, no Adam, no refresh.  The last micro-step without a
    loss scaler and without an all-reduce is ONE launch per model (swn_adam_accum_step: the last gradient never reaches the buffer,
    which leaves cleared).  Otherwise: add, one all-reduce of the buffer, the inf check on it - the loss scale changes only here, so
    every micro-gradient of a window carried the same scale (GradScaler's accumulation rule) - then Adam from the buffer.  The buffer
    of a model that does not step - skipped, or not in `stepping` - is cleared (zero_grad follows anyway: runner.py:689-690).

    Finite guard on (set_check_finite; the step's metrics were judged behind the loss kernel): the same launches in their guarded
    forms, which read the device flag - nothing is read on the host, and the return value says that the optimizer launches were
    issued (res["step_ok"] says whether they took effect).  A flagged step leaves parameters, moments and each model's device step
    count alone and clears the accumulation buffers, on an accumulating micro-step too (the reference's zero_grad, runner.py:668-669;
    a model in `zero_grad` is then added like the others: the launch that adds its zeros is the one that clears).  With a loss
    scaler the host already reads found-inf on every step; the flag is read with it, in front of the scaler: a flagged step returns
    before GradScaler.step / update, and one that passes goes through found-inf as before."""
    first = models[0]
    ok = _guard_flag(models, grad_allreduce, flag_allreduce)
    scaler, A = first.loss_scaler, first.accum_steps
    inv, fused = 1.0 / A, False
    accum_add = ops.grad_accum if ok is None else (lambda acc, grad, s: ops.grad_accum_guarded(acc, grad, s, ok))
    if A > 1:
        accumulates = first._accumulates(should_accumulate) or not optimizer_step
        for m in models[1:]:
            m._micro = first._micro
        if accumulates:
            for m in models:
                if m not in zero_grad or ok is not None:
                    accum_add(m.accum, m.grad, inv)
            return False
        fused = grad_allreduce is None and scaler is None
    scale = []
    for m in models:
        if A > 1 and not fused:
            accum_add(m.accum, m.grad, inv)
        scale.append(grad_allreduce(m._allreduce_view()) if grad_allreduce is not None else 1.0)
    if not optimizer_step:
        return False
    live = models if stepping is None else stepping
    if scaler is not None and ok is not None and not bool(ok.item()):
        return False                          # (the reference `continue`s in front of scaler.step / update; the buffers are cleared above)
    if scaler is not None:
        # GradScaler.step / update (runner.py:686-690) for ONE scaler over the group's optimizers.  No short-circuit: each _found_inf
        # records the scale its model's backward used (what Adam divides by) and is a collective under expert parallelism
        found = [m._found_inf() for m in live]
        scaler.update(any(found))
        for m in models:
            m._loss_scale_tensor()            # the device copies follow (a captured step reads them on its next replay)
        if skip_together:
            live = () if any(found) else live
        else:
            live = [m for m, bad in zip(live, found) if not bad]
    for m, sc in zip(models, scale):
        if m not in live:
            if A > 1:
                m.accum.zero_()
            continue
        if scaler is not None:
            sc /= m._applied_loss_scale       # fp16: the gradient carries the loss scale
        if ok is not None:                    # the step count is the device's: it advances only where the flag lets the step through
            if A == 1:
                ops.adam_step_guarded(m.flat, m.grad, m.m, m.v, None, m._guard["step"], ok, m.lr, grad_scale=sc)
            else:
                ops.adam_accum_step_guarded(m.flat, m.accum, m.grad if fused else None, m.m, m.v, None, m._guard["step"], ok, m.lr,
                                            accum_scale=inv if fused else 1.0, grad_scale=sc)
            if refresh is None:
                m.refresh_compute_copies()        # (behind a dropped step it rewrites the copies with the values they hold)
            continue
        m.step_count += 1
        if A == 1:
            ops.adam_step(m.flat, m.grad, m.m, m.v, None, m.step_count, m.lr, grad_scale=sc)
        else:
            ops.adam_accum_step(m.flat, m.accum, m.grad if fused else None, m.m, m.v, None, m.step_count, m.lr,
                                accum_scale=inv if fused else 1.0, grad_scale=sc)
        if refresh is None:
            m.refresh_compute_copies()
    if live and refresh is not None:
        refresh()
    return bool(live)
