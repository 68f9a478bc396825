"""What gradient accumulation (SwitchNeRF.set_accumulation) costs at the benchmark shape, on one GPU, in one process, the variants
interleaved round by round (profiles/r20_accum.md):

  step level (eager train_step, device events around each call, 8192 rays x 256 samples, bf16):
    plain_nostep   A = 1, train_step(optimizer_step=False)          the step without accumulation that drops its gradient
    accum_micro    A = 2, an accumulating micro-step                = plain_nostep + one swn_grad_accum
    plain_step     A = 1, train_step()                              the plain step: swn_adam_step + refresh
    fused_last     A = 2, the window's last micro-step              swn_adam_accum_step + refresh
    unfused_last   A = 2, the last micro-step with a grad_allreduce swn_grad_accum + (all-reduce: a no-op here) + swn_adam_accum_step + refresh
  kernel level (the launches alone on the model's flat buffers, back to back):
    grad_accum, adam_step, adam_accum_step (with and without the last gradient)

With A = 1 the code path is the one without the feature, so plain_nostep / plain_step are the baselines measured in the same process.

    python scripts/accum_timing.py [--rays 8192 --samples 256 --rounds 30 --out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import synth  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def summary(xs):
    xs = sorted(xs)
    return dict(median_ms=statistics.median(xs), min_ms=xs[0], p90_ms=xs[int(0.9 * (len(xs) - 1))], max_ms=xs[-1], n=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--chunk", type=int, default=131072)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "accum_timing.py measures on the GPU"
    from switch_nerf_amd import ops
    from switch_nerf_amd.model import SwitchNeRF, BUILDING
    dev = torch.device("cuda:0")
    rays, img, rgbs = (torch.from_numpy(t).to(dev) for t in synth.make_rays(1000, a.rays))
    chunk = min(a.chunk, a.rays * a.samples)
    plain = SwitchNeRF(BUILDING, dtype=torch.bfloat16, device=dev, seed=0)
    accum = SwitchNeRF(BUILDING, dtype=torch.bfloat16, device=dev, seed=0)
    accum.set_accumulation(2)
    one = lambda v: 1.0
    step = lambda m, **kw: m.train_step(rgbs, rays, img, a.samples, chunk, perturb=0.0, **kw)
    variants = {
        "plain_nostep": lambda: step(plain, optimizer_step=False),
        "accum_micro": lambda: step(accum, should_accumulate=True),
        "plain_step": lambda: step(plain),
        "fused_last": lambda: step(accum, should_accumulate=False),
        "unfused_last": lambda: step(accum, should_accumulate=False, grad_allreduce=one),
    }
    m = accum
    kernels = {
        "grad_accum": lambda: ops.grad_accum(m.accum, m.grad, 0.5),
        "adam_step": lambda: ops.adam_step(m.flat, m.grad, m.m, m.v, None, 3, 0.0),
        "adam_accum_step": lambda: ops.adam_accum_step(m.flat, m.accum, m.grad, m.m, m.v, None, 3, 0.0, accum_scale=0.5),
        "adam_accum_step_nograd": lambda: ops.adam_accum_step(m.flat, m.accum, None, m.m, m.v, None, 3, 0.0),
    }
    for _ in range(a.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in list(variants) + list(kernels)}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            times[k].append(timed(fn))
    for _ in range(a.rounds):                 # (lr 0: the parameters stay put while the launches are timed, 20 per sample)
        for k, fn in kernels.items():
            times[k].append(timed(lambda: [fn() for _ in range(20)]) / 20)
    res = dict(rays=a.rays, samples=a.samples, chunk=chunk, dtype="bf16", rounds=a.rounds, n_flat=int(plain.n_flat),
               grad_bytes=int(plain.n_flat) * 4, device=torch.cuda.get_device_name(0), **{k: summary(v) for k, v in times.items()})
    med = lambda k: res[k]["median_ms"]
    res["delta_ms"] = dict(accum_micro_minus_plain_nostep=med("accum_micro") - med("plain_nostep"),
                           fused_last_minus_plain_step=med("fused_last") - med("plain_step"),
                           unfused_last_minus_fused_last=med("unfused_last") - med("fused_last"))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
