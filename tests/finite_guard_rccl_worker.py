"""Launched by tests/test_finite_guard_gpu.py: ONE rank, backend nccl = RCCL, loopback (parallel.init_from_env(loopback=True)).  The
guarded step with the gradient all-reduce and the MIN all-reduce of the guard's flag issued for real must equal the guarded step
that issues no collective: poison, clean, poison, clean - flags, parameters, moments, step counts and skipped counters."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import synth  # noqa: E402
from switch_nerf_amd import parallel  # noqa: E402
from switch_nerf_amd.model import SwitchNeRF  # noqa: E402

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
parallel.init_from_env("nccl", dev, loopback=True)
allreduce = parallel.make_grad_allreduce(loopback=True)
assert allreduce.active
N, S = 64, 8
models = []
for _ in range(2):
    m = SwitchNeRF(synth.BUILDING, dtype=torch.bfloat16, device=dev)
    m.load_state_dict(synth.make_weights(41, synth.BUILDING))
    m.set_check_finite(True)
    models.append(m)
a, b = models
ok = True
for it in range(4):
    rays, img, rgbs = (torch.from_numpy(x).to(dev) for x in synth.make_rays(980 + it, N))
    if it % 2 == 0:
        rgbs[5, 0] = float("nan")
    ra = a.train_step(rgbs, rays, img, S, N * S, perturb=0.0, grad_allreduce=allreduce)
    rb = b.train_step(rgbs, rays, img, S, N * S, perturb=0.0)
    ok &= int(ra["step_ok"].item()) == int(rb["step_ok"].item()) == it % 2
    for k in ("flat", "m", "v"):
        ok &= bool(torch.equal(getattr(a, k), getattr(b, k)))
ok &= a.step_count == b.step_count == 2 and a.skipped_steps() == b.skipped_steps() == 2
ok &= bool(torch.isfinite(a.flat).all())
print(f"FINITE_GUARD_RCCL: {'OK' if ok else 'MISMATCH'}", flush=True)
torch.distributed.barrier()
torch.distributed.destroy_process_group()
sys.exit(0 if ok else 1)
