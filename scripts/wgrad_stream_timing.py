"""Time the balanced weight-gradient stream launch (ops.wgrad_multi -> swn_wgrad_multi) at the step's shapes: the 7 expert layers
(256 x 256, 16 segments x 8 experts of capacity 16384, router-like fill, first layer's A and last layer's B read through the routing
permutation) and the two dense launches (2,097,152 points: the tail's 2 jobs, the front's 3).  HIP events around 5 back-to-back
launches, best of 3 repeats.
  python scripts/wgrad_stream_timing.py            random operands
  ZERO=1 python scripts/wgrad_stream_timing.py     all-zero operands (nothing toggles in the matrix pipe)
  SWN_LIB=switch_nerf_amd/libswn_hip_<variant>.so  another build of the library (A/B on one device)"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from switch_nerf_amd import ops as o  # noqa: E402

dev, dt = torch.device("cuda"), torch.bfloat16
zero = bool(os.environ.get("ZERO"))
torch.manual_seed(0)


def mk(rows, cols):
    return torch.zeros(rows, cols, device=dev, dtype=dt) if zero else torch.randn(rows, cols, device=dev).to(dt)


def timed(f, reps=3, n=5):
    f()
    f()
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            f()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b) / n
        best = ms if best is None else min(best, ms)
    return best


# ---- expert launch
M, E, L, CAP, NSEG = 256, 8, 7, 16384, 16
NG, ROWS = NSEG * E, NSEG * E * CAP
acts = [mk(ROWS, M) for _ in range(L)]
dzs = [mk(ROWS, M) for _ in range(L)]
perm = torch.randperm(ROWS, device=dev).int()
dw = [torch.zeros(E, M, M, device=dev) for _ in range(L)]
db = [torch.zeros(E, M, device=dev) for _ in range(L)]
jobs = [(acts[l], dzs[l], dw[l], db[l], perm if l == 0 else None, perm if l == L - 1 else None) for l in range(L)]
counts = torch.tensor(([CAP] * 3 + [int(CAP * 0.664)] * 5) * NSEG, dtype=torch.int32, device=dev)
kept = int(counts.sum())
ms = timed(lambda: o.wgrad_multi(jobs, n_groups=NG, n_wsets=E, group_stride=CAP, group_rows=counts, group_rows_clamp=CAP, tag=1))
nbytes = kept * L * (M + M) * 2
print(json.dumps({"launch": "expert", "zero": zero, "ms": round(ms, 4), "TBps": round(nbytes / ms / 1e9, 3)}))
del acts, dzs, dw, db, jobs
torch.cuda.empty_cache()

# ---- dense launches (model.py: the tail's and the front's weight gradients, one launch each)
P, KP, H2 = 8192 * 256, 128, 128
z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
tail = [(mk(P, M), mk(P, H2), z(1, M, H2), None), (mk(P, M), mk(P, M), z(1, M, M), z(1, M))]
front = [(mk(P, M), mk(P, M), z(1, M, M), z(1, M)), (mk(P, M), mk(P, M), z(1, M, M), z(1, M)), (mk(P, KP), mk(P, M), z(1, KP, M), z(1, M))]
for name, js in (("dense_tail", tail), ("dense_front", front)):
    items = [(a, b, w, bb, None, None) for a, b, w, bb in js]
    ms = timed(lambda: o.wgrad_multi(items))
    nbytes = sum((a.shape[1] + b.shape[1]) * 2 * P for a, b, _w, _b in js)
    print(json.dumps({"launch": name, "zero": zero, "ms": round(ms, 4), "TBps": round(nbytes / ms / 1e9, 3)}))
