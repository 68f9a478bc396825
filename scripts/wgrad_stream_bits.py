"""SHA-256 of dW and db of the three launches scripts/wgrad_stream_timing.py times (same shapes, seeded random operands, one launch
each into zeroed outputs): run it once per build of the library (SWN_LIB=...) and compare the lines - equal digests = equal bits."""
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from switch_nerf_amd import ops as o  # noqa: E402

dev, dt = torch.device("cuda"), torch.bfloat16
torch.manual_seed(0)
mk = lambda rows, cols: torch.randn(rows, cols, device=dev).to(dt)  # noqa: E731
z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731


def digest(jobs):
    torch.cuda.synchronize()
    h, n = hashlib.sha256(), 0
    for j in jobs:
        for t in (j[2], j[3]):
            if t is not None:
                h.update(t.cpu().numpy().tobytes())
                n += t.numel()
    return {"values": n, "sha256": h.hexdigest()}


M, E, L, CAP, NSEG = 256, 8, 7, 16384, 16
NG, ROWS = NSEG * E, NSEG * E * CAP
perm = torch.randperm(ROWS, device=dev).int()
jobs = [(mk(ROWS, M), mk(ROWS, M), z(E, M, M), z(E, M), perm if l == 0 else None, perm if l == L - 1 else None) for l in range(L)]
counts = torch.tensor(([CAP] * 3 + [int(CAP * 0.664)] * 5) * NSEG, dtype=torch.int32, device=dev)
o.wgrad_multi(jobs, n_groups=NG, n_wsets=E, group_stride=CAP, group_rows=counts, group_rows_clamp=CAP, tag=1)
print(json.dumps({"launch": "expert", **digest(jobs)}))
del jobs
torch.cuda.empty_cache()

P, KP, H2 = 8192 * 256, 128, 128
tail = [(mk(P, M), mk(P, H2), z(1, M, H2), None, None, None), (mk(P, M), mk(P, M), z(1, M, M), z(1, M), None, None)]
o.wgrad_multi(tail)
print(json.dumps({"launch": "dense_tail", **digest(tail)}))
del tail
torch.cuda.empty_cache()
front = [(mk(P, M), mk(P, M), z(1, M, M), z(1, M), None, None), (mk(P, M), mk(P, M), z(1, M, M), z(1, M), None, None),
         (mk(P, KP), mk(P, M), z(1, KP, M), z(1, M), None, None)]
o.wgrad_multi(front)
print(json.dumps({"launch": "dense_front", **digest(front)}))
