"""What affine_appearance costs (profiles/r10_affine_appearance.md): the graphed training step at the bench shape (8192 rays x 256 samples,
bf16) of three models in ONE process - the affine model, (a) the default model with fused_heads off (the same unfused tail and separate
heads launches, no transform), (b) the default fused step - in 6 interleaved rounds of 10 replays, the order rotating per round; then the
two new per-point launches (swn_heads_affine_fwd / swn_heads_affine_bwd) and their plain siblings alone at 2,097,152 points as time and
HBM bytes / time.  Prints JSON lines.

    python scripts/affine_cost.py [result.json]
"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch
import synth
import affine_weights as aw
from switch_nerf_amd import ops
from switch_nerf_amd.model import SwitchNeRF
from switch_nerf_amd.graph import GraphedTrainStep

out = {}
def dev(a): return torch.from_numpy(np.ascontiguousarray(a)).cuda()
def ev_time(fn, iters):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / iters

# ---- the two per-point launches alone
N, S, M, H2 = 8192, 256, 256, 128
P = N * S
g = torch.Generator(device="cuda").manual_seed(1)
y = torch.relu(torch.randn(P, M, device="cuda", generator=g)).bfloat16()
h2 = torch.relu(torch.randn(P, H2, device="cuda", generator=g)).bfloat16()
ws, bs = torch.randn(M, device="cuda", generator=g) / 16, torch.zeros(1, device="cuda")
wc, bc = torch.randn(3, H2, device="cuda", generator=g) / 11, torch.zeros(3, device="cuda")
T = torch.eye(3, 4, device="cuda").reshape(1, 12).repeat(N, 1) + 0.1 * torch.randn(N, 12, device="cuda", generator=g)
d_raw = torch.randn(P, 4, device="cuda", generator=g)
acc = [torch.zeros(M, device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(3, H2, device="cuda"), torch.zeros(3, device="cuda")]
raw = ops.heads_affine_fwd(y, h2, ws, bs, wc, bc, None, T, S)
fwd_bytes = P * (2 * M + 2 * H2 + 16)                       # y + h2 read, raw written
bwd_bytes = P * (2 * M + 2 * H2 + 16 + 16 + 2 * H2 + 4)     # y + h2 + raw + d_raw read, dh2 + dsig written
for name, fn, nbytes in (("heads_affine_fwd", lambda: ops.heads_affine_fwd(y, h2, ws, bs, wc, bc, None, T, S), fwd_bytes),
                         ("heads_fwd", lambda: ops.heads_fwd(y, h2, ws, bs, wc, bc, None), fwd_bytes),
                         ("heads_affine_bwd", lambda: ops.heads_affine_bwd(y, h2, wc, bc, T, raw, d_raw, *acc, rows_per_group=S), bwd_bytes),
                         ("heads_bwd", lambda: ops.heads_bwd(y, h2, wc, raw, d_raw, *acc, rows_per_group=S), bwd_bytes)):
    ms = ev_time(fn, 20)
    out[name + "_us"] = 1e3 * ms
    out[name + "_TBps"] = nbytes / (ms * 1e-3) / 1e12
print(json.dumps(out), flush=True)
del y, h2, raw, d_raw

# ---- the graphed step of the three models
chunk = 131072
rays, img, rgbs = (dev(a) for a in synth.make_rays(1, N))
models = {"affine": SwitchNeRF(aw.affine_cfg(), dtype=torch.bfloat16),
          "unfused_heads": SwitchNeRF(synth.BUILDING, dtype=torch.bfloat16, kernel_switches=dict(fused_heads=False)),
          "default": SwitchNeRF(synth.BUILDING, dtype=torch.bfloat16)}
models["affine"].load_state_dict(aw.make_affine_weights(1))
for k in ("unfused_heads", "default"):
    models[k].load_state_dict(synth.make_weights(1, synth.BUILDING))
steps = {k: GraphedTrainStep(m, rgbs, rays, img, S, chunk, perturb=1.0, noise_std=1.0) for k, m in models.items()}
out["kernel_set"] = {k: {q: v for q, v in m.kernel_set().items() if q != "env_overrides"} for k, m in models.items()}
names = list(steps)
times = {k: [] for k in names}
for rnd in range(6):
    for k in names[rnd % 3:] + names[: rnd % 3]:
        s = steps[k]
        for _ in range(3): s()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10): s()
        torch.cuda.synchronize()
        times[k].append((time.perf_counter() - t0) / 10 * 1e3)
for k in names:
    out[f"step_ms_{k}"] = times[k]
    out[f"step_ms_{k}_median"] = float(np.median(times[k]))
out["transform_price_ms"] = out["step_ms_affine_median"] - out["step_ms_unfused_heads_median"]
out["unfused_price_ms"] = out["step_ms_affine_median"] - out["step_ms_default_median"]
print(json.dumps(out), flush=True)
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
