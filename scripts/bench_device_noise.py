"""Seeded device noise, the measurements of profiles/r08_device_noise.md: swn_rng_fill at 2,097,152 elements against the framework's
in-place draws, and the default benchmark config's graphed step with device noise on against off in ONE process (8 rounds of 20 replays,
order alternating per round).  Prints JSON lines; `fill-only` as first argument stops after the fill timing.
`bg` (profiles/r09_bg_device_noise.md): BackgroundScene.train_step (eager; perturb 1, noise std 1, synth.make_bg_rays) with the scene's
device noise on against off - off draws the same noise from the framework generator, as rendering.render_rays does - at 64 rays x 16
samples and at 8192 x 256, one process, 8 alternating rounds per shape; and swn_rng_fill_rows against swn_rng_fill at one size.

    python scripts/bench_device_noise.py [fill-only | all [result.json] | bg [result.json]]
"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch
import synth
from switch_nerf_amd import ops
from switch_nerf_amd.model import SwitchNeRF
from switch_nerf_amd.graph import GraphedTrainStep

out = {}
def dev(a): return torch.from_numpy(np.ascontiguousarray(a)).cuda()
def ev_time(fn, iters):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / iters

def bench_bg(path):
    from switch_nerf_amd.background import BackgroundScene
    from switch_nerf_amd.dense import DenseNeRF
    st = ops.rng_step_tensor(0, "cuda")
    n_rows, per_row = 4096, 128                       # about the background draw of the full batch: half the rays x 128 samples
    idx = torch.randperm(8192, device="cuda")[:n_rows].contiguous()
    buf = torch.empty(n_rows, per_row, device="cuda")
    for kind, name in ((0, "uniform"), (1, "normal")):
        out[f"fill_rows_{name}_us"] = 1e3 * ev_time(lambda: ops.rng_fill_rows(n_rows, per_row, 0, idx, kind, 1234, st, 1, 1, 1.0, 8192, out=buf), 200)
        out[f"fill_{name}_us"] = 1e3 * ev_time(lambda: ops.rng_fill(n_rows * per_row, 0, kind, 1234, st, 1, out=buf.view(-1)), 200)
    print(json.dumps(out), flush=True)
    for N, S, chunk, reps in ((64, 16, 1024, 20), (8192, 256, 131072, 5)):
        rays, img, rgbs = (dev(a) for a in synth.make_bg_rays(1, N))
        fg = SwitchNeRF(synth.BUILDING, dtype=torch.bfloat16)
        fg.load_state_dict(synth.make_weights(1, synth.BUILDING))
        bg = DenseNeRF(synth.DENSE_BG, dtype=torch.bfloat16)
        bg.load_state_dict(synth.make_dense_weights(2, synth.DENSE_BG))
        scene = BackgroundScene(fg, bg, synth.SPHERE_CENTER, synth.SPHERE_RADIUS)

        def step(on):
            kw = {} if on else dict(sigma_noise=torch.randn(N * S, device="cuda"), sigma_noise_bg="randn")
            return scene.train_step(rgbs, rays, img, S, chunk, perturb=1.0, noise_std=1.0, **kw)
        times = {"off": [], "on": []}
        for rnd in range(8):
            for k in (("off", "on") if rnd % 2 == 0 else ("on", "off")):
                scene.set_device_noise(None if k == "off" else 2024, step=rnd * 100)
                for _ in range(2): r = step(k == "on")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps): r = step(k == "on")
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) / reps * 1e3)
        tag = f"{N}x{S}"
        out[f"bg_{tag}_n_bg"] = int(r["ctx"]["Nb"])
        for k in times:
            out[f"bg_step_ms_{k}_{tag}"] = times[k]
            out[f"bg_step_ms_{k}_{tag}_median"] = float(np.median(times[k]))
        out[f"bg_step_ms_diff_{tag}_median"] = float(np.median(np.array(times["on"]) - np.array(times["off"])))
        print(json.dumps(out), flush=True)
        del scene, fg, bg
    if path:
        json.dump(out, open(path, "w"), indent=1)


if len(sys.argv) > 1 and sys.argv[1] == "bg":
    bench_bg(sys.argv[2] if len(sys.argv) > 2 else None)
    sys.exit(0)

n = 2097152
st = ops.rng_step_tensor(0, "cuda")
buf = torch.empty(n, device="cuda")
for kind, name in ((0, "uniform"), (1, "normal")):
    out[f"fill_{name}_us"] = 1e3 * ev_time(lambda: ops.rng_fill(n, 0, kind, 1234, st, 1, out=buf), 200)
out["torch_rand_us"] = 1e3 * ev_time(lambda: torch.rand(n, device="cuda", out=buf) if False else buf.uniform_(), 200)
out["torch_randn_us"] = 1e3 * ev_time(lambda: buf.normal_(), 200)
print(json.dumps(out), flush=True)

if len(sys.argv) > 1 and sys.argv[1] == "fill-only":
    sys.exit(0)
N, S, chunk = 8192, 256, 131072
rays, img, rgbs = (dev(a) for a in synth.make_rays(1, N))
model = SwitchNeRF(synth.BUILDING, dtype=torch.bfloat16)
model.load_state_dict(synth.make_weights(1, synth.BUILDING))
steps = {}
model.set_device_noise(None)
steps["off"] = GraphedTrainStep(model, rgbs, rays, img, S, chunk, perturb=1.0, noise_std=1.0)
model.set_device_noise(2024)
steps["on"] = GraphedTrainStep(model, rgbs, rays, img, S, chunk, perturb=1.0, noise_std=1.0)
times = {"off": [], "on": []}
for rnd in range(8):                      # interleaved A/B rounds in one process, order alternating (off on / on off)
    for k in (("off", "on") if rnd % 2 == 0 else ("on", "off")):
        model.set_device_noise(None if k == "off" else 2024, step=rnd * 100)
        g = steps[k]
        for _ in range(3): g()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20): g()
        torch.cuda.synchronize()
        times[k].append((time.perf_counter() - t0) / 20 * 1e3)
out["step_ms_off"] = times["off"]; out["step_ms_on"] = times["on"]
out["step_ms_off_median"] = float(np.median(times["off"])); out["step_ms_on_median"] = float(np.median(times["on"]))
print(json.dumps(out), flush=True)
if len(sys.argv) > 2:
    json.dump(out, open(sys.argv[2], "w"), indent=1)
