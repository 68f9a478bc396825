"""The training step of a scene with a background model, the measurements of profiles/r12_bg_graph.md: the eager compact step (the
default path), the eager padded step (bg_capacity = N) and the replayed padded step (graph.GraphedBackgroundStep, one capture with
bg_capacity = N for every batch) - plus a replay captured with bg_capacity = the batch's own n_bg, whose distance to the bg_capacity = N
replay is the GPU work the padding costs.  bf16, the scene's device noise on, perturb 1, noise std 1; 8192 x 256 and 1024 x 256; three
batches whose share of background rays is 0, half and all; one process, 8 rounds per batch with the order of the variants rotating.
Times are host clock around `reps` steps ending in a device synchronise.  Prints JSON lines.

    python scripts/bench_bg_graph.py [result.json] [--shapes 8192x256,1024x256] [--rounds 8]
"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch
import synth
from switch_nerf_amd.background import BackgroundScene
from switch_nerf_amd.dense import DenseNeRF
from switch_nerf_amd.graph import GraphedBackgroundStep
from switch_nerf_amd.model import SwitchNeRF

ap = argparse.ArgumentParser()
ap.add_argument("result", nargs="?")
ap.add_argument("--shapes", default="8192x256,1024x256")
ap.add_argument("--rounds", type=int, default=8)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_bg_graph.py needs a GPU"
def dev(a): return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def batch(N, share):
    """far = 0.3 ends inside the bound, far = 5 behind it (fg_far lies between ~0.45 and ~0.95 for these origins)."""
    rays, img, rgbs = synth.make_rays(11, N, far=0.3)
    n_far = {"none": 0, "half": N // 2, "all": N}[share]
    rays[np.random.default_rng(12).permutation(N)[:n_far], 7] = 5.0
    return dev(rgbs), dev(rays), dev(img)


out = {}
for shape in args.shapes.split(","):
    N, S = (int(v) for v in shape.split("x"))
    chunk, reps = min(131072, N * S), (5 if N * S > 1 << 20 else 20)
    fg = SwitchNeRF(synth.BUILDING, dtype=torch.bfloat16)
    fg.load_state_dict(synth.make_weights(1, synth.BUILDING))
    bg = DenseNeRF(synth.DENSE_BG, dtype=torch.bfloat16)
    bg.load_state_dict(synth.make_dense_weights(2, synth.DENSE_BG))
    scene = BackgroundScene(fg, bg, synth.SPHERE_CENTER, synth.SPHERE_RADIUS)
    scene.set_device_noise(2024)
    batches = {share: batch(N, share) for share in ("none", "half", "all")}
    replay_full = GraphedBackgroundStep(scene, *batches["half"], S, chunk, perturb=1.0, noise_std=1.0)        # ONE capture, bg_capacity = N
    for share, b in batches.items():
        n_bg = int(scene.train_step(*b, S, chunk, perturb=1.0, noise_std=1.0)["ctx"]["Nb"])
        replay_fit = GraphedBackgroundStep(scene, *b, S, chunk, perturb=1.0, noise_std=1.0, bg_capacity=max(1, n_bg))
        variants = {
            "compact_eager": lambda: scene.train_step(*b, S, chunk, perturb=1.0, noise_std=1.0),
            "padded_eager": lambda: scene.train_step(*b, S, chunk, perturb=1.0, noise_std=1.0, bg_capacity=N),
            "padded_replay": lambda: replay_full(*b),
            "fitted_replay": lambda: replay_fit(*b),
        }
        names = list(variants)
        times = {k: [] for k in names}
        for rnd in range(args.rounds):
            for k in names[rnd % 4:] + names[:rnd % 4]:
                for _ in range(2): variants[k]()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps): variants[k]()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) / reps * 1e3)
        rec = dict(n_bg=n_bg, reps=reps)
        for k in names:
            rec[k + "_ms"] = [round(t, 4) for t in times[k]]
            rec[k + "_ms_median"] = float(np.median(times[k]))
        rec["replay_over_compact"] = rec["padded_replay_ms_median"] / rec["compact_eager_ms_median"]
        rec["padding_gpu_ms"] = rec["padded_replay_ms_median"] - rec["fitted_replay_ms_median"]
        out[f"{shape}_{share}"] = rec
        print(json.dumps({f"{shape}_{share}": rec}), flush=True)
        del replay_fit, variants
    del replay_full, scene, fg, bg
if args.result:
    json.dump(out, open(args.result, "w"), indent=1)
