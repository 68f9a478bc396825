"""A/B of the expert weight-gradient launch of the no-drop step (capacity_factor = 0): swn_wgrad_multi over the packed groups (what the
cf = 0 step runs) against swn_wgrad_blocks (the batched launch of the static-capacity steps) over the same kept rows in the strided layout
(cf = E: capacity = the segment).  Same box, same batch, the launch replayed on the step's live buffers.

    python scripts/dyncap_wgrad_ab.py [--rays 2048] [--reps 20]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import synth  # noqa: E402
from switch_nerf_amd.model import SwitchNeRF  # noqa: E402


def time_wgrad(cf, rays, samples, chunk, reps):
    m = SwitchNeRF(synth.BUILDING, dtype=torch.bfloat16, capacity_factor=cf)
    m.load_state_dict(synth.make_weights(5, synth.BUILDING))
    m.profile = True
    r, img, rgb = (torch.from_numpy(a).cuda() for a in synth.make_rays(6, rays))
    st = m.train_step(rgb, r, img, samples, chunk, perturb=0.0, optimizer_step=False)
    fn = st["ctx"]["_relaunch"]["expert_wgrad"]
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    kept = int(st["ctx"]["counts"].clamp(max=st["ctx"]["cap"]).sum().item())
    return ts[len(ts) // 2], ts[0], kept


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--chunk", type=int, default=131072)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    E = synth.BUILDING["num_experts"]
    for name, cf in (("wgrad_multi, packed groups (cf = 0)", 0.0), ("wgrad_blocks, strided groups (cf = E)", float(E)),
                     ("wgrad_multi, packed groups (cf = 0), again", 0.0)):
        med, best, kept = time_wgrad(cf, a.rays, a.samples, a.chunk, a.reps)
        print(f"{name}: median {med:.3f} ms, best {best:.3f} ms over {a.reps} launches, {kept} kept rows")
        torch.cuda.empty_cache()
