"""Training a Mega-NeRF whose cells use spherical-harmonics colour (switch_nerf_amd/mega.py, joint_training + sh_training), the
measurements of profiles/r17_mega_sh_train.md: degrees 0, 2 and 4 at 8192 x 256 and 1024 x 256 points, bf16, 4 cells of the DENSE
configuration without a direction block (centroids on a square: balanced cells), hard margin, perturbation and sigma noise supplied.

  ms per step     MegaNeRF.train_step with sh cells against the same batch through 4 plain-colour cells (joint_training alone, what the
                  model trained before this path existed).  Host clock around steps that end in a device synchronise, alternating
                  windows; the median of 3 windows of 3 steps after 2 warm-up steps each.
  per kernel      device events, median of 5 windows of 20 calls, on one cell's share of the rows (P / 4): swn_heads_coef_fwd,
                  swn_heads_coef_bwd (its launches together) and, on all packed rows, swn_cells_blend_sh_bwd.
  folded heads    the same head rows through the existing swn_heads_sh_fwd / swn_heads_sh_bwd at rows_per_group = 1 (what gluing the two
                  existing halves together would run), and both backward workspaces in bytes.

    python scripts/mega_sh_train_timing.py [result.json] [--only-rays N]
"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch

import synth
from switch_nerf_amd import _lib, ops
from switch_nerf_amd.dense import DENSE, DenseNeRF
from switch_nerf_amd.mega import MegaNeRF

K = 4
CEN = np.array([[sx, sy, 0.0] for sx in (-0.4, 0.4) for sy in (-0.4, 0.4)], np.float32)


def window(step, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def ev_time(fn, iters=20, windows=5):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / iters * 1e3)
    return float(np.median(ts))             # microseconds per call


def steps(N, S, deg, dev="cuda"):
    cfg = dict(DENSE, pos_dir_dim=0, sh_deg=deg)
    rays, img, rgbs = (torch.from_numpy(a).to(dev) for a in synth.make_rays(5, N, DENSE["appearance_count"]))
    g = torch.Generator(device=dev).manual_seed(1)
    pr, noise = torch.rand(N, S, device=dev, generator=g), torch.randn(N * S, device=dev, generator=g)
    sh = MegaNeRF([DenseNeRF(cfg, dtype=torch.bfloat16, seed=10 + i) for i in range(K)], CEN, 1.0, False, False, joint_training=True,
                  sh_training=True)
    plain = MegaNeRF([DenseNeRF(DENSE, dtype=torch.bfloat16, seed=10 + i) for i in range(K)], CEN, 1.0, False, False, joint_training=True)
    run = {k: (lambda m=m: m.train_step(rgbs, rays, img, S, perturb=1.0, perturb_rand=pr, sigma_noise=noise)) for k, m in (("sh", sh), ("plain", plain))}
    for _ in range(2):
        st = run["sh"]()
        run["plain"]()
    ms = dict(sh=[], plain=[])
    for _ in range(3):
        for k in ms:
            ms[k].append(window(run[k], 3))
    return dict(members_per_cell=st["ctx"]["counts"], ms_per_step={k: dict(median=float(np.median(v)), min=min(v), max=max(v)) for k, v in ms.items()})


def kernels(P, deg, dev="cuda"):
    n, M, H2, B = P // K, DENSE["layer_dim"], DENSE["layer_dim"] // 2, (deg + 1) ** 2
    g = torch.Generator(device=dev).manual_seed(2)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    y, h2 = r(n, M).relu().bfloat16(), r(n, H2).relu().bfloat16()
    ws, bs, wc, bc = r(M) / 16, r(1), r(3 * B, H2) / 8, r(3 * B)
    dirs, q, d_raw = r(n, 3), r(n, 4), r(n, 4)
    rows_out = torch.empty(n, 3 * B + 1, device=dev)
    gr = [torch.zeros(s, device=dev) for s in ((M,), (1,), (3 * B, H2), (3 * B,))]
    out = {}
    out["heads_coef_fwd_us"] = ev_time(lambda: ops.heads_coef_fwd(y, h2, ws, bs, wc, bc, None, deg, rows_out, deg == 0))
    out["heads_coef_bwd_us"] = ev_time(lambda: ops.heads_coef_bwd(y, h2, wc, q, dirs, rows_out, *gr, deg))
    out["heads_coef_bwd_workspace_bytes"] = ops.heads_coef_bwd_workspace_bytes(n, M, H2, deg)
    nb = C.c_size_t(0)
    _lib.call("swn_heads_sh_bwd_workspace_bytes", n, M, H2, 1, deg, C.byref(nb))
    out["folded_bwd_workspace_bytes_cell"] = int(nb.value)
    _lib.call("swn_heads_sh_bwd_workspace_bytes", P, M, H2, 1, deg, C.byref(nb))
    out["folded_bwd_workspace_bytes_all_rows"] = int(nb.value)
    raw = ops.heads_sh_fwd(y, h2, ws, bs, wc, bc, None, dirs, 1, deg)
    out["folded_fwd_rpg1_us"] = ev_time(lambda: ops.heads_sh_fwd(y, h2, ws, bs, wc, bc, None, dirs, 1, deg), iters=5, windows=3)
    out["folded_bwd_rpg1_us"] = ev_time(lambda: ops.heads_sh_bwd(y, h2, wc, bc, dirs, raw, d_raw, *gr, 1, deg), iters=5, windows=3)
    # the blend's adjoint on every packed row (hard margin: total = P)
    x = torch.cat([torch.rand(P, 3, device=dev, generator=g) * 2 - 1, torch.zeros(P, 1, device=dev)], 1)
    w, counts = ops.cells_assign(x, torch.from_numpy(CEN).to(dev), 0, 1.0)
    begin, rows, slot = ops.cells_pack(w, counts, P)
    raw4, d4, dd = torch.rand(P, 4, device=dev, generator=g), r(P, 4), r(P // 256, 3)
    sub = torch.rand(P, 4, device=dev, generator=g) if deg == 0 else None
    out["cells_blend_sh_bwd_us"] = ev_time(lambda: ops.cells_blend_sh_bwd(w, rows, begin, raw4, d4, dd, 256, deg, P, True, sub))
    out["head_rows"], out["packed_rows"] = n, P
    return out


def main():
    out_path = next((a for a in sys.argv[1:] if a.endswith(".json")), None)
    only = int(sys.argv[sys.argv.index("--only-rays") + 1]) if "--only-rays" in sys.argv else None
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, cells=K, dtype="bf16", cfg="DENSE, pos_dir_dim 0", cases=[])
    for N in (8192, 1024):
        if only is not None and N != only:
            continue
        for deg in (0, 2, 4):
            c = dict(rays=N, samples=256, deg=deg)
            c.update(steps(N, 256, deg))
            c["kernels"] = kernels(N * 256, deg)
            res["cases"].append(c)
            print(json.dumps(c), flush=True)
            torch.cuda.empty_cache()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
