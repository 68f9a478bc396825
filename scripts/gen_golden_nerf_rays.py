"""Fixture of the NeRF-dataset rays (switch_nerf_amd/nerf_rays.py over csrc/raygen_nerf.hip) from the REFERENCE's own
datasets/nerf_data: ray_utils.get_rays / ndc_rays and load_bungee.get_bungee_nearfar_radii, on the CPU.

Usage (build container only, like scripts/gen_golden_raygen.py: the reference is not on the GPU box):
    python scripts/gen_golden_nerf_rays.py

Input dtype.  nerf_loader.py:104 makes the poses with torch.tensor(poses): float32 for Blender and LLFF (their loaders end in
.astype(np.float32)), float64 for the bungee scenes (load_bungee.py:29 reads them from JSON and never casts).  K (:120) is float32
with an LLFF focal (np.float32) and float64 with a Blender / bungee one (np.float64), but get_rays uses it only through 0-dim
elements, which leave the float32 pixel grid float32.  So a float32 pose keeps the whole chain float32; a float64 pose promotes it from
the rotation on, and nerf_loader.py:175 rounds the result to float32 at the very end.  Three copies are written:
    (no prefix)  float32 K and poses: what Blender / LLFF run, and the arithmetic the device kernels restate
    f64_         float64 K, poses AND pixel grid (torch's default dtype set to float64): the mathematics, the yardstick of the tests
    ld_          bungee only: float64 poses over the float32 pixel grid, rounded to float32 at the end - what the bungee loader runs
focal is handed to ndc_rays as a Python float, so that -1 / (W / (2 focal)) is formed in double as the kernels' host side forms it.

Writes tests/golden/nerf_rays.npz, data only:
    cams (names); per camera <cam>_W, _H, _K [3, 3], _c2w [3, 4] (fp32-representable), _focal, _near, _far
    scene_scaling_factor, scene_origin [3], near_ndc
    [f64_]<cam>_rays_o / _rays_d [H, W, 3]          get_rays
    [f64_]<cam>_dn [H, W, 3]                        rays_d / norm (nerf_loader.py:160)
    [f64_]<cam>_ndc_o / _ndc_d [H, W, 3]            ndc_rays(H, W, focal, near_ndc, rays_o, rays_d)
    [f64_|ld_]<cam>_{sphere,flat}_rays [H, W, 8], _radii [H, W, 1]     get_bungee_nearfar_radii
Before it writes, the generator checks that every reference output is finite, that both discriminants of the sphere form are positive,
that every ray descends (flat; the camera b7x4 stands above z = 250, where the reference's flat near is not clamped, the others show
the clamp) and that |d_z| >= 0.3 |d| (NDC).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("SWN_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(REF, "switch_nerf", "datasets", "nerf_data"))
for missing in ("cv2", "imageio"):          # load_bungee imports them for its image reading; the ray functions use neither
    try:
        __import__(missing)
    except ImportError:
        sys.modules[missing] = types.ModuleType(missing)
import ray_utils as ref  # noqa: E402  (the modules alone: the package's __init__ pulls in the whole trainer)
import load_bungee as ref_bungee  # noqa: E402
import nerf_rays_restate as restate  # noqa: E402

SCALE = 2e-4                                      # scene_scaling_factor: 1 unit = 5 km
ORIGIN = np.array([30.0, -20.0, -6371011.0])      # scene_origin: the globe's centre lies one earth radius below the scene
NEAR_NDC = 1.0
NEAR, FAR = 2.0, 6.0


def look(origin, forward, roll):
    """c2w [3, 4] (fp32-representable float64) of a camera at `origin` looking along `forward` (z up; the camera looks along its -z)."""
    f = np.asarray(forward, np.float64)
    f = f / np.linalg.norm(f)
    r = np.cross(f, np.array([0.0, 0.0, 1.0]) if abs(f[2]) < 0.99 else np.array([0.0, 1.0, 0.0]))
    r = r / np.linalg.norm(r)
    u = np.cross(r, f)
    c, s = np.cos(roll), np.sin(roll)
    r, u = c * r + s * u, c * u - s * r
    m = np.concatenate([np.stack([r, u, -f], 1), np.asarray(origin, np.float64)[:, None]], 1)
    return m.astype(np.float32).astype(np.float64)


def intrinsics(fx, fy, cx, cy):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)


CAMS = [  # name, W, H, K (fx != fy, principal point off-centre), c2w (a general rotation, looking down), focal of ndc_rays
    ("a5x3", 5, 3, intrinsics(6.5, 7.25, 2.25, 1.75), look([0.10, -0.20, 0.50], [0.20, 0.10, -1.0], 0.30), 6.5),
    ("b7x4", 7, 4, intrinsics(9.0, 8.5, 3.75, 1.625), look([-0.30, 0.15, 300.0], [-0.15, 0.25, -1.0], -0.70), 9.0),
    ("c4x2", 4, 2, intrinsics(5.25, 4.75, 1.5, 1.25), look([0.05, 0.40, 0.35], [0.10, -0.20, -1.0], 1.20), 5.25),
    ("d37x29", 37, 29, intrinsics(40.0, 43.5, 17.25, 15.625), look([0.20, -0.10, 0.60], [-0.25, 0.15, -1.0], 0.45), 41.0),
]


def run(W, H, K, c2w, focal, tdtype, default):
    """The reference's chain for one camera with K, c2w of dtype `tdtype` under the default dtype `default` -> numpy arrays."""
    torch.set_default_dtype(default)
    try:
        Kt, pose = torch.tensor(K, dtype=tdtype), torch.tensor(c2w, dtype=tdtype)
        o, d = ref.get_rays(H, W, Kt, pose)
        dn = d / torch.norm(d, dim=-1, keepdim=True)                        # nerf_loader.py:160
        no, nd = ref.ndc_rays(H, W, float(focal), NEAR_NDC, o, d)           # nerf_loader.py:158
        out = dict(rays_o=o, rays_d=d, dn=dn, ndc_o=no, ndc_d=nd)
        rays6 = torch.cat([o, dn], -1)[None]                                # [1, H, W, 6]: nerf_loader.py:161-162
        for kind in ("sphere", "flat"):
            r, rad = ref_bungee.get_bungee_nearfar_radii(rays=rays6, scene_scaling_factor=SCALE, scene_origin=ORIGIN, ray_nearfar=kind)
            out[f"{kind}_rays"], out[f"{kind}_radii"] = r[0], rad[0]
        return {k: v.contiguous().numpy() for k, v in out.items()}
    finally:
        torch.set_default_dtype(torch.float32)


def main():
    torch.set_num_threads(1)
    out = dict(cams=np.array([c[0] for c in CAMS]), scene_scaling_factor=np.float64(SCALE), scene_origin=ORIGIN,
               near_ndc=np.float64(NEAR_NDC))
    for name, W, H, K, c2w, focal in CAMS:
        out.update({f"{name}_W": np.int32(W), f"{name}_H": np.int32(H), f"{name}_K": K.astype(np.float32),
                    f"{name}_c2w": c2w.astype(np.float32), f"{name}_focal": np.float64(focal), f"{name}_near": np.float64(NEAR),
                    f"{name}_far": np.float64(FAR)})
        assert np.array_equal(K.astype(np.float32).astype(np.float64), K)
        f32 = run(W, H, K, c2w, focal, torch.float32, torch.float32)
        f64 = run(W, H, K, c2w, focal, torch.float64, torch.float64)
        ld = run(W, H, K, c2w, focal, torch.float64, torch.float32)
        for k, v in f32.items():
            assert v.dtype == np.float32, (name, k, v.dtype)
        for k, v in f64.items():
            assert v.dtype == np.float64, (name, k, v.dtype)
        assert ld["rays_d"].dtype == np.float64                  # a float64 pose promotes the chain
        for tag, res in (("", f32), ("f64_", f64), ("ld_", ld)):
            for k, v in res.items():
                assert np.isfinite(v).all(), (tag, name, k)          # the inputs keep the reference itself finite
                if tag != "ld_":
                    out[f"{tag}{name}_{k}"] = v
                elif k.startswith(("sphere", "flat")):
                    out[f"{tag}{name}_{k}"] = v.astype(np.float32)   # nerf_loader.py:175-177
        # the conditions the cases are chosen for, on the yardstick
        dn = f64["dn"]
        assert (np.abs(dn[..., 2]) >= 0.3).all() and (dn[..., 2] < 0).all(), name
        Kv = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
        o, d = restate.get_rays(W, H, Kv, c2w, np.float64)
        d = restate.normalize(d)
        g = restate.globe_center(SCALE, ORIGIN).astype(np.float64)
        oc = o - g
        b = 2 * (oc * d).sum(-1)
        for radius in (restate.EARTH_RADIUS + restate.BUILDING_HEIGHT, restate.EARTH_RADIUS):
            delta = b * b - 4 * ((oc * oc).sum(-1) - (radius * SCALE) ** 2)
            assert (delta > 0).all(), name
        assert (f64["sphere_rays"][..., 6] > 0).all() and (f64["sphere_rays"][..., 7] > f64["sphere_rays"][..., 6]).all(), name
        # flat: the reference's near is (250 - o_z) / d_z in scene units, so a descending ray has one only from above z = 250 (b7x4);
        # the other cameras show the clamp
        fn, ff = f64["flat_rays"][..., 6], f64["flat_rays"][..., 7]
        assert ((fn > 1.0).all() if c2w[2, 3] > restate.BUILDING_HEIGHT else (fn == 1e-6).all()) and (ff > fn).all(), name
        print(f"{name}: sphere near {f64['sphere_rays'][..., 6].min():.4f}..{f64['sphere_rays'][..., 6].max():.4f}, far "
              f"{f64['sphere_rays'][..., 7].min():.4f}..{f64['sphere_rays'][..., 7].max():.4f}; the float32 reference's distance from "
              f"float64: sphere near {restate.rel_dist(f32['sphere_rays'][..., 6], f64['sphere_rays'][..., 6]):.3e} far "
              f"{restate.rel_dist(f32['sphere_rays'][..., 7], f64['sphere_rays'][..., 7]):.3e} (relative), directions "
              f"{restate.dist(f32['dn'], f64['dn']):.3e}")
    path = os.path.join(ROOT, "tests", "golden", "nerf_rays.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(CAMS)} cameras, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
