"""Fixture of the ray generation (switch_nerf_amd/rays.py over csrc/raygen.hip) from the REFERENCE's own ray_utils.get_ray_directions /
get_rays / get_rays_batch, on the CPU in fp32, outside autocast.

Usage (build container only, like scripts/gen_golden_metrics.py: the reference is not on the GPU box):
    python scripts/gen_golden_raygen.py

Writes tests/golden/raygen.npz, data only:
    W, H, intrinsics (fx, fy, cx, cy), cases (the names)
    dirs_center / dirs_corner      get_ray_directions with center_pixels on / off, fp32 [H, W, 3]
    <case>_c2w [3, 4], _near, _far, _center (0 / 1), _alt (the altitude pair; absent: no planes), _rays fp32 [H, W, 8]:
                                   get_rays(directions [H, W, 3], c2w, near, far, alt)
    batch_c2w [3, 3, 4], batch_pix [50] (row-major pixel indices, repeats included), batch_near / _far / _alt / _center,
    batch_rays fp32 [3, 50, 8]     get_rays_batch(directions.view(-1, 3)[pix], c2w, near, far, alt)
    ref_err_dirs_cam, ref_err_dir  the reference's own fp32 error against the fp64 restatement (tests/raygen_restate.py), max over all
    ref_err_near, ref_err_far      cases: direction components absolute, near and far relative.  The device's bound is 4 x these.
Before it writes, the generator checks what the tests rely on: on every pixel of every case the restatement's |d.x| >= 1e-4 and
|o.x - altitude| >= 1e-4 for both planes, the reference takes the same two branches as the restatement on every ray, and each case shows
what it is named for.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("SWN_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(REF, "switch_nerf"))
import ray_utils as ref  # noqa: E402  (the module alone: the package's __init__ pulls in the whole trainer)
import raygen_restate as restate  # noqa: E402

W, H = 37, 29
FX, FY, CX, CY = 40.0, 43.5, 17.25, 15.625          # fx != fy, an off-centre principal point; fp32-representable
NEAR, FAR = 0.1, 10.0
ALT = [-0.5, 0.3]                                   # x is down: the upper plane (near bound) first, then the ground (far bound)


def look(origin, forward, roll=0.0):
    """c2w [3, 4] fp32 of a camera at `origin` looking along `forward` (world: x down, y right, z back; the camera looks along its -z)."""
    f = np.asarray(forward, np.float64)
    f = f / np.linalg.norm(f)
    r = np.cross(f, np.array([-1.0, 0.0, 0.0]))
    r = r / np.linalg.norm(r)
    u = np.cross(r, f)
    c, s = np.cos(roll), np.sin(roll)
    r, u = c * r + s * u, c * u - s * r
    return torch.from_numpy(np.concatenate([np.stack([r, u, -f], 1), np.asarray(origin, np.float64)[:, None]], 1).astype(np.float32))


CASES = [  # name, c2w, far, altitude pair, center_pixels
    ("plain_center", look([0.2, -0.1, 0.3], [1.0, -0.5, -0.8], 0.1), FAR, None, True),
    ("plain_corner", look([0.2, -0.1, 0.3], [1.0, -0.5, -0.8], 0.1), FAR, None, False),
    ("above_down", look([-2.0, 0.1, -0.2], [1.0, 0.15, -0.1], 0.2), FAR, ALT, True),
    ("oblique_horizon", look([-1.0, 0.3, 0.2], [0.2, 0.3, -1.0]), FAR, ALT, True),
    ("between", look([-0.1, -0.2, 0.1], [0.8, 0.3, -0.5], -0.15), FAR, ALT, True),
    ("below", look([0.8, 0.0, 0.4], [0.5, -0.4, -0.7], 0.05), FAR, ALT, True),
    ("near_beyond_far", look([-30.0, 0.5, -0.5], [1.0, -0.1, 0.2], 0.3), FAR, ALT, True),
]


def check_clear(name, want, c2w, alt):
    dx = np.abs(want[..., 3]).min()
    assert dx >= restate.CLEAR, (name, "min |d.x|", dx)
    for a in (alt or []):
        gap = abs(float(c2w[0, 3]) - float(np.float32(a)))
        assert gap >= restate.CLEAR, (name, "|o.x - altitude|", gap)
    return dx


def main():
    torch.set_num_threads(1)
    out = dict(W=np.int32(W), H=np.int32(H), intrinsics=np.array([FX, FY, CX, CY], np.float32), cases=np.array([c[0] for c in CASES]))
    err = dict(dirs_cam=0.0, dir=0.0, near=0.0, far=0.0)
    dirs = {}
    for center in (True, False):
        d = ref.get_ray_directions(W, H, FX, FY, CX, CY, center, torch.device("cpu"))
        assert d.dtype == torch.float32 and tuple(d.shape) == (H, W, 3)
        dirs[center] = d
        out["dirs_center" if center else "dirs_corner"] = d.numpy()
        err["dirs_cam"] = max(err["dirs_cam"], float(np.abs(d.numpy().astype(np.float64) - restate.directions(W, H, FX, FY, CX, CY, center)).max()))

    def measure(name, got, want, alt, c2w_x):
        e = restate.errors(got, want)
        assert e["origin_exact"], name
        for k in ("dir", "near", "far"):
            err[k] = max(err[k], e[k])
        if alt is not None:       # the reference took the restatement's branches on every ray
            for b_ref, b_want in zip(restate.branches(got, alt), restate.branches(want, alt)):
                assert np.array_equal(b_ref, b_want), name
        return e

    for name, c2w, far, alt, center in CASES:
        r = ref.get_rays(dirs[center], c2w, NEAR, far, alt)
        assert r.dtype == torch.float32 and tuple(r.shape) == (H, W, 8)
        want, hit_n, hit_f = restate.rays(restate.directions(W, H, FX, FY, CX, CY, center), c2w.numpy(), NEAR, far, alt)
        dx = check_clear(name, want, c2w.numpy(), alt)
        e = measure(name, r.numpy(), want, alt, float(c2w[0, 3]))
        near32, far32 = np.float32(NEAR), np.float32(far)
        rn, rf = r.numpy()[..., 6], r.numpy()[..., 7]
        if name == "above_down":
            assert hit_n.all() and hit_f.all() and (rn > near32).all() and (rf < far32).all()
        if name == "oblique_horizon":
            assert (want[..., 3] <= 0).any() and (want[..., 3] > 0).any()
        if name == "between":
            assert not hit_n.any() and (rn == near32).all() and hit_f.any() and (rf[hit_f] < far32).any()
        if name == "below":
            assert not hit_n.any() and not hit_f.any() and (rn == near32).all() and (rf == far32).all()
        if name == "near_beyond_far":
            assert hit_n.all() and (rn > far32).all() and (rf == rn).all()
        print(f"{name}: min |d.x| {dx:.3e}, near-plane rays {int(hit_n.sum())}, far-plane rays {int(hit_f.sum())}, reference error "
              f"dir {e['dir']:.3e} near {e['near']:.3e} far {e['far']:.3e}")
        out.update({f"{name}_c2w": c2w.numpy(), f"{name}_near": np.float32(NEAR), f"{name}_far": np.float32(far),
                    f"{name}_center": np.int32(center), f"{name}_rays": r.numpy()})
        if alt is not None:
            out[f"{name}_alt"] = np.array(alt, np.float32)

    # get_rays_batch: 3 cameras x 50 pixel indices with repeats
    rng = np.random.default_rng(24)
    pix = rng.integers(0, W * H, size=50).astype(np.int64)
    pix[7], pix[31], pix[49] = pix[3], pix[3], 0
    pix[12] = W * H - 1
    c2ws = torch.stack([CASES[2][1], CASES[3][1], CASES[4][1]])
    rb = ref.get_rays_batch(dirs[True].view(-1, 3)[torch.from_numpy(pix)], c2ws, NEAR, FAR, ALT)
    assert rb.dtype == torch.float32 and tuple(rb.shape) == (3, 50, 8)
    dsel = restate.directions(W, H, FX, FY, CX, CY, True).reshape(-1, 3)[pix]
    for k in range(3):
        want, _, _ = restate.rays(dsel, c2ws[k].numpy(), NEAR, FAR, ALT)
        check_clear(f"batch[{k}]", want, c2ws[k].numpy(), ALT)
        measure(f"batch[{k}]", rb[k].numpy(), want, ALT, float(c2ws[k, 0, 3]))
    out.update(batch_c2w=c2ws.numpy(), batch_pix=pix, batch_near=np.float32(NEAR), batch_far=np.float32(FAR),
               batch_alt=np.array(ALT, np.float32), batch_center=np.int32(1), batch_rays=rb.numpy())
    for k, v in err.items():
        assert v > 0
        out[f"ref_err_{k}"] = np.float64(v)
    print("the reference's own fp32 error:", {k: f"{v:.3e}" for k, v in err.items()})
    path = os.path.join(ROOT, "tests", "golden", "raygen.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(CASES)} image cases + the batch case, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
