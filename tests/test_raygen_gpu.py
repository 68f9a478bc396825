"""GPU: the ray kernels (switch_nerf_amd/rays.py over csrc/raygen.hip) against the fp64 restatement (tests/raygen_restate.py) on the
fixture of the reference's own rays (tests/golden/raygen.npz): a 37 x 29 image (1073 pixels: no multiple of 64 or 256, a row shorter
than a wave), fx != fy, an off-centre principal point.  Bounds: 4 x the reference's own fp32 error stored in the fixture (direction
components absolute, near / far relative); origins and the default near / far exact; on every ray the branches o.x < altitude and
d.x > 0 as the reference took them.  The entries agree with each other bit for bit.

Measured on the MI355X: profiles/r24_raygen.md."""
import numpy as np
import pytest
import torch

import raygen_restate as restate
from raygen_restate import CASES, intr, want_batch, want_case

pytestmark = pytest.mark.gpu

W, H = 37, 29
P = W * H
_cache = {}


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(f"{golden_dir}/raygen.npz")


def want(g, name):
    """The restatement of a case: computed once, shared, never modified."""
    if name not in _cache:
        _cache[name] = want_batch(g) if name == "batch" else want_case(g, name)
    return _cache[name]


def alt_of(g, name):
    return [float(a) for a in g[f"{name}_alt"]] if f"{name}_alt" in g.files else None


def camera(g, name, index=0, c2w=None):
    from switch_nerf_amd.rays import Camera
    return Camera(W, H, g["intrinsics"].tolist(), torch.from_numpy(g[f"{name}_c2w"] if c2w is None else c2w), index)


def args(g, name):
    return float(g[f"{name}_near"]), float(g[f"{name}_far"]), alt_of(g, name), bool(g[f"{name}_center"])


def bits(t):
    return t.contiguous().view(torch.int32)


def check(g, what, got, want_rays, ref_rays, near, far, alt):
    """got (device, [..., 8]) within the bounds of the restatement, exact where the values are copies, the reference's branches."""
    got = got.cpu().numpy()
    assert got.shape == want_rays.shape and got.dtype == np.float32, what
    e = restate.errors(got, want_rays)
    bound = {k: restate.MARGIN * float(g[f"ref_err_{k}"]) for k in ("dir", "near", "far")}
    print(f"    {what}: dir {e['dir']:.3e} (bound {bound['dir']:.3e}) near {e['near']:.3e} ({bound['near']:.3e}) far {e['far']:.3e} "
          f"({bound['far']:.3e})")
    assert e["origin_exact"], what
    for k in bound:
        assert e[k] <= bound[k], (what, k, e[k], bound[k])
    for col, default in ((6, near), (7, far)):
        copies = want_rays[..., col] == np.float64(np.float32(default))
        assert np.array_equal(got[..., col][copies], np.full(int(copies.sum()), np.float32(default))), (what, col)
    if alt is not None:
        for b_got, b_ref in zip(restate.branches(got, alt), restate.branches(ref_rays, alt)):
            assert np.array_equal(b_got, b_ref), what


@pytest.mark.parametrize("name", CASES)
def test_image_case_every_entry(golden, name):
    from switch_nerf_amd import rays
    g = golden
    (want_rays, _, _), _ = want(g, name)
    near, far, alt, center = args(g, name)
    cam = camera(g, name)
    ref = g[f"{name}_rays"]
    print(f"\n{name}")
    fused = rays.camera_rays(cam, near, far, alt, center)
    assert fused.shape == (P, 8)
    check(g, "fused", fused.view(H, W, 8), want_rays, ref, near, far, alt)
    dirs = rays.get_ray_directions(W, H, *intr(g), center, "cuda")
    assert dirs.shape == (H, W, 3) and dirs.dtype == torch.float32
    cam_err = float(np.abs(dirs.cpu().numpy().astype(np.float64) - restate.directions(W, H, *intr(g), center)).max())
    print(f"    camera-space directions: {cam_err:.3e} (bound {restate.MARGIN * float(g['ref_err_dirs_cam']):.3e})")
    assert cam_err <= restate.MARGIN * float(g["ref_err_dirs_cam"])
    pair = rays.get_rays(dirs, torch.from_numpy(g[f"{name}_c2w"]).cuda(), near, far, alt)
    assert pair.shape == (H, W, 8)
    check(g, "two launches", pair, want_rays, ref, near, far, alt)
    assert torch.equal(bits(pair.view(P, 8)), bits(fused))                      # the fused entry IS the two-launch pair
    table = rays.camera_table([cam])
    for dt in (torch.int32, torch.int64):
        got = rays.pixel_rays(table, torch.zeros(P, dtype=dt, device="cuda"), torch.arange(P, dtype=dt, device="cuda"), W, H, near, far,
                              alt, center, check=True)
        check(g, f"gather {dt}", got.view(H, W, 8), want_rays, ref, near, far, alt)
        assert torch.equal(bits(got), bits(fused))


def test_batch_case_every_entry(golden):
    """get_rays_batch's case: 3 cameras x 50 pixel indices with repeats."""
    from switch_nerf_amd import rays
    g = golden
    wants = want(g, "batch")
    near, far, alt, center = args(g, "batch")
    pix = torch.from_numpy(g["batch_pix"]).cuda()
    cams = [camera(g, "batch", k, c2w=g["batch_c2w"][k]) for k in range(3)]
    dirs = rays.get_ray_directions(W, H, *intr(g), center, "cuda")
    pair = rays.get_rays_batch(dirs.view(-1, 3)[pix], torch.from_numpy(g["batch_c2w"]).cuda(), near, far, alt)
    assert pair.shape == (3, 50, 8)
    table = rays.camera_table(cams)
    print()
    for dt in (torch.int32, torch.int64):
        ci = torch.arange(3, device="cuda").repeat_interleave(50).to(dt)
        gather = rays.pixel_rays(table, ci, pix.repeat(3).to(dt), W, H, near, far, alt, center, check=True).view(3, 50, 8)
        assert torch.equal(bits(gather), bits(pair))
    for k in range(3):
        check(g, f"get_rays_batch camera {k}", pair[k], wants[k][0], g["batch_rays"][k], near, far, alt)
        fused = rays.camera_rays(cams[k], near, far, alt, center)[pix]
        assert torch.equal(bits(fused), bits(pair[k]))


@pytest.mark.parametrize("name", ["oblique_horizon", "plain_corner"])
def test_pixel_range_is_a_slice_of_the_image(golden, name):
    from switch_nerf_amd import rays
    g = golden
    near, far, alt, center = args(g, name)
    cam = camera(g, name)
    whole = rays.camera_rays(cam, near, far, alt, center)
    seen = 0
    for begin in (0, 1, 36, 37, 1000):
        for n in (1, 63, 64, 65, 257, P - begin):
            if begin + n > P:
                continue
            part = rays.camera_rays(cam, near, far, alt, center, pixel_begin=begin, n=n)
            assert part.shape == (n, 8) and torch.equal(bits(part), bits(whole[begin:begin + n])), (begin, n)
            seen += 1
        tail = rays.camera_rays(cam, near, far, alt, center, pixel_begin=begin)          # n None: to the end
        assert torch.equal(bits(tail), bits(whole[begin:]))
    assert seen == 4 * 6 + 5


def test_one_pixel_image(golden):
    from switch_nerf_amd import rays
    g = golden
    near, far, alt, center = args(g, "above_down")
    cam = rays.Camera(1, 1, [40.0, 43.5, 0.25, -0.5], torch.from_numpy(g["above_down_c2w"]), 3)
    one = rays.camera_rays(cam, near, far, alt, center)
    assert one.shape == (1, 8)
    w, _, _ = restate.rays(restate.directions(1, 1, 40.0, 43.5, 0.25, -0.5, center), g["above_down_c2w"], near, far, alt)
    e = restate.errors(one.cpu().numpy().reshape(1, 1, 8), w)
    assert e["origin_exact"] and all(e[k] <= restate.MARGIN * float(g[f"ref_err_{k}"]) for k in ("dir", "near", "far")), e
    pair = rays.get_rays(rays.get_ray_directions(1, 1, 40.0, 43.5, 0.25, -0.5, center, "cuda"), cam.c2w.cuda(), near, far, alt)
    assert torch.equal(bits(pair.view(1, 8)), bits(one))
    assert torch.equal(bits(rays.camera_rays(cam, near, far, alt, center, pixel_begin=0, n=1)), bits(one))


@pytest.mark.parametrize("N", [1, 257])
def test_gather_equals_the_cameras_own_pixels(golden, N):
    from switch_nerf_amd import rays
    g = golden
    near, far, alt, center = args(g, "batch")
    cams = [camera(g, "batch", k, c2w=g["batch_c2w"][k]) for k in range(3)]
    whole = torch.stack([rays.camera_rays(c, near, far, alt, center) for c in cams])
    rng = np.random.default_rng(N)
    ci, pi = torch.from_numpy(rng.integers(0, 3, N)).cuda(), torch.from_numpy(rng.integers(0, P, N)).cuda()
    pi[-1] = P - 1
    table = rays.camera_table(cams)
    for dt in (torch.int32, torch.int64):
        got = rays.pixel_rays(table, ci.to(dt), pi.to(dt), W, H, near, far, alt, center)
        assert got.shape == (N, 8) and torch.equal(bits(got), bits(whole[ci, pi]))
    with pytest.raises(ValueError, match="index out of range"):
        rays.pixel_rays(table, ci, torch.full_like(pi, P), W, H, near, far, alt, center, check=True)
    with pytest.raises(ValueError, match="index out of range"):
        rays.pixel_rays(table, torch.full_like(ci, 3), pi, W, H, near, far, alt, center, check=True)


def test_out_buffers_are_written_in_place(golden):
    from switch_nerf_amd import rays
    g = golden
    near, far, alt, center = args(g, "between")
    cam = camera(g, "between", index=7)
    whole = rays.camera_rays(cam, near, far, alt, center)
    buf = torch.full((P + 2, 8), -1.0, device="cuda")
    idx = torch.full((300,), -1, dtype=torch.long, device="cuda")
    out = rays.camera_rays(cam, near, far, alt, center, pixel_begin=100, n=257, out=buf[1:258], image_indices_out=idx[3:260])
    assert out.data_ptr() == buf[1:258].data_ptr() and torch.equal(bits(buf[1:258]), bits(whole[100:357]))
    assert (buf[0] == -1).all() and (buf[258:] == -1).all()                    # nothing outside the slice
    assert (idx[3:260] == 7).all() and (idx[:3] == -1).all() and (idx[260:] == -1).all()
    table = rays.camera_table([cam])
    z = torch.zeros(257, dtype=torch.int32, device="cuda")
    out2 = rays.pixel_rays(table, z, torch.arange(100, 357, dtype=torch.int32, device="cuda"), W, H, near, far, alt, center, out=buf[1:258])
    assert out2.data_ptr() == buf[1:258].data_ptr() and torch.equal(bits(out2), bits(whole[100:357]))
    with pytest.raises(ValueError, match="out must be"):
        rays.camera_rays(cam, near, far, alt, center, n=10, out=buf[:11])
    with pytest.raises(ValueError, match="image_indices_out"):
        rays.camera_rays(cam, near, far, alt, center, n=10, out=buf[:10], image_indices_out=idx[:10].int())
