"""GPU: switch_nerf_amd/nerf_rays.py over csrc/raygen_nerf.hip against tests/golden/nerf_rays.npz (the reference's own get_rays,
ndc_rays and get_bungee_nearfar_radii on 5 x 3, 7 x 4, 4 x 2 and 37 x 29 images) and the restatement tests/nerf_rays_restate.py.

Bit for bit against the float32 fixture: get_rays, RAW, NORMALIZED, ndc_rays, NDC, the flat near / far, and the radii of the small
images - every step there is an fp32 mul, add, div, sqrt or the one fused multiply-add written out in the kernel.  Two things cannot:
  - the radii of the 37 x 29 image: the reference's vectorised CPU torch.sqrt is not correctly rounded (tests/test_nerf_rays_cpu.py:
    5 of 1073 values sit one ulp from the IEEE square root of the same sums).  Bound: twice the float32 fixture's own distance from the
    float64 fixture, which is 5.5e-08 absolute on radii of 1e-2 - the directions' 1e-7 cancels into them (profiles/r25_nerf_rays.md);
  - the sphere near / far, formed in fp64 in the kernel on purpose: within the float32 fixture's own relative distance from the float64
    fixture (1.3e-4 ... 3.9e-4 on the low cameras, 3.5e-7 on the high one), not a fixed tolerance.
Everything the kernels write also equals the restatement bit for bit (the sphere form with its distance in fp64).
The reference's cat([dx, dx[:, -2:-1]]) gives the last image row the radius of row H - 3 (dx has H - 1 rows), which the fixture shows
and the kernel follows; with H = 2 the reference's slice is empty and the kernel's last row repeats row 0."""
import numpy as np
import pytest
import torch

import nerf_rays_restate as R

pytestmark = pytest.mark.gpu

F32 = np.float32
NEAR, FAR = 2.0, 6.0
RANGES = {  # (pixel_begin, n): mid-row starts, spans of rows, the last row, n = 1
    "a5x3": [(0, 15), (2, 9), (7, 1), (11, 4), (14, 1)],
    "b7x4": [(3, 20), (21, 7), (22, 3), (27, 1)],
    "c4x2": [(0, 8), (1, 6), (4, 4), (5, 1), (7, 1)],
    "d37x29": [(250, 600), (0, 1073), (1036, 37), (1050, 23), (511, 2), (1072, 1)],      # 250 + 600: across workgroups
}


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(f"{golden_dir}/nerf_rays.npz")


class Cam:
    def __init__(self, g, c):
        from switch_nerf_amd import nerf_rays as nr
        self.c, self.W, self.H = c, int(g[f"{c}_W"]), int(g[f"{c}_H"])
        self.K, self.c2w, self.focal = g[f"{c}_K"], g[f"{c}_c2w"], float(g[f"{c}_focal"])
        self.Kv = (self.K[0, 0], self.K[1, 1], self.K[0, 2], self.K[1, 2])
        self.cam = nr.PinholeCamera(self.W, self.H, self.K, self.c2w)
        self.S, self.O = float(g["scene_scaling_factor"]), g["scene_origin"]
        self.whole = {m: nr.camera_rays(self.cam, m, NEAR, FAR, focal=self.focal) for m in ("raw", "normalized", "ndc")}
        for kind in ("sphere", "flat"):
            self.whole[kind], self.whole[kind + "_radii"] = nr.bungee_rays(self.cam, self.S, self.O, kind)

    def np(self, key):
        return self.whole[key].cpu().numpy()


@pytest.fixture(scope="module")
def cams(g):
    return {c: Cam(g, c) for c in map(str, g["cams"])}


def eq(a: torch.Tensor, b) -> bool:
    b = torch.as_tensor(b).to(a.device)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_get_rays_and_the_three_modes_bit_for_bit(g, cams):
    from switch_nerf_amd import nerf_rays as nr
    for c, k in cams.items():
        W, H, P = k.W, k.H, k.W * k.H
        o, d = nr.get_rays(H, W, torch.from_numpy(k.K), torch.from_numpy(k.c2w).cuda())
        assert o.shape == d.shape == (H, W, 3) and eq(o, g[f"{c}_rays_o"]) and eq(d, g[f"{c}_rays_d"]), c
        o4, d4 = nr.get_rays(H, W, torch.from_numpy(k.K).cuda(), torch.cat([torch.from_numpy(k.c2w), torch.tensor([[0, 0, 0, 1.0]])]).cuda())
        assert eq(o4, o) and eq(d4, d)                                             # a [4, 4] pose, K on the device
        no, nd = nr.ndc_rays(H, W, k.focal, float(g["near_ndc"]), o, d)
        assert no.shape == (H, W, 3) and eq(no, g[f"{c}_ndc_o"]) and eq(nd, g[f"{c}_ndc_d"]), c
        want = {"raw": (g[f"{c}_rays_o"], g[f"{c}_rays_d"]), "normalized": (g[f"{c}_rays_o"], g[f"{c}_dn"]),
                "ndc": (g[f"{c}_ndc_o"], g[f"{c}_ndc_d"])}
        for mode, (wo, wd) in want.items():
            r = k.whole[mode]
            assert r.shape == (P, 8) and r.dtype == torch.float32
            assert eq(r[:, :3].contiguous(), wo.reshape(P, 3)) and eq(r[:, 3:6].contiguous(), wd.reshape(P, 3)), (c, mode)
            assert (r[:, 6] == NEAR).all() and (r[:, 7] == FAR).all()
            assert eq(r, R.mode_rays(W, H, k.Kv, k.c2w, mode, NEAR, FAR, F32, k.focal).reshape(P, 8)), (c, mode)
        # the fused forms equal the two-step ones
        assert eq(k.whole["ndc"][:, :3].contiguous(), no.view(P, 3)) and eq(k.whole["ndc"][:, 3:6].contiguous(), nd.view(P, 3))
        # focal None: K[0][0]
        assert eq(nr.camera_rays(k.cam, "ndc", NEAR, FAR), R.mode_rays(W, H, k.Kv, k.c2w, "ndc", NEAR, FAR, F32).reshape(P, 8))


def test_flat_near_far_bit_for_bit(g, cams):
    for c, k in cams.items():
        P = k.W * k.H
        assert eq(k.whole["flat"], g[f"{c}_flat_rays"].reshape(P, 8)), c
        assert eq(k.whole["flat"][:, :6].contiguous(), k.whole["normalized"][:, :6].contiguous())
    assert (cams["a5x3"].whole["flat"][:, 6] == 1e-6).all() and (cams["b7x4"].whole["flat"][:, 6] > 1).all()      # the clamp, and none


def test_sphere_near_far_within_the_float32_reference_distance(g, cams):
    for c, k in cams.items():
        P = k.W * k.H
        got = k.np("sphere")
        assert R.same_bits(got[:, :6], g[f"{c}_sphere_rays"].reshape(P, 8)[:, :6])           # origins and directions: bit for bit
        want = g[f"f64_{c}_sphere_rays"].reshape(P, 8)[:, 6:]
        bound = R.rel_dist(g[f"{c}_sphere_rays"].reshape(P, 8)[:, 6:], want)
        mine = R.rel_dist(got[:, 6:], want)
        print(f"{c}: sphere near / far relative distance from float64: kernel {mine:.3e}, float32 reference {bound:.3e}")
        assert mine <= bound, c
        rest, _ = R.bungee_rays(k.W, k.H, k.Kv, k.c2w, k.S, k.O, "sphere", F32, np.float64)
        assert R.same_bits(got, rest.reshape(P, 8)), c                                       # the fp64 steps are IEEE, too
        assert (got[:, 6] > 0).all() and (got[:, 7] > got[:, 6]).all()


def test_radii(g, cams):
    for c, k in cams.items():
        W, H, P = k.W, k.H, k.W * k.H
        rad = k.np("sphere_radii")
        assert rad.shape == (P, 1) and R.same_bits(rad, k.np("flat_radii"))
        rad = rad.reshape(H, W, 1)
        ref32, ref64 = g[f"{c}_flat_radii"], g[f"f64_{c}_flat_radii"]
        rows = ref32.shape[0]                                                # H, or H - 1 where H == 2 (the reference's empty slice)
        ref_dist = R.dist(ref32, ref64)
        mine = R.dist(rad[:rows], ref64)
        print(f"{c}: radii distance from float64: kernel {mine:.3e}, float32 reference {ref_dist:.3e}")
        assert mine <= 2 * ref_dist, c
        if P < 64:
            assert R.same_bits(rad[:rows], ref32), c
        assert R.same_bits(rad, R.radii(R.normalize(R.get_rays(W, H, k.Kv, k.c2w, F32)[1]), F32)), c
        last = H - 3 if H >= 3 else 0
        assert R.same_bits(rad[H - 1], rad[last]) and (rad > 0).all()
        if H >= 3:
            assert R.same_bits(rad[H - 1], ref32[H - 1]) or P >= 64
            assert not R.same_bits(rad[H - 1], rad[H - 2])


def test_pixel_ranges_equal_rows_of_the_whole_image(cams):
    from switch_nerf_amd import nerf_rays as nr
    for c, k in cams.items():
        assert any(b >= (k.H - 1) * k.W for b, _ in RANGES[c])               # a range that begins in the last row
        for b, n in RANGES[c]:
            for mode in ("raw", "normalized", "ndc"):
                assert eq(nr.camera_rays(k.cam, mode, NEAR, FAR, focal=k.focal, pixel_begin=b, n=n), k.whole[mode][b:b + n]), (c, mode, b, n)
            for kind in ("sphere", "flat"):
                r, rad = nr.bungee_rays(k.cam, k.S, k.O, kind, pixel_begin=b, n=n)
                assert eq(r, k.whole[kind][b:b + n]) and eq(rad, k.whole[kind + "_radii"][b:b + n]), (c, kind, b, n)
        r = nr.camera_rays(k.cam, "normalized", NEAR, FAR, pixel_begin=k.W + 1)             # n None: to the end of the image
        assert eq(r, k.whole["normalized"][k.W + 1:])


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_gather_form_gives_the_fused_form_bits(cams, dtype):
    from switch_nerf_amd import nerf_rays as nr
    k = cams["d37x29"]
    other = nr.PinholeCamera(k.W, k.H, cams["b7x4"].K, cams["a5x3"].c2w)           # a second camera of the same size
    table = nr.camera_table([k.cam, other, k.cam])
    P = k.W * k.H
    rng = np.random.default_rng(7)
    pix = rng.integers(0, P, size=300)
    pix[:6] = [0, P - 1, P - k.W, k.W - 1, pix[10], (k.H - 2) * k.W + 3]                # corners, the last row, a repeat
    ci = torch.from_numpy(rng.integers(0, 3, size=300)).to("cuda", dtype)
    pi = torch.from_numpy(pix).to("cuda", dtype)
    whole = {0: k.whole, 2: k.whole, 1: {m: nr.camera_rays(other, m, NEAR, FAR, focal=k.focal) for m in ("raw", "normalized", "ndc")}}
    for kind in ("sphere", "flat"):
        whole[1][kind], whole[1][kind + "_radii"] = nr.bungee_rays(other, k.S, k.O, kind)
    pick = lambda key: torch.stack([whole[int(a)][key][int(b)] for a, b in zip(ci.tolist(), pi.tolist())])
    for mode in ("raw", "normalized", "ndc"):
        r = nr.pixel_rays(table, ci, pi, k.W, k.H, mode, NEAR, FAR, focal=k.focal, check=True)
        assert eq(r, pick(mode)), mode
    for kind in ("sphere", "flat"):
        r, rad = nr.pixel_rays(table, ci, pi, k.W, k.H, kind, scene_scaling_factor=k.S, scene_origin=k.O)
        assert eq(r, pick(kind)) and eq(rad, pick(kind + "_radii")), kind
    with pytest.raises(ValueError, match="index out of range"):
        nr.pixel_rays(table, ci, pi + P, k.W, k.H, "raw", NEAR, FAR, check=True)


def test_out_buffers_are_written_in_place(cams):
    from switch_nerf_amd import nerf_rays as nr
    k = cams["b7x4"]
    b, n = 3, 20
    buf = torch.full((n + 2, 8), -7.0, device="cuda")
    out = buf[1:n + 1]
    got = nr.camera_rays(k.cam, "normalized", NEAR, FAR, pixel_begin=b, n=n, out=out)
    assert got is out and eq(out, k.whole["normalized"][b:b + n]) and (buf[0] == -7).all() and (buf[-1] == -7).all()
    rbuf = torch.full((n + 2, 1), -7.0, device="cuda")
    rout = rbuf[1:n + 1]
    r, rad = nr.bungee_rays(k.cam, k.S, k.O, "sphere", pixel_begin=b, n=n, out=out, radii_out=rout)
    assert r is out and rad is rout and eq(out, k.whole["sphere"][b:b + n]) and eq(rout, k.whole["sphere_radii"][b:b + n])
    assert (rbuf[0] == -7).all() and (rbuf[-1] == -7).all() and (buf[0] == -7).all() and (buf[-1] == -7).all()
    table = nr.camera_table([k.cam])
    ci, pi = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.arange(b, b + n, device="cuda")
    out.fill_(0)
    rout.fill_(0)
    r, rad = nr.pixel_rays(table, ci, pi, k.W, k.H, "flat", scene_scaling_factor=k.S, scene_origin=k.O, out=out, radii_out=rout)
    assert r is out and rad is rout and eq(out, k.whole["flat"][b:b + n]) and eq(rout, k.whole["flat_radii"][b:b + n])
    for bad in (torch.zeros(n, 8, device="cuda", dtype=torch.float64), torch.zeros(n + 1, 8, device="cuda"), torch.zeros(8, n, device="cuda").t()):
        with pytest.raises(ValueError, match="out must be a contiguous fp32 device tensor"):
            nr.camera_rays(k.cam, "raw", NEAR, FAR, pixel_begin=b, n=n, out=bad)
    with pytest.raises(ValueError, match="radii_out must be a contiguous fp32 tensor"):
        nr.bungee_rays(k.cam, k.S, k.O, "flat", pixel_begin=b, n=n, out=out, radii_out=torch.zeros(n, device="cuda"))
