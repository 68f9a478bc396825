"""CPU-only: the NeRF-dataset ray fixture (tests/golden/nerf_rays.npz, the reference's own get_rays / ndc_rays /
get_bungee_nearfar_radii) against the fp32 restatement (tests/nerf_rays_restate.py), the refusals of the host layer
(switch_nerf_amd/nerf_rays.py) and of the C entries (csrc/raygen_nerf.hip: validation before any launch), and the agreement of
include/swn.h, _lib.py and the built library on the new symbols.

What the restatement settles, bit for bit against the float32 fixture: the pixel grid and K (sub, div, neg), the rotation as
(c0 r0 + c1 r1) + c2 r2, torch.norm as sqrt(fma(z, z, fma(y, y, x x))), ndc_rays statement by statement with its host coefficients
formed in double, the flat near / far.  Two steps cannot be settled that way:
  - the radii's torch.sqrt: the reference's vectorised CPU sqrt is not correctly rounded (on the 37 x 29 image 5 of 1073 radii sit one
    ulp from sqrt of the very same sums, which equal the restatement's - at most two ulps after the division); the small images match bit for bit;
  - the sphere near / far, which the kernel forms in fp64 on purpose: checked against the float64 fixture by the float32 reference's
    own distance from it.
The reference's radii: cat([dx, dx[:, -2:-1]]) over dx's H - 1 rows gives the last image row dx(H - 3), and with H = 2 an empty slice,
i.e. H - 1 rows of radii; the fixture shows both."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import nerf_rays_restate as R

F32 = np.float32


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(f"{golden_dir}/nerf_rays.npz")


def cams(g):
    for c in map(str, g["cams"]):
        K = g[f"{c}_K"]
        yield c, int(g[f"{c}_W"]), int(g[f"{c}_H"]), (K[0, 0], K[1, 1], K[0, 2], K[1, 2]), g[f"{c}_c2w"]


def test_fixture_cases(golden, golden_dir):
    g = golden
    assert [(W, H) for _, W, H, _, _ in cams(g)] == [(5, 3), (7, 4), (4, 2), (37, 29)]
    for c, W, H, (fx, fy, cx, cy), c2w in cams(g):
        assert fx != fy and cx != W / 2 and cy != H / 2 and W != H
        rot = c2w[:, :3].astype(np.float64)
        assert np.abs(rot @ rot.T - np.eye(3)).max() < 1e-6 and (np.abs(rot) > 0.05).all()          # a general rotation
        for k in ("rays_o", "rays_d", "dn", "ndc_o", "ndc_d", "sphere_rays", "flat_rays", "sphere_radii", "flat_radii"):
            for tag, dt in (("", np.float32), ("f64_", np.float64)):
                a = g[f"{tag}{c}_{k}"]
                assert a.dtype == dt and np.isfinite(a).all(), (tag, c, k)
        dn = g[f"f64_{c}_dn"]
        assert (dn[..., 2] < -0.3).all()                                 # NDC: |d_z| well away from 0; flat: every ray descends
        assert g[f"{c}_flat_radii"].shape == ((H - 1) if H == 2 else H, W, 1)
    assert 37 * 29 > 4 * 256 and 37 * 29 % 256 != 0                      # a range can cross workgroup boundaries
    assert (g["b7x4_flat_rays"][..., 6] > 1).all() and (g["a5x3_flat_rays"][..., 6] == F32(1e-6)).all()      # unclamped / clamped near
    assert os.path.getsize(f"{golden_dir}/nerf_rays.npz") < 1 << 20


def test_restatement_equals_the_float32_fixture(golden):
    g = golden
    S, O = float(g["scene_scaling_factor"]), g["scene_origin"]
    for c, W, H, K, c2w in cams(g):
        o, d = R.get_rays(W, H, K, c2w, F32)
        assert R.same_bits(o, g[f"{c}_rays_o"]) and R.same_bits(d, g[f"{c}_rays_d"]), c
        assert R.same_bits(R.normalize(d), g[f"{c}_dn"]), c
        no, nd = R.ndc_rays(W, H, float(g[f"{c}_focal"]), float(g["near_ndc"]), o, d, F32)
        assert R.same_bits(no, g[f"{c}_ndc_o"]) and R.same_bits(nd, g[f"{c}_ndc_d"]), c
        for mode, want in (("raw", d), ("normalized", g[f"{c}_dn"]), ("ndc", g[f"{c}_ndc_d"])):
            r = R.mode_rays(W, H, K, c2w, mode, 2.0, 6.0, F32, float(g[f"{c}_focal"]))
            assert R.same_bits(r[..., 3:6], want) and (r[..., 6] == 2).all() and (r[..., 7] == 6).all()
        flat, rad = R.bungee_rays(W, H, K, c2w, S, O, "flat", F32)
        assert R.same_bits(flat, g[f"{c}_flat_rays"]), c
        ref_rad = g[f"{c}_flat_radii"]
        assert R.same_bits(ref_rad, g[f"{c}_sphere_radii"])
        if H == 2:          # the reference returns one row; the restatement's last row repeats it
            assert R.same_bits(rad[:1], ref_rad) and R.same_bits(rad[1], rad[0])
        elif W * H < 64:
            assert R.same_bits(rad, ref_rad), c
        else:               # torch's vectorised sqrt: not correctly rounded, see the module docstring
            ulp = np.abs(rad.view(np.int32).astype(np.int64) - ref_rad.view(np.int32))
            # (one ulp of the square root, carried through the division's own rounding: two ulps at the most)
            assert ulp.max() <= 2 and (ulp == 0).mean() >= 0.99, (c, int(ulp.max()), float((ulp == 0).mean()))
        if H > 2:           # the last row is dx(H - 3), not dx(H - 2)
            assert R.same_bits(ref_rad[H - 1], ref_rad[H - 3]) and not R.same_bits(ref_rad[H - 1], ref_rad[H - 2])


def test_sphere_restatement_in_fp64_beats_the_float32_reference(golden):
    """The kernel's sphere form (fp32 rays, fp64 distance) lies within the float32 reference's own distance from the float64 fixture -
    the bound the GPU test holds the kernel to - and the float32 reference's cancellation error is what the issue says it is."""
    g = golden
    S, O = float(g["scene_scaling_factor"]), g["scene_origin"]
    for c, W, H, K, c2w in cams(g):
        want = g[f"f64_{c}_sphere_rays"][..., 6:]
        ref_dist = R.rel_dist(g[f"{c}_sphere_rays"][..., 6:], want)
        got, _ = R.bungee_rays(W, H, K, c2w, S, O, "sphere", F32, np.float64)
        mine = R.rel_dist(got[..., 6:], want)
        print(f"{c}: sphere near / far, relative distance from float64: float32 reference {ref_dist:.3e}, fp64-distance form {mine:.3e}")
        assert mine <= ref_dist
        assert R.rel_dist(g[f"ld_{c}_sphere_rays"][..., 6:], want) <= ref_dist          # the bungee loader's own float64 chain, too


def test_host_layer_refuses_bad_arguments():
    from switch_nerf_amd import nerf_rays as nr
    K = torch.tensor([[40.0, 0, 17.25], [0, 43.5, 15.625], [0, 0, 1]])
    pose = torch.eye(4)[:3]
    cam = nr.PinholeCamera(37, 29, K, pose)
    assert nr.PinholeCamera(37, 29, K.numpy(), torch.eye(4)).c2w.shape == (3, 4)
    assert cam.row().tolist() == torch.eye(4)[:3].reshape(-1).tolist() + [40.0, 43.5, 17.25, 15.625]
    s = cam.struct()
    assert (s.fx, s.fy, s.cx, s.cy, s.W, s.H) == (40.0, 43.5, 17.25, 15.625, 37, 29) and list(s.c2w) == pose.reshape(-1).tolist()
    for bad_K in (torch.eye(4), torch.zeros(4), [[1.0, 0.0], [0.0, 1.0]]):
        with pytest.raises(ValueError, match="K must be"):
            nr.PinholeCamera(37, 29, bad_K, pose)
    for bad_pose in (torch.eye(3), torch.zeros(12), torch.zeros(4, 3)):
        with pytest.raises(ValueError, match="c2w must be"):
            nr.PinholeCamera(37, 29, K, bad_pose)
    with pytest.raises(ValueError, match="bad image size"):
        nr.PinholeCamera(0, 29, K, pose)
    for kw in (dict(pixel_begin=1000, n=74), dict(pixel_begin=-1, n=4), dict(pixel_begin=1073), dict(n=0), dict(n=-2)):
        with pytest.raises(ValueError, match="pixel range"):
            nr.camera_rays(cam, "normalized", 2.0, 6.0, **kw)
        with pytest.raises(ValueError, match="pixel range"):
            nr.bungee_rays(cam, 2e-4, [0.0, 0.0, -6371011.0], "sphere", **kw)
    with pytest.raises(ValueError, match="unknown mode 'centered'"):
        nr.camera_rays(cam, "centered", 2.0, 6.0)
    with pytest.raises(ValueError, match="unknown mode 'sphere'"):          # the bungee forms are bungee_rays'
        nr.camera_rays(cam, "sphere", 2.0, 6.0)
    with pytest.raises(ValueError, match="unknown ray_nearfar 'round'"):
        nr.bungee_rays(cam, 2e-4, [0.0, 0.0, -6371011.0], "round")
    with pytest.raises(ValueError, match="near 6.0 > far 2.0"):
        nr.camera_rays(cam, "raw", 6.0, 2.0)
    with pytest.raises(ValueError, match="focal must be positive"):
        nr.camera_rays(cam, "ndc", 0.0, 1.0, focal=0.0)
    with pytest.raises(ValueError, match="H must be at least 2"):
        nr.bungee_rays(nr.PinholeCamera(37, 1, K, pose), 2e-4, [0.0, 0.0, -6371011.0], "flat")
    with pytest.raises(ValueError, match="scene_scaling_factor must be positive"):
        nr.bungee_rays(cam, 0.0, [0.0, 0.0, -6371011.0], "flat")
    with pytest.raises(ValueError, match="three values"):
        nr.bungee_rays(cam, 2e-4, [0.0, -6371011.0], "sphere")
    # a CPU tensor where a device one is needed
    with pytest.raises(ValueError, match="out must be a contiguous fp32 device tensor"):
        nr.camera_rays(cam, "raw", 2.0, 6.0, n=4, out=torch.zeros(4, 8))
    with pytest.raises(ValueError, match="out must be a contiguous fp32 device tensor"):
        nr.bungee_rays(cam, 2e-4, [0.0, 0.0, -6371011.0], "flat", n=4, out=torch.zeros(4, 8), radii_out=torch.zeros(4, 1))
    with pytest.raises(ValueError, match="there is no CPU path"):
        nr.get_rays(29, 37, K, pose)
    with pytest.raises(ValueError, match=r"K must be \[3, 3\]"):
        nr.get_rays(29, 37, torch.eye(4), pose)
    with pytest.raises(ValueError, match="c2w must be a tensor"):
        nr.get_rays(29, 37, K, torch.eye(3))
    with pytest.raises(ValueError, match="bad image size"):
        nr.get_rays(0, 37, K, pose)
    o = torch.zeros(29, 37, 3)
    with pytest.raises(ValueError, match="there is no CPU path"):
        nr.ndc_rays(29, 37, 40.0, 1.0, o, o)
    with pytest.raises(ValueError, match="non-empty fp32 tensor"):
        nr.ndc_rays(29, 37, 40.0, 1.0, o.double(), o)
    with pytest.raises(ValueError, match="share shape and device"):
        nr.ndc_rays(29, 37, 40.0, 1.0, o, o[:5])
    with pytest.raises(ValueError, match="focal must be positive"):
        nr.ndc_rays(29, 37, -1.0, 1.0, o, o)
    table = nr.camera_table([cam, cam], device="cpu")
    assert table.shape == (2, 16) and table[1].tolist() == cam.row().tolist()
    ci, pi = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match=r"\[M, 16\]"):
        nr.pixel_rays(table[:, :12], ci, pi, 37, 29, "raw")
    with pytest.raises(ValueError, match="unknown mode"):
        nr.pixel_rays(table, ci, pi, 37, 29, "centered")
    with pytest.raises(ValueError, match="share dtype and shape"):
        nr.pixel_rays(table, ci, pi.long(), 37, 29, "raw")
    with pytest.raises(ValueError, match="share dtype and shape"):
        nr.pixel_rays(table, ci[:0], pi[:0], 37, 29, "raw")
    with pytest.raises(ValueError, match="int32 or int64"):
        nr.pixel_rays(table, ci.float(), pi.float(), 37, 29, "raw")
    with pytest.raises(ValueError, match="needs a positive focal"):
        nr.pixel_rays(table, ci, pi, 37, 29, "ndc")
    with pytest.raises(ValueError, match="needs scene_scaling_factor and scene_origin"):
        nr.pixel_rays(table, ci, pi, 37, 29, "sphere")
    with pytest.raises(ValueError, match="H must be at least 2"):
        nr.pixel_rays(table, ci, pi, 37, 1, "flat", scene_scaling_factor=2e-4, scene_origin=[0, 0, 0])
    with pytest.raises(ValueError, match="near 6.0 > far 2.0"):
        nr.pixel_rays(table, ci, pi, 37, 29, "normalized", 6.0, 2.0)
    with pytest.raises(ValueError, match="there is no CPU path"):
        nr.pixel_rays(table, ci, pi, 37, 29, "normalized", 2.0, 6.0)
    with pytest.raises(ValueError, match="no cameras"):
        nr.camera_table([])
    with pytest.raises(ValueError, match="share W and H"):
        nr.camera_table([cam, nr.PinholeCamera(36, 29, K, pose)], device="cpu")


def test_render_image_nerf_refuses_training_mode():
    from switch_nerf_amd import nerf_rays as nr, rendering
    cam = nr.PinholeCamera(7, 4, torch.eye(3), torch.eye(4)[:3])
    hp = SimpleNamespace(image_pixel_batch_size=10)
    with pytest.raises(RuntimeError, match="render_image_nerf: nerf is in training mode"):
        rendering.render_image_nerf(SimpleNamespace(training=True), cam, hp, 2.0, 6.0)
    with pytest.raises(RuntimeError, match="render_image_nerf_mip: nerf is in training mode"):
        rendering.render_image_nerf_mip(SimpleNamespace(training=True), cam, hp, 2e-4, [0.0, 0.0, -6371011.0], "sphere")


def _cam_struct(W=37, H=29):
    from switch_nerf_amd import nerf_rays as nr
    return nr.PinholeCamera(W, H, torch.tensor([[40.0, 0, 17.25], [0, 43.5, 15.625], [0, 0, 1]]), torch.eye(4)[:3]).struct()


def test_c_entries_refuse_before_launch():
    """Each -1 path of the five entries, without a GPU (fake non-null pointers are never dereferenced on the host)."""
    from switch_nerf_amd import _lib
    lib = _lib.load()
    p, q = C.c_void_p(0x1000), C.c_void_p(0x1004)
    err = lambda: lib.swn_last_error().decode()
    cam = _cam_struct()
    org = (C.c_double * 3)(0.0, 0.0, -6371011.0)
    f = lib.swn_nerf_rays_from_camera
    assert f(None, 1, 2.0, 6.0, 40.0, 1.0, 0, 10, p, None) == -1 and "null pointer" in err()
    assert f(C.byref(cam), 1, 2.0, 6.0, 40.0, 1.0, 0, 10, None, None) == -1 and "null pointer" in err()
    assert f(C.byref(cam), 1, 2.0, 6.0, 40.0, 1.0, 0, 0, p, None) == -1 and "n must be positive" in err()
    assert f(C.byref(cam), 1, 2.0, 6.0, 40.0, 1.0, 1000, 74, p, None) == -1 and "outside the image's 1073 pixels" in err()
    assert f(C.byref(cam), 1, 2.0, 6.0, 40.0, 1.0, -1, 4, p, None) == -1 and "outside the image" in err()
    assert f(C.byref(cam), 1, 2.0, 6.0, 40.0, 1.0, 0, 10, q, None) == -1 and "misaligned" in err()
    for mode in (-1, 3, 4, 5):
        assert f(C.byref(cam), mode, 2.0, 6.0, 40.0, 1.0, 0, 10, p, None) == -1 and "mode must be" in err()
    assert f(C.byref(cam), 0, 6.5, 6.0, 40.0, 1.0, 0, 10, p, None) == -1 and "near 6.5 > far 6" in err()
    assert f(C.byref(cam), 2, 0.0, 1.0, 0.0, 1.0, 0, 10, p, None) == -1 and "positive finite focal" in err()
    bad = _cam_struct()
    bad.H = 0
    assert f(C.byref(bad), 1, 2.0, 6.0, 40.0, 1.0, 0, 10, p, None) == -1 and "bad image size" in err()
    f = lib.swn_nerf_rays_bungee
    assert f(C.byref(cam), 2e-4, org, 0, 0, 10, p, None, None) == -1 and "null pointer" in err()
    assert f(C.byref(cam), 2e-4, None, 0, 0, 10, p, p, None) == -1 and "null pointer (scene_origin)" in err()
    assert f(C.byref(cam), 2e-4, org, 2, 0, 10, p, p, None) == -1 and "ray_nearfar must be" in err()
    assert f(C.byref(cam), 0.0, org, 1, 0, 10, p, p, None) == -1 and "scene_scaling_factor must be positive" in err()
    assert f(C.byref(cam), 2e-4, org, 1, 1070, 10, p, p, None) == -1 and "outside the image" in err()
    one_row = _cam_struct(37, 1)
    assert f(C.byref(one_row), 2e-4, org, 1, 0, 10, p, p, None) == -1 and "two image rows, got H 1" in err()
    f = lib.swn_nerf_rays_from_pixels
    for i64 in (0, 1):
        assert f(None, 3, p, p, i64, 10, 37, 29, 1, 2.0, 6.0, 40.0, 1.0, 2e-4, org, p, None, None) == -1 and "null pointer" in err()
        assert f(p, 3, p, None, i64, 10, 37, 29, 1, 2.0, 6.0, 40.0, 1.0, 2e-4, org, p, None, None) == -1 and "null pointer" in err()
        assert f(p, 3, p, p, i64, 0, 37, 29, 1, 2.0, 6.0, 40.0, 1.0, 2e-4, org, p, None, None) == -1 and "n must be positive" in err()
        assert f(p, 0, p, p, i64, 10, 37, 29, 1, 2.0, 6.0, 40.0, 1.0, 2e-4, org, p, None, None) == -1 and "bad sizes" in err()
        assert f(p, 3, p, p, i64, 10, 37, 29, 7, 2.0, 6.0, 40.0, 1.0, 2e-4, org, p, None, None) == -1 and "unknown mode 7" in err()
        assert f(p, 3, p, p, i64, 10, 37, 29, 3, 2.0, 6.0, 40.0, 1.0, 2e-4, org, p, None, None) == -1 and "write radii" in err()
        assert f(p, 3, p, p, i64, 10, 37, 1, 4, 2.0, 6.0, 40.0, 1.0, 2e-4, org, p, p, None) == -1 and "two image rows" in err()
        assert f(p, 3, p, p, i64, 10, 37, 29, 0, 6.5, 6.0, 40.0, 1.0, 2e-4, org, p, None, None) == -1 and "near 6.5 > far 6" in err()
    assert f(p, 3, p, p, 0, 10, 1 << 16, 1 << 16, 1, 2.0, 6.0, 40.0, 1.0, 2e-4, org, p, None, None) == -1 and "outside int32 indices" in err()
    assert f(p, 3, q, q, 1, 10, 37, 29, 1, 2.0, 6.0, 40.0, 1.0, 2e-4, org, p, None, None) == -1 and "misaligned" in err()
    f = lib.swn_nerf_rays_dirs
    assert f(None, 37, 29, p, p, None) == -1 and "null pointer" in err()
    assert f(p, 0, 29, p, p, None) == -1 and "bad image size" in err()
    assert f(q, 37, 29, p, p, None) == -1 and "misaligned" in err()
    f = lib.swn_nerf_ndc
    assert f(p, p, 10, 37, 29, 40.0, 1.0, p, None, None) == -1 and "null pointer" in err()
    assert f(p, p, 0, 37, 29, 40.0, 1.0, p, p, None) == -1 and "n must be positive" in err()
    assert f(p, p, 10, 37, 0, 40.0, 1.0, p, p, None) == -1 and "bad image size" in err()
    assert f(p, p, 10, 37, 29, -2.0, 1.0, p, p, None) == -1 and "positive finite focal" in err()


NEW = ("swn_nerf_rays_from_camera", "swn_nerf_rays_bungee", "swn_nerf_rays_from_pixels", "swn_nerf_rays_dirs", "swn_nerf_ndc")


def test_header_binding_and_library_agree_on_the_new_symbols():
    from switch_nerf_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "swn.h")).read(), flags=re.S)
    ctype = {"int": _lib.i32, "long": _lib.i64, "float": _lib.f32, "double": _lib.f64}
    lib = _lib.load()
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, f"{name} is not declared in include/swn.h"
        want = []
        for arg in m.group(1).split(","):
            arg = " ".join(arg.split())
            if "swn_nerf_camera*" in arg:
                want.append(C.POINTER(_lib.NerfCamera))
            elif "*" in arg:
                want.append(_lib.vp)
            else:
                want.append(ctype[arg.rsplit(" ", 1)[0]])
        assert _lib.SIGNATURES[name] == want, name
        assert hasattr(lib, name), f"the built library does not export {name}"
    fields = re.search(r"typedef struct swn_nerf_camera \{(.*?)\}", text, re.S).group(1)
    assert " ".join(fields.split()) == "float c2w[12]; float fx, fy, cx, cy; int32_t W, H;"
    assert [f[0] for f in _lib.NerfCamera._fields_] == ["c2w", "fx", "fy", "cx", "cy", "W", "H"] and C.sizeof(_lib.NerfCamera) == 72
    for k, v in dict(RAW=0, NORMALIZED=1, NDC=2, BUNGEE_SPHERE=3, BUNGEE_FLAT=4, SPHERE=0, FLAT=1).items():
        assert re.search(r"#define SWN_NERF_%s %d\b" % (k, v), text) and getattr(_lib, f"NERF_{k}") == v
    f16 = C.CDLL(_lib.LIB_PATH_F16)
    assert all(hasattr(f16, name) for name in NEW)
