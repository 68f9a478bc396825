"""CPU-only: the ray-generation fixture (tests/golden/raygen.npz, the reference's own ray_utils in fp32) against the fp64 restatement
(tests/raygen_restate.py), the conditions the fixture keeps so that no ray sits on a branch, the pixel-batch arithmetic of
rendering.render_image, every refusal of the C entries (csrc/raygen.hip: validation before any launch) and of the wrappers
(switch_nerf_amd/rays.py), the Camera / camera_table layouts and render_image's training-mode refusal."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import raygen_restate as restate
from raygen_restate import CASES, intr, want_batch, want_case


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(f"{golden_dir}/raygen.npz")
    assert list(map(str, g["cases"])) == CASES
    return g


def test_fixture_shape_and_size(golden, golden_dir):
    import os
    g = golden
    assert (int(g["W"]), int(g["H"])) == (37, 29) and 37 * 29 % 64 != 0 and 37 * 29 % 256 != 0
    fx, fy, cx, cy = intr(g)
    assert fx != fy and cx != 37 / 2 and cy != 29 / 2
    for name in CASES:
        assert g[f"{name}_rays"].shape == (29, 37, 8) and g[f"{name}_rays"].dtype == np.float32
    assert g["batch_rays"].shape == (3, 50, 8) and len(set(g["batch_pix"].tolist())) < 50          # repeats included
    assert os.path.getsize(f"{golden_dir}/raygen.npz") < 256 * 1024


def test_restatement_against_the_reference(golden):
    """The reference's fp32 rays lie within the errors the generator measured and stored (and reach them: the stored numbers ARE the
    maxima), origins and the default near / far exactly; the camera-space directions likewise."""
    g = golden
    worst = dict(dir=0.0, near=0.0, far=0.0)
    for name in CASES:
        (want, _, _), alt = want_case(g, name)
        got = g[f"{name}_rays"]
        e = restate.errors(got, want)
        assert e["origin_exact"], name
        for k in worst:
            worst[k] = max(worst[k], e[k])
        for col, default in ((6, g[f"{name}_near"]), (7, g[f"{name}_far"])):
            copies = want[..., col] == np.float64(np.float32(default))
            assert np.array_equal(got[..., col][copies], np.full(int(copies.sum()), np.float32(default))), (name, col)
    for k, (want, _, _) in enumerate(want_batch(g)):
        e = restate.errors(g["batch_rays"][k], want)
        assert e["origin_exact"]
        for q in worst:
            worst[q] = max(worst[q], e[q])
    for k, v in worst.items():
        assert v == float(g[f"ref_err_{k}"]), (k, v)
    cam = max(float(np.abs(g[n].astype(np.float64) - restate.directions(37, 29, *intr(g), c)).max())
              for n, c in (("dirs_center", True), ("dirs_corner", False)))
    assert cam == float(g["ref_err_dirs_cam"])
    assert 0 < cam < 4e-7 and 0 < worst["dir"] < 4e-7          # a few fp32 ulps of a unit vector's component


def test_fixture_keeps_clear_of_the_branches(golden):
    """|d.x| >= 1e-4 on every pixel of every case and |o.x - altitude| >= 1e-4 for both planes, so the discontinuous conditions
    o.x < alt and d.x > 0 are decided the same way by every valid fp32 order - and the reference decides them as the restatement does."""
    g = golden
    items = [(name, want_case(g, name)[0][0], g[f"{name}_rays"], g[f"{name}_alt"] if f"{name}_alt" in g.files else None, g[f"{name}_c2w"])
             for name in CASES]
    items += [(f"batch{k}", w[0], g["batch_rays"][k], g["batch_alt"], g["batch_c2w"][k]) for k, w in enumerate(want_batch(g))]
    for name, want, got, alt, c2w in items:
        assert np.abs(want[..., 3]).min() >= restate.CLEAR, name
        if alt is not None:
            assert alt[0] < alt[1]
            for a in alt:
                assert abs(float(c2w[0, 3]) - float(a)) >= restate.CLEAR, name
            for b_got, b_want in zip(restate.branches(got, alt), restate.branches(want, alt)):
                assert np.array_equal(b_got, b_want), name


def test_cases_show_what_they_are_named_for(golden):
    g = golden
    res = {name: want_case(g, name)[0] for name in CASES}
    near, far = np.float32(g["above_down_near"]), np.float32(g["above_down_far"])
    r = lambda n: g[f"{n}_rays"]
    assert "plain_center_alt" not in g.files and int(g["plain_center_center"]) == 1 and int(g["plain_corner_center"]) == 0
    assert res["above_down"][1].all() and res["above_down"][2].all() and (r("above_down")[..., 6] > near).all() and (r("above_down")[..., 7] < far).all()
    dx = res["oblique_horizon"][0][..., 3]
    assert (dx <= 0).any() and (dx > 0).any()
    assert not res["between"][1].any() and res["between"][2].all() and (r("between")[..., 6] == near).all() and (r("between")[..., 7] < far).any()
    assert not res["below"][1].any() and not res["below"][2].any() and (r("below")[..., 7] == far).all()
    nb = r("near_beyond_far")
    assert (nb[..., 6] > far).all() and np.array_equal(nb[..., 6], nb[..., 7])          # far = max(near, far)


def test_render_image_batch_arithmetic():
    from switch_nerf_amd.rays import batches
    assert batches(1073, 256) == [(0, 256), (256, 256), (512, 256), (768, 256), (1024, 49)]
    assert batches(1024, 256) == [(0, 256), (256, 256), (512, 256), (768, 256)]          # no empty tail
    assert batches(1073, 5000) == [(0, 1073)]                                            # a batch larger than the image
    assert batches(1073, 1073) == [(0, 1073)]
    assert batches(3, 1) == [(0, 1), (1, 1), (2, 1)]                                     # a batch of 1
    assert batches(1, 1) == [(0, 1)]
    for P, B in ((1073, 64), (1073, 1072), (7, 3)):
        spans = batches(P, B)
        assert [b for b, _ in spans] == list(range(0, P, B)) and sum(n for _, n in spans) == P and all(1 <= n <= B for _, n in spans)
    for bad in ((0, 4), (4, 0), (4, -1)):
        with pytest.raises(ValueError):
            batches(*bad)


def _cam_struct(W=37, H=29):
    from switch_nerf_amd.rays import Camera
    return Camera(W, H, [40.0, 43.5, 17.25, 15.625], torch.eye(4)[:3], 5).struct(True)


def test_c_entries_refuse_before_launch():
    """Each -1 path of the four entries, without a GPU (fake non-null pointers are never dereferenced on the host)."""
    from switch_nerf_amd import _lib
    lib = _lib.load()
    p, q = C.c_void_p(0x1000), C.c_void_p(0x1004)
    err = lambda: lib.swn_last_error().decode()
    cam = _cam_struct()
    alt, flat, desc = (C.c_float * 2)(-0.5, 0.3), (C.c_float * 2)(0.3, 0.3), (C.c_float * 2)(0.3, -0.5)
    f = lib.swn_rays_from_camera
    assert f(None, 0.1, 10.0, None, 0, 10, p, None, None) == -1 and "null pointer" in err()
    assert f(C.byref(cam), 0.1, 10.0, None, 0, 10, None, None, None) == -1 and "null pointer" in err()
    assert f(C.byref(cam), 0.1, 10.0, None, 0, 0, p, None, None) == -1 and "n must be positive" in err()
    assert f(C.byref(cam), 0.1, 10.0, None, 0, -3, p, None, None) == -1 and "n must be positive" in err()
    assert f(C.byref(cam), 0.1, 10.0, None, 1000, 74, p, None, None) == -1 and "outside the image's 1073 pixels" in err()
    assert f(C.byref(cam), 0.1, 10.0, None, -1, 10, p, None, None) == -1 and "outside the image" in err()
    assert f(C.byref(cam), 0.1, 10.0, None, 1073, 1, p, None, None) == -1 and "outside the image" in err()
    assert f(C.byref(cam), 0.1, 10.0, desc, 0, 10, p, None, None) == -1 and "ascending" in err()
    assert f(C.byref(cam), 0.1, 10.0, flat, 0, 10, p, None, None) == -1 and "ascending" in err()
    assert f(C.byref(cam), 10.5, 10.0, alt, 0, 10, p, None, None) == -1 and "near 10.5 > far 10" in err()
    assert f(C.byref(cam), 0.1, 10.0, alt, 0, 10, q, None, None) == -1 and "misaligned" in err()
    bad = _cam_struct()
    bad.W = 0
    assert f(C.byref(bad), 0.1, 10.0, None, 0, 10, p, None, None) == -1 and "bad image size" in err()
    f = lib.swn_ray_directions
    assert f(37, 29, 40.0, 43.5, 17.25, 15.625, 1, None, None) == -1 and "null pointer" in err()
    assert f(0, 29, 40.0, 43.5, 17.25, 15.625, 1, p, None) == -1 and "bad image size" in err()
    assert f(37, -1, 40.0, 43.5, 17.25, 15.625, 1, p, None) == -1 and "bad image size" in err()
    f = lib.swn_rays_from_directions
    assert f(None, p, 1, 10, 0.1, 10.0, None, p, None) == -1 and "null pointer" in err()
    assert f(p, None, 1, 10, 0.1, 10.0, None, p, None) == -1 and "null pointer" in err()
    assert f(p, p, 1, 10, 0.1, 10.0, None, None, None) == -1 and "null pointer" in err()
    assert f(p, p, 1, 0, 0.1, 10.0, None, p, None) == -1 and "n must be positive" in err()
    assert f(p, p, 0, 10, 0.1, 10.0, None, p, None) == -1 and "cameras" in err()
    assert f(p, p, 1, 10, 0.1, 10.0, desc, p, None) == -1 and "ascending" in err()
    assert f(p, p, 1, 10, 0.2, 0.1, None, p, None) == -1 and "near 0.2 > far 0.1" in err()
    assert f(p, q, 1, 10, 0.1, 10.0, None, p, None) == -1 and "misaligned" in err()
    f = lib.swn_rays_from_pixels
    for i64 in (0, 1):
        assert f(None, 3, p, p, i64, 10, 37, 29, 1, 0.1, 10.0, None, p, None) == -1 and "null pointer" in err()
        assert f(p, 3, None, p, i64, 10, 37, 29, 1, 0.1, 10.0, None, p, None) == -1 and "null pointer" in err()
        assert f(p, 3, p, None, i64, 10, 37, 29, 1, 0.1, 10.0, None, p, None) == -1 and "null pointer" in err()
        assert f(p, 3, p, p, i64, 10, 37, 29, 1, 0.1, 10.0, None, None, None) == -1 and "null pointer" in err()
        assert f(p, 3, p, p, i64, 0, 37, 29, 1, 0.1, 10.0, None, p, None) == -1 and "n must be positive" in err()
        assert f(p, 0, p, p, i64, 10, 37, 29, 1, 0.1, 10.0, None, p, None) == -1 and "bad sizes" in err()
        assert f(p, 3, p, p, i64, 10, 37, 0, 1, 0.1, 10.0, None, p, None) == -1 and "bad sizes" in err()
        assert f(p, 3, p, p, i64, 10, 37, 29, 1, 0.1, 10.0, desc, p, None) == -1 and "ascending" in err()
        assert f(p, 3, p, p, i64, 10, 37, 29, 1, 0.2, 0.1, alt, p, None) == -1 and "near 0.2 > far 0.1" in err()
    assert f(p, 3, p, p, 0, 10, 1 << 16, 1 << 16, 1, 0.1, 10.0, None, p, None) == -1 and "outside int32 indices" in err()
    assert f(p, 3, q, q, 1, 10, 37, 29, 1, 0.1, 10.0, None, p, None) == -1 and "misaligned" in err()


def test_wrappers_raise_value_errors():
    from switch_nerf_amd import rays
    cam = rays.Camera(37, 29, [40.0, 43.5, 17.25, 15.625], torch.eye(4)[:3], 5)
    for kw in (dict(pixel_begin=1000, n=74), dict(pixel_begin=-1, n=4), dict(pixel_begin=1073), dict(n=0), dict(n=-2)):
        with pytest.raises(ValueError, match="pixel range"):
            rays.camera_rays(cam, 0.1, 10.0, None, True, **kw)
    with pytest.raises(ValueError, match="near 2.0 > far 1.0"):
        rays.camera_rays(cam, 2.0, 1.0)
    for alt in ([0.3, -0.5], [0.3, 0.3], [0.1], [0.1, 0.2, 0.3]):
        with pytest.raises(ValueError, match="ascending pair"):
            rays.camera_rays(cam, 0.1, 10.0, alt)
    with pytest.raises(ValueError, match="bad image size"):
        rays.get_ray_directions(0, 29, 40.0, 43.5, 17.25, 15.625, True, "cpu")
    d = torch.zeros(29, 37, 3)
    with pytest.raises(ValueError, match=r"c2w must be \[3, 4\]"):
        rays.get_rays(d, torch.eye(4), 0.1, 10.0, None)
    with pytest.raises(ValueError, match="non-empty fp32 tensor"):
        rays.get_rays(d.double(), torch.eye(4)[:3], 0.1, 10.0, None)
    with pytest.raises(ValueError, match="non-empty fp32 tensor"):
        rays.get_rays(torch.zeros(5, 4), torch.eye(4)[:3], 0.1, 10.0, None)
    with pytest.raises(ValueError, match="there is no CPU path"):
        rays.get_rays(d, torch.eye(4)[:3], 0.1, 10.0, None)
    with pytest.raises(ValueError, match="ascending pair"):
        rays.get_rays(d, torch.eye(4)[:3], 0.1, 10.0, [0.3, -0.5])
    with pytest.raises(ValueError, match=r"directions \[P, 3\] and c2w \[K, 3, 4\]"):
        rays.get_rays_batch(d, torch.eye(4)[:3][None], 0.1, 10.0, None)
    with pytest.raises(ValueError, match=r"directions \[P, 3\] and c2w \[K, 3, 4\]"):
        rays.get_rays_batch(d.view(-1, 3), torch.eye(4)[:3], 0.1, 10.0, None)
    with pytest.raises(ValueError, match="there is no CPU path"):
        rays.get_rays_batch(d.view(-1, 3), torch.eye(4)[:3][None], 0.1, 10.0, None)
    table = rays.camera_table([cam, cam], device="cpu")
    ci, pi = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match=r"\[M, 16\]"):
        rays.pixel_rays(table[:, :12], ci, pi, 37, 29, 0.1, 10.0)
    with pytest.raises(ValueError, match="share dtype and shape"):
        rays.pixel_rays(table, ci, pi.long(), 37, 29, 0.1, 10.0)
    with pytest.raises(ValueError, match="share dtype and shape"):
        rays.pixel_rays(table, ci, pi[:3], 37, 29, 0.1, 10.0)
    with pytest.raises(ValueError, match="share dtype and shape"):
        rays.pixel_rays(table, ci[:0], pi[:0], 37, 29, 0.1, 10.0)
    with pytest.raises(ValueError, match="int32 or int64"):
        rays.pixel_rays(table, ci.float(), pi.float(), 37, 29, 0.1, 10.0)
    with pytest.raises(ValueError, match="bad image size"):
        rays.pixel_rays(table, ci, pi, 37, 0, 0.1, 10.0)
    with pytest.raises(ValueError, match="near 2.0 > far 1.0"):
        rays.pixel_rays(table, ci, pi, 37, 29, 2.0, 1.0)
    with pytest.raises(ValueError, match="there is no CPU path"):
        rays.pixel_rays(table, ci, pi, 37, 29, 0.1, 10.0)
    with pytest.raises(ValueError, match="no cameras"):
        rays.camera_table([])
    with pytest.raises(ValueError, match="share W and H"):
        rays.camera_table([cam, rays.Camera(36, 29, [40.0, 43.5], torch.eye(4)[:3])], device="cpu")
    with pytest.raises(ValueError, match=r"c2w must be \[3, 4\]"):
        rays.Camera(37, 29, [40.0, 43.5], torch.eye(4))
    with pytest.raises(ValueError, match="intrinsics"):
        rays.Camera(37, 29, [40.0, 43.5, 1.0], torch.eye(4)[:3])
    with pytest.raises(ValueError, match="bad image size"):
        rays.Camera(0, 29, [40.0, 43.5], torch.eye(4)[:3])


def test_camera_and_table_layouts():
    """Camera.struct is swn_camera field for field (c2w row-major, intrinsics, sizes, flag, the int64 index at byte 80); a table row is
    c2w then fx, fy, cx, cy; two intrinsics centre the principal point as the reference's ImageMetadata does."""
    from switch_nerf_amd import _lib, rays
    c2w = torch.arange(12, dtype=torch.float64).view(3, 4) / 8
    cam = rays.Camera(37, 29, torch.tensor([40.0, 43.5, 17.25, 15.625]), c2w, 1 << 40)
    assert cam.c2w.dtype == torch.float32 and cam.c2w.device.type == "cpu" and cam.image_index == 1 << 40
    s = cam.struct(False)
    assert C.sizeof(_lib.Camera) == 88 and _lib.Camera.image_index.offset == 80 and _lib.Camera.fx.offset == 48 and _lib.Camera.W.offset == 64
    assert list(s.c2w) == [k / 8 for k in range(12)] and (s.fx, s.fy, s.cx, s.cy) == (40.0, 43.5, 17.25, 15.625)
    assert (s.W, s.H, s.center_pixels, s.image_index) == (37, 29, 0, 1 << 40) and cam.struct(True).center_pixels == 1
    other = rays.Camera(37, 29, [50.0, 60.0], -c2w, 2)
    assert other.intrinsics.tolist() == [50.0, 60.0, 18.5, 14.5]
    table = rays.camera_table([cam, other], device="cpu")
    assert table.shape == (2, 16) and table.dtype == torch.float32 and table.is_contiguous()
    assert table[0].tolist() == [k / 8 for k in range(12)] + [40.0, 43.5, 17.25, 15.625]
    assert table[1].tolist() == [-k / 8 for k in range(12)] + [50.0, 60.0, 18.5, 14.5]


def test_render_image_refuses_training_mode():
    from switch_nerf_amd import rays, rendering
    cam = rays.Camera(37, 29, [40.0, 43.5], torch.eye(4)[:3])
    hp = SimpleNamespace(image_pixel_batch_size=256)
    with pytest.raises(RuntimeError, match="nerf is in training mode"):
        rendering.render_image(SimpleNamespace(training=True), None, cam, hp, 0.1, 10.0)
    with pytest.raises(RuntimeError, match="bg_nerf is in training mode"):
        rendering.render_image(SimpleNamespace(training=False), SimpleNamespace(training=True), cam, hp, 0.1, 10.0)
    with pytest.raises(RuntimeError, match="training mode"):
        rendering.validate_image(SimpleNamespace(training=True), None, cam, torch.zeros(29, 37, 3), hp, 0.1, 10.0)
