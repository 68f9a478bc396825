"""CPU-only: the PLY writer of the point-cloud export (switch_nerf_amd/points.py) and the numpy restatement the GPU point tests
compare against (tests/points_restate.py)."""
import os

import numpy as np

import points_restate as PR


def test_ply_header_text_all_modes():
    from switch_nerf_amd import points, ops
    rgba = points.ply_header(7, ops.PLY_RGBA)
    assert rgba == (b"ply\nformat binary_little_endian 1.0\nelement vertex 7\nproperty float x\nproperty float y\n"
                    b"property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n"
                    b"end_header\n")
    assert points.ply_header(7, ops.PLY_SEG_ALPHA) == rgba
    assert points.ply_header(0, ops.PLY_SEG_RGB) == (b"ply\nformat binary_little_endian 1.0\nelement vertex 0\nproperty float x\n"
                                                     b"property float y\nproperty float z\nproperty uchar red\n"
                                                     b"property uchar green\nproperty uchar blue\nend_header\n")
    assert (ops.PLY_RGBA, ops.PLY_SEG_ALPHA, ops.PLY_SEG_RGB) == (PR.RGBA, PR.SEG_ALPHA, PR.SEG_RGB)
    assert [ops.PLY_RECORD_BYTES[m] for m in (PR.RGBA, PR.SEG_ALPHA, PR.SEG_RGB)] == [PR.DTYPES[m].itemsize for m in (0, 1, 2)]


def _hand_arrays():
    # 2 rays x 5 samples
    pts = np.arange(30, dtype=np.float32).reshape(2, 5, 3) * np.float32(0.5) - 3
    rgb = np.tile(np.array([0.0, 0.5, 1.0], np.float32), (2, 5, 1))
    rgb[1, :, 0] = 0.2
    alpha = np.array([[0, 0.25, 0.5, 0.75, 1], [1, 0.1, 0.2, 0.3, 0.4]], np.float32)
    idx = np.array([[0, 2, 2, 1, 0], [2, 2, 0, 1, 1]], np.int32)
    pixel = np.array([[1.0, 0.5, 0.0], [0.2, 0.2, 0.2]], np.float32)
    palette = np.array([[128, 0, 0], [0, 128, 0], [128, 128, 0]], np.uint8)
    return pts, rgb, alpha, idx, pixel, palette


def test_restatement_on_hand_checked_example():
    pts, rgb, alpha, idx, pixel, palette = _hand_arrays()
    # (x * 255) truncated: 0.5 -> 127.5 -> 127, 0.2 -> 51, 0.25 -> 63, 0.75 -> 191, 0.1 -> 25, 0.3 -> 76, 0.4 -> 102
    assert PR.q8([0.0, 0.5, 1.0, 0.2, 0.25, 0.75, 0.1, 0.3, 0.4]).tolist() == [0, 127, 255, 51, 63, 191, 25, 76, 102]
    rec = PR.records(PR.RGBA, pts, alpha, 2, pts_rgb=rgb)                 # samples 0, 2, 4 of each ray
    assert rec.shape == (6,) and rec.dtype.itemsize == 16
    assert rec["x"].tolist() == [-3.0, 0.0, 3.0, 4.5, 7.5, 10.5]
    assert rec["z"].tolist() == [-2.0, 1.0, 4.0, 5.5, 8.5, 11.5]
    assert rec["red"].tolist() == [0, 0, 0, 51, 51, 51] and rec["green"].tolist() == [127] * 6 and rec["blue"].tolist() == [255] * 6
    assert rec["alpha"].tolist() == [0, 127, 255, 255, 51, 102]
    parts = PR.by_expert(rec, idx, 2, 3)                                  # kept experts: [0, 2, 0], [2, 0, 1]
    assert [p["x"].tolist() for p in parts] == [[-3.0, 3.0, 7.5], [10.5], [0.0, 4.5]]
    seg = PR.records(PR.SEG_ALPHA, pts, alpha, 2, idx=idx, palette=palette)
    assert seg["red"].tolist() == [128, 128, 128, 128, 128, 0] and seg["green"].tolist() == [0, 128, 0, 128, 0, 128]
    assert seg["alpha"].tolist() == rec["alpha"].tolist()
    segr = PR.records(PR.SEG_RGB, pts, alpha, 2, idx=idx, pixel_rgb=pixel, palette=palette)
    assert segr.dtype.itemsize == 15
    # the last kept sample of each ray carries the pixel colour
    assert [tuple(r)[3:] for r in segr] == [(128, 0, 0), (128, 128, 0), (255, 127, 0), (128, 128, 0), (128, 0, 0), (51, 51, 51)]


def test_writer_body_bytes_all_modes(tmp_path):
    from switch_nerf_amd import points
    pts, rgb, alpha, idx, pixel, palette = _hand_arrays()
    for mode in (PR.RGBA, PR.SEG_ALPHA, PR.SEG_RGB):
        rec = PR.records(mode, pts, alpha, 1, idx=idx, pts_rgb=rgb, pixel_rgb=pixel, palette=palette)
        p = str(tmp_path / f"m{mode}.ply")
        w = points.PlyWriter(p, mode)
        w.append(rec.view(np.uint8))
        assert w.close() == 10
        data = open(p, "rb").read()
        hdr = points.ply_header(10, mode)
        assert data[:len(hdr)] == hdr and data[len(hdr):] == rec.tobytes()
        lines, body = PR.read_ply(p)
        assert lines[2] == "element vertex 10" and np.array_equal(body, rec)
    # the first record by hand: x y z = -3 -2.5 -2 (f4 little endian), rgba = 0 127 255 0
    first = open(str(tmp_path / "m0.ply"), "rb").read()[len(points.ply_header(10, 0)):][:16]
    assert first == np.array([-3.0, -2.5, -2.0], "<f4").tobytes() + bytes([0, 127, 255, 0])
    assert not [f for f in os.listdir(tmp_path) if f.startswith(".spool_")]


def test_spooling_ragged_batches_equals_one_batch(tmp_path):
    from switch_nerf_amd import points
    rng = np.random.default_rng(3)
    R, S = 37, 11
    pts = rng.standard_normal((R, S, 3)).astype(np.float32)
    rgb = rng.uniform(0, 1, (R, S, 3)).astype(np.float32)
    alpha = rng.uniform(0, 1, (R, S)).astype(np.float32)
    one = points.PlyWriter(str(tmp_path / "one.ply"), PR.RGBA)
    one.append(PR.records(PR.RGBA, pts, alpha, 3, pts_rgb=rgb).view(np.uint8))
    many = points.PlyWriter(str(tmp_path / "many.ply"), PR.RGBA)
    for a, b in ((0, 10), (10, 11), (11, 11), (11, 30), (30, 37)):            # ragged, one empty batch
        many.append(PR.records(PR.RGBA, pts[a:b], alpha[a:b], 3, pts_rgb=rgb[a:b]).view(np.uint8))
    assert one.close() == many.close() == R * 4
    assert open(tmp_path / "one.ply", "rb").read() == open(tmp_path / "many.ply", "rb").read()
    empty = points.PlyWriter(str(tmp_path / "empty.ply"), PR.SEG_RGB)
    assert empty.close() == 0
    assert open(tmp_path / "empty.ply", "rb").read() == points.ply_header(0, PR.SEG_RGB)


def test_file_name_set():
    from switch_nerf_amd import points
    assert points.point_file_names(3, "coarse", 2, False) == ["003_coarse_pts_rgba.ply", "003_coarse_pts_rgba_top_0_exp_0.ply",
                                                              "003_coarse_pts_rgba_top_0_exp_1.ply"]
    names = points.point_file_names(12, "fine", 2, True)
    assert names == ["012_fine_pts_rgba.ply", "012_fine_pts_rgba_top_0_exp_0.ply", "012_fine_pts_rgba_top_0_exp_1.ply",
                     "012_fine_top_0_alpha.ply", "012_fine_top_0_alpha_exp_0.ply", "012_fine_top_0_alpha_exp_1.ply",
                     "012_fine_top_0.ply", "012_fine_top_0_exp_0.ply", "012_fine_top_0_exp_1.ply"]
    assert points.point_file_names(0, "coarse", 8, True, moe=False) == ["000_coarse_pts_rgba.ply"]
    groups = points._groups(12, "fine", 2, True, True)
    assert sorted([g[1] for g in groups] + sum([g[2] for g in groups], [])) == sorted(names)
    assert points.VOC_PALETTE[0].tolist() == [128, 0, 0] and points.VOC_PALETTE.shape == (20, 3)
