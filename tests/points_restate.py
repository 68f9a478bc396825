"""numpy restatement of the reference's point export (Runner._run_validation_points, runner.py:2024-2142), used by the point tests:
strided slice [:, ::skip], (x * 255).astype(uint8) on float32, records as numpy structured arrays, stable boolean masks by expert.
Also a minimal reader of the binary PLY files the export writes."""
import numpy as np

RGBA, SEG_ALPHA, SEG_RGB = 0, 1, 2          # switch_nerf_amd.ops.PLY_* (swn_points_pack modes)
XYZ = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
DTYPES = {RGBA: np.dtype(XYZ + [("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")]),
          SEG_ALPHA: np.dtype(XYZ + [("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")]),
          SEG_RGB: np.dtype(XYZ + [("red", "u1"), ("green", "u1"), ("blue", "u1")])}


def q8(x):
    """(x * 255).to(torch.uint8) on float32."""
    return (np.asarray(x, np.float32) * np.float32(255)).astype(np.uint8)


def records(mode, pts, pts_alpha, skip=1, idx=None, pts_rgb=None, pixel_rgb=None, palette=None):
    """The kept samples' records [R * ceil(S / skip)] (ray-major, sample-minor)."""
    pts = np.asarray(pts, np.float32)[:, ::skip]
    R, Sk = pts.shape[:2]
    rec = np.empty(R * Sk, DTYPES[mode])
    for i, c in enumerate("xyz"):
        rec[c] = pts[..., i].reshape(-1)
    if mode == RGBA:
        cols = np.concatenate([q8(np.asarray(pts_rgb)[:, ::skip]), q8(np.asarray(pts_alpha)[:, ::skip])[..., None]], -1)
    else:
        e = np.asarray(idx).reshape(R, -1)[:, ::skip]
        seg = np.zeros((R, Sk, 3), np.uint8)
        for x in range(len(palette)):
            seg[e == x] = palette[x]
        if mode == SEG_ALPHA:
            cols = np.concatenate([seg, q8(np.asarray(pts_alpha)[:, ::skip])[..., None]], -1)
        else:
            seg[:, -1] = q8(pixel_rgb)
            cols = seg
    for i, c in enumerate(DTYPES[mode].names[3:]):
        rec[c] = cols[..., i].reshape(-1)
    return rec


def by_expert(rec, idx, skip, n_experts):
    """[records of expert 0, of expert 1, ...] with the reference's boolean masks (stable)."""
    R = idx.shape[0]
    e = np.asarray(idx).reshape(R, -1)[:, ::skip].reshape(-1)
    return [rec[e == x] for x in range(n_experts)]


def read_ply(path):
    """-> (header lines, structured array of the vertices)."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")[:-1]
    names = [ln.split()[-1] for ln in lines if ln.startswith("property")]
    mode = RGBA if names[-1] == "alpha" else SEG_RGB
    body = np.frombuffer(data[end:], DTYPES[mode])
    n = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[-1])
    assert body.shape[0] == n, (path, n, body.shape)
    return lines, body
