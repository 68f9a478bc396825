"""fp64 restatement of the reference's ray_utils.py (get_ray_directions, get_rays / get_rays_batch, _get_rays_inner) in numpy: what
the fixture tests/golden/raygen.npz and the device kernels (switch_nerf_amd/csrc/raygen.hip) are measured against.  The inputs
(intrinsics, poses, near, far, altitudes) are the fp32 values the reference and the device see, widened to fp64; every operation
after that is fp64."""
import numpy as np

MARGIN = 4.0          # the device's bound = MARGIN x the reference's own measured fp32 error (a different but equally valid fp32 order)
CLEAR = 1e-4          # the fixture keeps |d.x| and |o.x - altitude| at least this far from the two branch conditions


def f64(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def directions(W, H, fx, fy, cx, cy, center_pixels):
    """-> [H, W, 3] unit camera-space directions."""
    fx, fy, cx, cy = (float(np.float32(v)) for v in (fx, fy, cx, cy))
    i, j = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="xy")
    if center_pixels:
        i, j = i + 0.5, j + 0.5
    d = np.stack([(i - cx) / fx, -(j - cy) / fy, -np.ones_like(i)], -1)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def plane_bound(o, d, alt, bound):
    """_truncate_with_plane_intersection on [..., 3] arrays -> (bound, the rays it set)."""
    alt = float(np.float32(alt))
    hit = (o[..., 0] < alt) & (d[..., 0] > 0)
    n = np.array([-1.0, 0.0, 0.0])
    pp = np.array([alt, 0.0, 0.0])
    with np.errstate(divide="ignore", invalid="ignore"):
        w = o - pp
        si = -(w @ n) / (d @ n)
        p = w + si[..., None] * d + pp
        dist = np.linalg.norm(o - p, axis=-1)
    return np.where(hit, dist, bound), hit


def rays(dirs, c2w, near, far, altitude_range=None):
    """dirs [..., 3] (camera space, unit), c2w [3, 4] -> (rays [..., 8], near-plane branch [...], far-plane branch [...])."""
    c2w = f64(c2w)
    near, far = float(np.float32(near)), float(np.float32(far))
    d = dirs @ c2w[:, :3].T
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.broadcast_to(c2w[:, 3], d.shape)
    nb, fb = np.full(d.shape[:-1], near), np.full(d.shape[:-1], far)
    hit_n = hit_f = np.zeros(d.shape[:-1], bool)
    if altitude_range is not None:
        nb, hit_n = plane_bound(o, d, altitude_range[0], nb)
        nb = np.maximum(nb, near)
        fb, hit_f = plane_bound(o, d, altitude_range[1], fb)
        fb = np.minimum(fb, far)
        fb = np.maximum(nb, fb)
    return np.concatenate([o, d, nb[..., None], fb[..., None]], -1), hit_n, hit_f


def branches(r, altitude_range):
    """The two branch decisions read off finished rays [..., 8] (fp32 or fp64): (o.x < a0) & (d.x > 0), (o.x < a1) & (d.x > 0)."""
    r = np.asarray(r)
    down = r[..., 3] > 0
    return tuple((r[..., 0] < np.float32(a)) & down for a in altitude_range)


def errors(got, want):
    """got fp32 rays [..., 8] against the restatement's `want` -> dict: origins exact?, max abs direction error, max relative near / far
    error."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    rel = lambda k: float(np.max(np.abs(got[..., k] - want[..., k]) / np.abs(want[..., k])))
    return dict(origin_exact=bool(np.array_equal(got[..., :3], want[..., :3])), dir=float(np.max(np.abs(got[..., 3:6] - want[..., 3:6]))),
                near=rel(6), far=rel(7))


# ---- the fixture's cases (tests/golden/raygen.npz, scripts/gen_golden_raygen.py)
CASES = ["plain_center", "plain_corner", "above_down", "oblique_horizon", "between", "below", "near_beyond_far"]


def intr(g):
    return [float(v) for v in g["intrinsics"]]


def want_case(g, name):
    W, H = int(g["W"]), int(g["H"])
    alt = g[f"{name}_alt"] if f"{name}_alt" in g.files else None
    d = directions(W, H, *intr(g), bool(g[f"{name}_center"]))
    return rays(d, g[f"{name}_c2w"], g[f"{name}_near"], g[f"{name}_far"], alt), alt


def want_batch(g):
    W, H = int(g["W"]), int(g["H"])
    d = directions(W, H, *intr(g), True).reshape(-1, 3)[g["batch_pix"]]
    return [rays(d, c, g["batch_near"], g["batch_far"], g["batch_alt"]) for c in g["batch_c2w"]]
