"""Restatement of the NeRF-dataset ray recipe (switch_nerf_amd/nerf_rays.py over csrc/raygen_nerf.hip), written from the formulas in
numpy with ONE operation per line of arithmetic, in the dtype `dt` it is asked for: np.float32 restates the device kernels step by
step (every step a correctly rounded IEEE operation, so numpy on the host gives the device's bits), np.float64 is the mathematics.

    camera dirs   c = ((i - cx) / fx, -(j - cy) / fy, -1) for the pixel (col i, row j): the pixel's corner, no centring
    get_rays      d = ((c0 r0 + c1 r1) + c2 r2 per row r of c2w[:, :3]),  o = c2w[:, 3]
    normalize     d / sqrt(fma(dz, dz, fma(dy, dy, dx dx))), each component divided: torch.norm's CPU kernel accumulates acc + v v
                  contracted to one fused multiply-add per element, which the kernels restate with explicit fmaf
    ndc_rays      t = -(near + oz) / dz;  o' = o + t d;  with cw = -1 / (W / (2 focal)), ch likewise (host doubles, rounded to dt):
                  o0 = (cw o'x) / o'z, o1 = (ch o'y) / o'z, o2 = 1 + (2 near) / o'z
                  d0 = cw (dx / dz - o'x / o'z), d1 = ch (dy / dz - o'y / o'z), d2 = (-2 near) / o'z
    bungee flat   near = max((250 s - oz s) / (dz s), 1e-6), far = (0 - oz s) / (dz s), s the scale rounded to dt
    bungee sphere with oc = o - globe, b = 2 ((oc0 d0 + oc1 d1) + oc2 d2), n2 = |d|^2, c = |oc|^2 - R^2:
                  delta = b b - (4 n2) c;  dist = (-b - sqrt(delta)) / (2 n2);  p = o + dist d;  near = |o - p| 0.9 (R with the
                  buildings' 250 m), far = |o - p| 1.1 (R the earth's).  The kernel forms dist in fp64 from its fp32 o, d and globe
                  (sphere_dist_dt=np.float64), the reference in its own dtype.
    radii         dx 2 / sqrt(12), dx(row r) = sqrt((qx qx + qy qy) + qz qz) with q = d(r) - d(r + 1) for r < H - 1; the last row takes
                  dx(H - 3), the reference's cat([dx, dx[:, -2:-1]]) (dx has H - 1 rows, so its row -2 is image row H - 3); with H = 2 that
                  slice is empty and the reference returns H - 1 rows - here the last row then takes dx(0), the only one there is
"""
import numpy as np

EARTH_RADIUS = 6371011
BUILDING_HEIGHT = 250
MODES = ("raw", "normalized", "ndc")


def _norm(x, y, z):
    xx = x * x
    yy = y * y
    zz = z * z
    return np.sqrt((xx + yy) + zz)


def camera_dirs(W, H, K, dt):
    """[H, W, 3] camera-space directions; K = (fx, fy, cx, cy)."""
    fx, fy, cx, cy = (dt(v) for v in K)
    i, j = np.meshgrid(np.arange(W).astype(dt), np.arange(H).astype(dt), indexing="xy")
    x = (i - cx) / fx
    y = -(j - cy) / fy
    return np.stack([x, y, -np.ones_like(x)], -1)


def get_rays(W, H, K, c2w, dt):
    """-> rays_o, rays_d, each [H, W, 3]."""
    c2w = np.asarray(c2w).astype(dt)
    c = camera_dirs(W, H, K, dt)
    d = np.stack([(c[..., 0] * c2w[r, 0] + c[..., 1] * c2w[r, 1]) + c[..., 2] * c2w[r, 2] for r in range(3)], -1)
    o = np.broadcast_to(c2w[:, 3], d.shape).copy()
    return o, d


def _fma(a, b, c):
    """fma(a, b, c) of fp32 arrays through double: a b is exact there, and the sum is rounded to double before fp32 - a second rounding
    that can differ from the fused one only on an fp32 tie of the 53-bit sum.  In fp64 (the yardstick) a plain a b + c."""
    if a.dtype == np.float32:
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    return a * b + c


def normalize(d):
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    n = np.sqrt(_fma(z, z, _fma(y, y, x * x)))
    return d / n[..., None]


def ndc_coefficients(W, H, focal, near, dt):
    """The four host scalars of ndc_rays, formed in double like the reference's Python floats and rounded once."""
    focal, near = float(focal), float(near)
    return dt(-1. / (W / (2. * focal))), dt(-1. / (H / (2. * focal))), dt(near), dt(2. * near)


def ndc_rays(W, H, focal, near, o, d, dt):
    cw, ch, nr, nr2 = ndc_coefficients(W, H, focal, near, dt)
    t = -(nr + o[..., 2]) / d[..., 2]
    o = o + t[..., None] * d
    oz = o[..., 2]
    o0 = (cw * o[..., 0]) / oz
    o1 = (ch * o[..., 1]) / oz
    o2 = dt(1) + nr2 / oz
    d0 = cw * (d[..., 0] / d[..., 2] - o[..., 0] / oz)
    d1 = ch * (d[..., 1] / d[..., 2] - o[..., 1] / oz)
    d2 = -nr2 / oz
    return np.stack([o0, o1, o2], -1), np.stack([d0, d1, d2], -1)


def globe_center(scene_scaling_factor, scene_origin):
    """fp32 in every dtype: the reference rounds it with .float()."""
    return (np.asarray(scene_origin, np.float64) * float(scene_scaling_factor)).astype(np.float32)


def flat_nearfar(o, d, scene_scaling_factor, dt):
    s = dt(scene_scaling_factor)
    p_near = dt(BUILDING_HEIGHT) * s
    den = d[..., 2] * s
    near = (p_near - o[..., 2] * s) / den
    far = (dt(0) - o[..., 2] * s) / den
    return np.maximum(near, dt(1e-6)), far


def sphere_nearfar(o, d, scene_scaling_factor, scene_origin, dt, sphere_dist_dt=None):
    """sphere_dist_dt: the dtype the distance along the ray is formed in (the kernel: np.float64 from dt inputs); None: dt itself."""
    w = dt if sphere_dist_dt is None else sphere_dist_dt
    g = globe_center(scene_scaling_factor, scene_origin).astype(w)
    ow, dw = o.astype(w), d.astype(w)
    oc = ow - g
    b = w(2) * ((oc[..., 0] * dw[..., 0] + oc[..., 1] * dw[..., 1]) + oc[..., 2] * dw[..., 2])
    n2 = (dw[..., 0] * dw[..., 0] + dw[..., 1] * dw[..., 1]) + dw[..., 2] * dw[..., 2]
    oc2 = (oc[..., 0] * oc[..., 0] + oc[..., 1] * oc[..., 1]) + oc[..., 2] * oc[..., 2]
    out = []
    for radius, k in ((EARTH_RADIUS + BUILDING_HEIGHT, 0.9), (EARTH_RADIUS, 1.1)):
        r = radius * float(scene_scaling_factor)
        delta = b * b - (w(4) * n2) * (oc2 - w(r * r))
        dist = ((-b - np.sqrt(delta)) / (w(2) * n2)).astype(dt)
        p = o + dist[..., None] * d
        q = o - p
        out.append(_norm(q[..., 0], q[..., 1], q[..., 2]) * dt(k))
    return out[0], out[1]


def radii(d, dt):
    """d [H, W, 3] normalised directions -> [H, W, 1]."""
    q = d[:-1] - d[1:]
    dx = _norm(q[..., 0], q[..., 1], q[..., 2])
    dx = np.concatenate([dx, dx[max(d.shape[0] - 3, 0)][None]], 0)
    return ((dx * dt(2)) / dt(np.sqrt(12)))[..., None]


def mode_rays(W, H, K, c2w, mode, near, far, dt, focal=None, near_ndc=1.0):
    """camera_rays: [H, W, 8]."""
    o, d = get_rays(W, H, K, c2w, dt)
    if mode == "normalized":
        d = normalize(d)
    elif mode == "ndc":
        o, d = ndc_rays(W, H, K[0] if focal is None else focal, near_ndc, o, d, dt)
    elif mode != "raw":
        raise ValueError(mode)
    nf = np.broadcast_to(np.array([near, far]).astype(dt), d.shape[:-1] + (2,))
    return np.concatenate([o, d, nf], -1)


def bungee_rays(W, H, K, c2w, scene_scaling_factor, scene_origin, ray_nearfar, dt, sphere_dist_dt=None):
    """-> rays [H, W, 8], radii [H, W, 1]."""
    o, d = get_rays(W, H, K, c2w, dt)
    d = normalize(d)
    if ray_nearfar == "sphere":
        near, far = sphere_nearfar(o, d, scene_scaling_factor, scene_origin, dt, sphere_dist_dt)
    elif ray_nearfar == "flat":
        near, far = flat_nearfar(o, d, scene_scaling_factor, dt)
    else:
        raise ValueError(ray_nearfar)
    return np.concatenate([o, d, near[..., None], far[..., None]], -1), radii(d, dt)


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def dist(a, b) -> float:
    """Largest absolute difference, in fp64."""
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def rel_dist(a, b) -> float:
    """Largest difference relative to |b|, in fp64 (near / far / radii: positive quantities of any magnitude)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / np.abs(b)).max())
