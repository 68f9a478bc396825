"""Rays the NeRF-dataset way on the device: the reference's datasets/nerf_data (ray_utils.get_rays / ndc_rays, nerf_loader.py's
normalisation and scalar near / far, load_bungee.get_bungee_nearfar_radii) over csrc/raygen_nerf.hip - the rays of the dense NeRF and
mip recipes (train_nerf, render_image_nerf, render_image_nerf_mip), as rays.py makes the Mega-NeRF ones.

    cam = PinholeCamera(W, H, K, c2w)                              # K 3x3 (fx, fy, cx, cy are read), c2w [3, 4] or [4, 4]
    rays = camera_rays(cam, "normalized", near, far)                                   # [H * W, 8], one launch (Blender, LLFF no_ndc)
    rays = camera_rays(cam, "ndc", 0.0, 1.0, focal=focal)                              # LLFF forward-facing (near_ndc = 1)
    rays, radii = bungee_rays(cam, scene_scaling_factor, scene_origin, "sphere")       # [H * W, 8], [H * W, 1]
    camera_rays(cam, "normalized", near, far, pixel_begin=b, n=n, out=static_rays)     # a pixel batch into a caller's buffer
    table = camera_table(cameras)                                  # [M, 16] on the device, once per dataset
    rays, radii = pixel_rays(table, cam_idx, pix_idx, W, H, "sphere", scene_scaling_factor=s, scene_origin=o)     # a training batch

get_rays / ndc_rays keep the reference's signatures and return shapes and run as its two steps; the fused and gather forms give the
same bits.  The pixel's corner is used and the camera direction is not normalised (ray_utils.py:14-24) - unlike rays.py, which centres
the pixel and normalises twice.  Everything is fp32 (the bungee loader's float64 poses are rounded: DESIGN.md section 8); there is no
CPU path and no backward.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from . import _lib, ops
from .rays import _need_device, batches  # noqa: F401  (batches: the pixel-batch walk shared with rays.py)

MODES = {"raw": _lib.NERF_RAW, "normalized": _lib.NERF_NORMALIZED, "ndc": _lib.NERF_NDC}
NEARFAR = {"sphere": _lib.NERF_SPHERE, "flat": _lib.NERF_FLAT}
_PIXEL_MODES = dict(MODES, sphere=_lib.NERF_BUNGEE_SPHERE, flat=_lib.NERF_BUNGEE_FLAT)


def _host_f32(x, name: str, shapes) -> torch.Tensor:
    t = torch.as_tensor(x).detach().to("cpu", torch.float32)
    if tuple(t.shape) not in shapes:
        raise ValueError(f"{name} must be {' or '.join(str(list(s)) for s in shapes)}, got {list(t.shape)}")
    return t


class PinholeCamera:
    """A plain holder: W, H, K [3, 3] (the reference reads K[0][0], K[1][1], K[0][2], K[1][2]) and c2w [3, 4] (a [4, 4] pose gives its
    first three rows), both fp32 on the host."""

    def __init__(self, W: int, H: int, K, c2w):
        self.W, self.H = int(W), int(H)
        if self.W < 1 or self.H < 1:
            raise ValueError(f"PinholeCamera: bad image size (W {W}, H {H})")
        self.K = _host_f32(K, "PinholeCamera: K", ((3, 3),)).contiguous()
        self.c2w = _host_f32(c2w, "PinholeCamera: c2w", ((3, 4), (4, 4)))[:3].contiguous()

    @property
    def intrinsics(self) -> torch.Tensor:
        """fx, fy, cx, cy"""
        return torch.stack([self.K[0, 0], self.K[1, 1], self.K[0, 2], self.K[1, 2]])

    def struct(self) -> "_lib.NerfCamera":
        """The camera as the library takes it by value (swn_nerf_camera, include/swn.h)."""
        c = _lib.NerfCamera()
        c.c2w[:] = self.c2w.reshape(-1).tolist()
        c.fx, c.fy, c.cx, c.cy = self.intrinsics.tolist()
        c.W, c.H = self.W, self.H
        return c

    def row(self) -> torch.Tensor:
        """The camera's row of a camera table: c2w row-major, then fx, fy, cx, cy (16 floats, host)."""
        return torch.cat([self.c2w.reshape(-1), self.intrinsics])


def _pixel_range(camera: PinholeCamera, pixel_begin, n) -> Tuple[int, int]:
    P = camera.W * camera.H
    pixel_begin = int(pixel_begin)
    n = P - pixel_begin if n is None else int(n)
    if n < 1 or pixel_begin < 0 or pixel_begin + n > P:
        raise ValueError(f"pixel range [{pixel_begin}, {pixel_begin + n}) outside the image's {P} pixels (or empty)")
    return pixel_begin, n


def _mode(mode, table=MODES, what="mode") -> int:
    if mode not in table:
        raise ValueError(f"unknown {what} {mode!r}: one of {sorted(table)}")
    return table[mode]


def _check_nearfar(near, far):
    if not float(near) <= float(far):
        raise ValueError(f"near {near} > far {far}")


def _check_bungee(H: int, scene_scaling_factor, scene_origin):
    if int(H) < 2:
        raise ValueError(f"the bungee radii difference two image rows: H must be at least 2, got {H}")
    if not float(scene_scaling_factor) > 0:
        raise ValueError(f"scene_scaling_factor must be positive, got {scene_scaling_factor}")
    if len(list(scene_origin)) != 3:
        raise ValueError("scene_origin must have three values")


def get_rays(H: int, W: int, K, c2w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """ray_utils.get_rays: K [3, 3] and ONE pose c2w ([3, 4] or [4, 4], a DEVICE tensor as in the reference, whose grid lives on
    c2w.device) -> raw rays_o, rays_d, each [H, W, 3] fp32.  No host read: K and the pose travel as one 16-float device row."""
    if int(H) < 1 or int(W) < 1:
        raise ValueError(f"bad image size (W {W}, H {H})")
    K = torch.as_tensor(K)
    if tuple(K.shape) != (3, 3):
        raise ValueError(f"K must be [3, 3], got {list(K.shape)}")
    if not torch.is_tensor(c2w) or tuple(c2w.shape) not in ((3, 4), (4, 4)):
        raise ValueError(f"c2w must be a tensor [3, 4] or [4, 4], got {list(getattr(c2w, 'shape', []))}")
    _need_device(c2w, "c2w")
    K = K.detach().to(c2w.device, torch.float32)
    row = torch.cat([c2w.detach()[:3].to(torch.float32).reshape(-1), torch.stack([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])]).contiguous()
    return ops.nerf_rays_dirs(row, W, H)


def ndc_rays(H: int, W: int, focal: float, near: float, rays_o: torch.Tensor, rays_d: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """ray_utils.ndc_rays over fp32 device tensors [..., 3] -> (rays_o, rays_d) of the same shape."""
    for name, t in (("rays_o", rays_o), ("rays_d", rays_d)):
        if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.dim() >= 1 and t.shape[-1] == 3 and t.numel() > 0):
            raise ValueError(f"{name} must be a non-empty fp32 tensor [..., 3]")
    if rays_o.shape != rays_d.shape or rays_o.device != rays_d.device:
        raise ValueError("rays_o and rays_d must share shape and device")
    if int(H) < 1 or int(W) < 1:
        raise ValueError(f"bad image size (W {W}, H {H})")
    if not float(focal) > 0:
        raise ValueError(f"focal must be positive, got {focal}")
    _need_device(rays_o, "rays_o")
    o, d = ops.nerf_ndc(rays_o.reshape(-1, 3).contiguous(), rays_d.reshape(-1, 3).contiguous(), W, H, focal, near)
    return o.view(rays_o.shape), d.view(rays_d.shape)


def camera_rays(camera: PinholeCamera, mode: str, near: float, far: float, focal: Optional[float] = None, near_ndc: float = 1.0,
                pixel_begin: int = 0, n: Optional[int] = None, out: Optional[torch.Tensor] = None, device=None) -> torch.Tensor:
    """The rays [n, 8] of the row-major pixels [pixel_begin, pixel_begin + n) of `camera` (n None: to the end of the image) in ONE
    launch.  mode: "raw" (get_rays only), "normalized" (rays_d / norm: nerf_loader.py:160) or "ndc" (ndc_rays(H, W, focal, near_ndc):
    nerf_loader.py:158; focal None: K[0][0]).  Columns 6, 7 are near / far (nerf_loader.py:173).  out: a caller's contiguous fp32
    [n, 8] device buffer, written in place and returned (a captured graph's static input)."""
    m = _mode(mode)
    pixel_begin, n = _pixel_range(camera, pixel_begin, n)
    _check_nearfar(near, far)
    focal = float(camera.K[0, 0]) if focal is None else float(focal)
    if m == _lib.NERF_NDC and not focal > 0:
        raise ValueError(f"focal must be positive, got {focal}")
    return ops.nerf_rays_from_camera(camera.struct(), m, near, far, focal, near_ndc, pixel_begin, n, out, device)


def bungee_rays(camera: PinholeCamera, scene_scaling_factor: float, scene_origin: Sequence[float], ray_nearfar: str, pixel_begin: int = 0,
                n: Optional[int] = None, out: Optional[torch.Tensor] = None, radii_out: Optional[torch.Tensor] = None,
                device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The bungee scenes' rays [n, 8] (normalised directions, per-ray near / far of get_bungee_nearfar_radii: ray_nearfar "sphere" or
    "flat") and mip radii [n, 1] of a pixel range, in ONE launch.  out / radii_out: caller-owned contiguous device buffers written in
    place and returned."""
    kind = _mode(ray_nearfar, NEARFAR, "ray_nearfar")
    _check_bungee(camera.H, scene_scaling_factor, scene_origin)
    pixel_begin, n = _pixel_range(camera, pixel_begin, n)
    return ops.nerf_rays_bungee(camera.struct(), scene_scaling_factor, scene_origin, kind, pixel_begin, n, out, radii_out, device)


def camera_table(cameras: Sequence[PinholeCamera], device="cuda") -> torch.Tensor:
    """The cameras of a dataset as a device table [M, 16] (PinholeCamera.row per camera) for pixel_rays.  The cameras share W and H."""
    cameras = list(cameras)
    if not cameras:
        raise ValueError("camera_table: no cameras")
    if any((c.W, c.H) != (cameras[0].W, cameras[0].H) for c in cameras):
        raise ValueError("camera_table: the cameras of one table share W and H (pixel indices are row-major in one image size)")
    return torch.stack([c.row() for c in cameras]).to(device)


def pixel_rays(table: torch.Tensor, cam_idx: torch.Tensor, pix_idx: torch.Tensor, W: int, H: int, mode: str, near: float = 0.0,
               far: float = 1.0, focal: Optional[float] = None, near_ndc: float = 1.0, scene_scaling_factor: Optional[float] = None,
               scene_origin: Optional[Sequence[float]] = None, out: Optional[torch.Tensor] = None,
               radii_out: Optional[torch.Tensor] = None, check: bool = False):
    """The gather form of a training batch: ray i is pixel pix_idx[i] (row-major in W x H) of camera cam_idx[i] of `table`
    (camera_table).  mode "raw" / "normalized" / "ndc" -> rays [N, 8] (ndc needs focal: the table holds K, not the loader's focal);
    mode "sphere" / "flat" -> (rays [N, 8], radii [N, 1]) of the bungee scenes.  The same pixel of the same camera gives the bits of
    camera_rays / bungee_rays.  The indices are int32 or int64 device tensors of one dtype; their values are the caller's business
    (check=True validates them first - a host read, so not for a captured step)."""
    if not (torch.is_tensor(table) and table.dtype == torch.float32 and table.dim() == 2 and table.shape[1] == 16
            and table.shape[0] >= 1 and table.is_contiguous()):
        raise ValueError("table must be a contiguous fp32 tensor [M, 16] (camera_table)")
    if int(W) < 1 or int(H) < 1:
        raise ValueError(f"bad image size (W {W}, H {H})")
    m = _mode(mode, _PIXEL_MODES)
    for name, t in (("cam_idx", cam_idx), ("pix_idx", pix_idx)):
        if not (torch.is_tensor(t) and t.dtype in (torch.int32, torch.int64) and t.dim() == 1 and t.device == table.device):
            raise ValueError(f"{name} must be a 1-d int32 or int64 tensor on {table.device}")
    if cam_idx.dtype != pix_idx.dtype or cam_idx.shape != pix_idx.shape or cam_idx.numel() < 1:
        raise ValueError("cam_idx and pix_idx must be non-empty and share dtype and shape")
    bungee = mode in NEARFAR
    if bungee:
        if scene_scaling_factor is None or scene_origin is None:
            raise ValueError(f"mode {mode!r} needs scene_scaling_factor and scene_origin")
        _check_bungee(H, scene_scaling_factor, scene_origin)
    else:
        _check_nearfar(near, far)
        if m == _lib.NERF_NDC and not (focal is not None and float(focal) > 0):
            raise ValueError("mode 'ndc' needs a positive focal")
    _need_device(table, "table")
    if check:
        lo = min(int(cam_idx.min()), int(pix_idx.min()))
        if lo < 0 or int(cam_idx.max()) >= table.shape[0] or int(pix_idx.max()) >= int(W) * int(H):
            raise ValueError(f"index out of range: cameras in [0, {table.shape[0]}), pixels in [0, {int(W) * int(H)})")
    rays, radii = ops.nerf_rays_from_pixels(table, cam_idx.contiguous(), pix_idx.contiguous(), W, H, m, near, far,
                                            1.0 if focal is None else focal, near_ndc, scene_scaling_factor if bungee else 1.0,
                                            scene_origin if bungee else None, out, radii_out)
    return (rays, radii) if bungee else rays
