"""Rays from cameras on the device: the reference's ray_utils.py (get_ray_directions, get_rays, get_rays_batch) over csrc/raygen.hip.

    cam = Camera(W, H, intrinsics, c2w, image_index)               # the fields of the reference's ImageMetadata that rendering needs
    rays = camera_rays(cam, near, far, ray_altitude_range, center_pixels)                    # [H * W, 8], one launch
    camera_rays(cam, near, far, alt, True, pixel_begin=b, n=n, out=static_rays)              # a pixel batch into a caller's buffer
    table = camera_table(cameras)                                  # [M, 16] on the device, once per dataset
    rays = pixel_rays(table, cam_idx, pix_idx, W, H, near, far, alt, center_pixels)          # a training batch: 12 bytes per stored ray

get_ray_directions / get_rays / get_rays_batch keep the reference's signatures and run as the reference's two steps (directions in
memory, then the rays); the fused forms give the same bits.  Everything is fp32, also where the reference's render_image runs get_rays
inside autocast; there is no CPU path and no backward (camera poses are not trained here).
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch

from . import _lib, ops


class Camera:
    """A plain holder: W, H, intrinsics (fx, fy, cx, cy), c2w [3, 4] (fp32, on the host) and image_index - ImageMetadata without the
    image.  Two intrinsics (fx, fy) put the principal point in the middle of the image, as ImageMetadata does."""

    def __init__(self, W: int, H: int, intrinsics, c2w, image_index: int = 0):
        self.W, self.H = int(W), int(H)
        if self.W < 1 or self.H < 1:
            raise ValueError(f"Camera: bad image size (W {W}, H {H})")
        k = [float(v) for v in (intrinsics.tolist() if torch.is_tensor(intrinsics) else intrinsics)]
        if len(k) == 2:
            k = [k[0], k[1], self.W / 2.0, self.H / 2.0]
        if len(k) != 4:
            raise ValueError(f"Camera: intrinsics are (fx, fy, cx, cy) or (fx, fy), got {len(k)} values")
        self.intrinsics = torch.tensor(k, dtype=torch.float32)
        c2w = torch.as_tensor(c2w).detach().to("cpu", torch.float32)
        if tuple(c2w.shape) != (3, 4):
            raise ValueError(f"Camera: c2w must be [3, 4], got {tuple(c2w.shape)}")
        self.c2w = c2w.contiguous()
        self.image_index = int(image_index)

    def struct(self, center_pixels: bool) -> "_lib.Camera":
        """The camera as the library takes it by value (swn_camera, include/swn.h)."""
        c = _lib.Camera()
        c.c2w[:] = self.c2w.reshape(-1).tolist()
        c.fx, c.fy, c.cx, c.cy = self.intrinsics.tolist()
        c.W, c.H, c.center_pixels, c.image_index = self.W, self.H, int(bool(center_pixels)), self.image_index
        return c

    def row(self) -> torch.Tensor:
        """The camera's row of a camera table: c2w row-major, then fx, fy, cx, cy (16 floats, host)."""
        return torch.cat([self.c2w.reshape(-1), self.intrinsics])


def _check_bounds(near, far, ray_altitude_range):
    if not float(near) <= float(far):
        raise ValueError(f"near {near} > far {far}")
    if ray_altitude_range is not None:
        a = list(ray_altitude_range)
        if len(a) != 2 or not float(a[0]) < float(a[1]):
            raise ValueError(f"ray_altitude_range must be an ascending pair, got {a}")


def batches(n_pixels: int, batch: int):
    """The (pixel_begin, n) of an image walked in batches of `batch` pixels, the last one ragged - Runner.render_image's loop."""
    n_pixels, batch = int(n_pixels), int(batch)
    if n_pixels < 1 or batch < 1:
        raise ValueError(f"batches: {n_pixels} pixels in batches of {batch}")
    return [(b, min(batch, n_pixels - b)) for b in range(0, n_pixels, batch)]


def camera_rays(camera: Camera, near: float, far: float, ray_altitude_range: Optional[Sequence[float]] = None,
                center_pixels: bool = True, pixel_begin: int = 0, n: Optional[int] = None, out: Optional[torch.Tensor] = None,
                image_indices_out: Optional[torch.Tensor] = None, device=None) -> torch.Tensor:
    """The rays [n, 8] of the row-major pixels [pixel_begin, pixel_begin + n) of `camera` (n None: to the end of the image), in ONE
    launch: the directions are never written.  out: a caller's contiguous fp32 [n, 8] device buffer, written in place and returned (a
    captured graph's static input); image_indices_out: an int64 [n] buffer filled with camera.image_index."""
    P = camera.W * camera.H
    pixel_begin = int(pixel_begin)
    n = P - pixel_begin if n is None else int(n)
    if n < 1 or pixel_begin < 0 or pixel_begin + n > P:
        raise ValueError(f"pixel range [{pixel_begin}, {pixel_begin + n}) outside the image's {P} pixels (or empty)")
    _check_bounds(near, far, ray_altitude_range)
    return ops.rays_from_camera(camera.struct(center_pixels), near, far, ray_altitude_range, pixel_begin, n, out, image_indices_out,
                                device)


def get_ray_directions(W: int, H: int, fx: float, fy: float, cx: float, cy: float, center_pixels: bool, device) -> torch.Tensor:
    """ray_utils.get_ray_directions: the unit camera-space directions [H, W, 3] on `device`."""
    if int(W) < 1 or int(H) < 1:
        raise ValueError(f"bad image size (W {W}, H {H})")
    return ops.ray_directions(W, H, fx, fy, cx, cy, center_pixels, device)


def _dirs(directions: torch.Tensor) -> torch.Tensor:
    if not (torch.is_tensor(directions) and directions.dtype == torch.float32 and directions.dim() >= 1 and directions.shape[-1] == 3
            and directions.numel() > 0):
        raise ValueError("directions must be a non-empty fp32 tensor [..., 3] (get_ray_directions)")
    return directions.reshape(-1, 3).contiguous()


def _need_device(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise ValueError(f"{name} must be a device tensor: rays are generated on the GPU only (there is no CPU path)")


def get_rays(directions: torch.Tensor, c2w: torch.Tensor, near: float, far: float, ray_altitude_range: List[float]) -> torch.Tensor:
    """ray_utils.get_rays: directions [..., 3] and ONE pose c2w [3, 4] -> rays [..., 8]."""
    d = _dirs(directions)
    if tuple(c2w.shape) != (3, 4):
        raise ValueError(f"c2w must be [3, 4], got {tuple(c2w.shape)}")
    _check_bounds(near, far, ray_altitude_range)
    _need_device(d, "directions")
    pose = c2w.detach().to(d.device, torch.float32).reshape(1, 3, 4).contiguous()
    return ops.rays_from_directions(d, pose, near, far, ray_altitude_range).view(*directions.shape[:-1], 8)


def get_rays_batch(directions: torch.Tensor, c2w: torch.Tensor, near: float, far: float, ray_altitude_range: List[float]) -> torch.Tensor:
    """ray_utils.get_rays_batch: directions [P, 3] and poses c2w [K, 3, 4] -> rays [K, P, 8]."""
    d = _dirs(directions)
    if directions.dim() != 2 or c2w.dim() != 3 or tuple(c2w.shape[1:]) != (3, 4) or c2w.shape[0] < 1:
        raise ValueError(f"directions [P, 3] and c2w [K, 3, 4], got {tuple(directions.shape)} and {tuple(c2w.shape)}")
    _check_bounds(near, far, ray_altitude_range)
    _need_device(d, "directions")
    return ops.rays_from_directions(d, c2w.detach().to(d.device, torch.float32).contiguous(), near, far, ray_altitude_range)


def camera_table(cameras: Sequence[Camera], device="cuda") -> torch.Tensor:
    """The cameras of a dataset as a device table [M, 16] (Camera.row per camera) for pixel_rays.  The cameras share W and H."""
    cameras = list(cameras)
    if not cameras:
        raise ValueError("camera_table: no cameras")
    if any((c.W, c.H) != (cameras[0].W, cameras[0].H) for c in cameras):
        raise ValueError("camera_table: the cameras of one table share W and H (pixel indices are row-major in one image size)")
    return torch.stack([c.row() for c in cameras]).to(device)


def pixel_rays(table: torch.Tensor, cam_idx: torch.Tensor, pix_idx: torch.Tensor, W: int, H: int, near: float, far: float,
               ray_altitude_range: Optional[Sequence[float]] = None, center_pixels: bool = True, out: Optional[torch.Tensor] = None,
               check: bool = False) -> torch.Tensor:
    """The gather form of a training batch: ray i is pixel pix_idx[i] (row-major in W x H) of camera cam_idx[i] of `table`
    (camera_table) -> rays [N, 8].  The indices are int32 or int64 device tensors of one dtype.  Index values are the caller's business,
    as for the other gather kernels; check=True validates them first - a host read, so not for a captured step."""
    if not (torch.is_tensor(table) and table.dtype == torch.float32 and table.dim() == 2 and table.shape[1] == 16
            and table.shape[0] >= 1 and table.is_contiguous()):
        raise ValueError("table must be a contiguous fp32 tensor [M, 16] (camera_table)")
    if int(W) < 1 or int(H) < 1:
        raise ValueError(f"bad image size (W {W}, H {H})")
    for name, t in (("cam_idx", cam_idx), ("pix_idx", pix_idx)):
        if not (torch.is_tensor(t) and t.dtype in (torch.int32, torch.int64) and t.dim() == 1 and t.device == table.device):
            raise ValueError(f"{name} must be a 1-d int32 or int64 tensor on {table.device}")
    if cam_idx.dtype != pix_idx.dtype or cam_idx.shape != pix_idx.shape or cam_idx.numel() < 1:
        raise ValueError("cam_idx and pix_idx must be non-empty and share dtype and shape")
    _check_bounds(near, far, ray_altitude_range)
    _need_device(table, "table")
    if check:
        lo = min(int(cam_idx.min()), int(pix_idx.min()))
        if lo < 0 or int(cam_idx.max()) >= table.shape[0] or int(pix_idx.max()) >= int(W) * int(H):
            raise ValueError(f"index out of range: cameras in [0, {table.shape[0]}), pixels in [0, {int(W) * int(H)})")
    return ops.rays_from_pixels(table, cam_idx.contiguous(), pix_idx.contiguous(), W, H, center_pixels, near, far, ray_altitude_range, out)
