"""Scene-decomposition point clouds: the export of Runner._run_validation_points (/root/reference/switch_nerf/runner.py:1870-2170,
driven by eval_points.py; README "Visualization").  One PLY file per image, sample type and expert shows which expert owns which
part of the scene.

    counts = render_image_points(nerf, bg_nerf, rays, image_index, hparams, out_dir, image_id)

renders the image's rays in pixel batches like rendering.render_image_rays with the point outputs on, packs every batch's PLY vertex
bodies on the device (swn_points_pack: quantisation, sample skip and the stable partition by expert) and spools only those bytes
to the files through a pinned host buffer.  Files (`i` = image_id, for each typ in hparams.render_test_points_typ):
    {i:03d}_{typ}_pts_rgba.ply, {i:03d}_{typ}_pts_rgba_top_0_exp_{e}.ply                  x y z f4, red green blue alpha u1
and with hparams.return_pts_class_seg (MoE models):
    {i:03d}_{typ}_top_0_alpha.ply, {i:03d}_{typ}_top_0_alpha_exp_{e}.ply                   expert palette colour + alpha
    {i:03d}_{typ}_top_0.ply, {i:03d}_{typ}_top_0_exp_{e}.ply                               expert palette colour (the last kept
                                                                                          sample of a ray: the rendered pixel)
A dense NeRF (no gates) writes the first file only.  Top-1 routing only.
"""
from __future__ import annotations

import os
import shutil
import tempfile
from argparse import Namespace
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import ops

# utils/functions.py:299 voc_palette() without its first (black) entry: the colour of expert e is VOC_PALETTE[e]
VOC_PALETTE = np.array([[128, 0, 0], [0, 128, 0], [128, 128, 0], [0, 0, 128], [128, 0, 128], [0, 128, 128], [128, 128, 128],
                        [64, 0, 0], [192, 0, 0], [64, 128, 0], [192, 128, 0], [64, 0, 128], [192, 0, 128], [64, 128, 128],
                        [192, 128, 128], [0, 64, 0], [128, 64, 0], [0, 192, 0], [128, 192, 0], [0, 64, 128]], dtype=np.uint8)

_PROPS = {ops.PLY_RGBA: ("red", "green", "blue", "alpha"), ops.PLY_SEG_ALPHA: ("red", "green", "blue", "alpha"),
          ops.PLY_SEG_RGB: ("red", "green", "blue")}


def ply_header(n: int, mode: int) -> bytes:
    """The header plyfile writes for a binary little-endian vertex element of x y z f4 + u1 colour channels (no comments)."""
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {int(n)}"]
    lines += [f"property float {c}" for c in "xyz"] + [f"property uchar {c}" for c in _PROPS[mode]]
    lines.append("end_header")
    return ("\n".join(lines) + "\n").encode("ascii")


class PlyWriter:
    """One PLY file whose vertex body arrives in pieces: append() spools the bytes to a temporary file next to the target, close()
    writes the header (the vertex count is known only then) followed by the body."""

    def __init__(self, path: str, mode: int):
        self.path, self.mode, self.n = path, mode, 0
        self.rec = ops.PLY_RECORD_BYTES[mode]
        fd, self._tmp = tempfile.mkstemp(prefix=".spool_", suffix=".body", dir=os.path.dirname(os.path.abspath(path)))
        self._body = os.fdopen(fd, "wb")

    def append(self, body) -> None:
        mv = memoryview(body).cast("B")
        assert len(mv) % self.rec == 0, (len(mv), self.rec)
        self._body.write(mv)
        self.n += len(mv) // self.rec

    def close(self) -> int:
        self._body.close()
        try:
            with open(self.path, "wb") as f:
                f.write(ply_header(self.n, self.mode))
                with open(self._tmp, "rb") as b:
                    shutil.copyfileobj(b, f, 1 << 22)
        finally:
            os.remove(self._tmp)
        return self.n

    def abort(self) -> None:
        self._body.close()
        if os.path.exists(self._tmp):
            os.remove(self._tmp)


def point_file_names(image_id: int, typ: str, n_experts: int, class_seg: bool, moe: bool = True) -> List[str]:
    """The reference's file names of one image and sample type (runner.py:2050-2052, :2091-2092, :2124-2125)."""
    names = [f"{image_id:03d}_{typ}_pts_rgba.ply"]
    if not moe:
        return names
    names += [f"{image_id:03d}_{typ}_pts_rgba_top_0_exp_{e}.ply" for e in range(n_experts)]
    if class_seg:
        names += [f"{image_id:03d}_{typ}_top_0_alpha.ply"] + [f"{image_id:03d}_{typ}_top_0_alpha_exp_{e}.ply" for e in range(n_experts)]
        names += [f"{image_id:03d}_{typ}_top_0.ply"] + [f"{image_id:03d}_{typ}_top_0_exp_{e}.ply" for e in range(n_experts)]
    return names


def _groups(image_id: int, typ: str, n_experts: int, class_seg: bool, moe: bool):
    """(mode, "all" file name, per-expert file names or None) of one image and sample type."""
    i = image_id
    out = [(ops.PLY_RGBA, f"{i:03d}_{typ}_pts_rgba.ply", [f"{i:03d}_{typ}_pts_rgba_top_0_exp_{e}.ply" for e in range(n_experts)]
            if moe else None)]
    if moe and class_seg:
        out.append((ops.PLY_SEG_ALPHA, f"{i:03d}_{typ}_top_0_alpha.ply",
                    [f"{i:03d}_{typ}_top_0_alpha_exp_{e}.ply" for e in range(n_experts)]))
        out.append((ops.PLY_SEG_RGB, f"{i:03d}_{typ}_top_0.ply", [f"{i:03d}_{typ}_top_0_exp_{e}.ply" for e in range(n_experts)]))
    return out


class _Pinned:
    """A growing pinned host buffer: device bodies come back through it (one copy each, no pageable staging)."""

    def __init__(self):
        self.buf = None

    def fetch(self, dev_bytes: torch.Tensor) -> np.ndarray:
        n = dev_bytes.numel()
        if self.buf is None or self.buf.numel() < n:
            self.buf = torch.empty(max(n, 1 << 20), dtype=torch.uint8, pin_memory=True)
        host = self.buf[:n]
        host.copy_(dev_bytes)                  # (synchronous: the host reads it right after)
        return host.numpy()


def render_image_points(nerf, bg_nerf, rays: torch.Tensor, image_index, hparams, out_dir: str, image_id: int, sphere_center=None,
                        sphere_radius=None) -> Dict[str, int]:
    """Render one image's rays ([R, 8]) in batches of hparams.image_pixel_batch_size with the point outputs on and write the
    reference's point files of that image into out_dir.  Honours hparams.render_test_points_typ (default ["coarse"]),
    render_test_points_sample_skip (1), return_pts_class_seg (False) and moe_expert_num.  -> {file name: point count}."""
    from .rendering import render_rays
    moe = _is_moe(nerf)
    h = Namespace(**vars(hparams))
    h.return_pts = h.return_pts_rgb = h.return_pts_alpha = True
    h.moe_return_gates = moe
    typs: Sequence[str] = list(getattr(hparams, "render_test_points_typ", ["coarse"]))
    skip = int(getattr(hparams, "render_test_points_sample_skip", 1))
    class_seg = bool(getattr(hparams, "return_pts_class_seg", False)) and moe
    E = int(getattr(hparams, "moe_expert_num", getattr(nerf, "E", 1))) if moe else 1
    assert E <= len(VOC_PALETTE), f"the palette has {len(VOC_PALETTE)} colours"
    if any(t not in ("coarse", "fine") for t in typs):
        raise ValueError(f"render_test_points_typ: {typs}")
    if "fine" in typs and int(getattr(hparams, "fine_samples", 0)) <= 0:
        raise ValueError("render_test_points_typ 'fine' needs fine_samples > 0")
    dev = rays.device
    palette = torch.from_numpy(VOC_PALETTE[:E].copy()).to(dev) if moe else None
    os.makedirs(out_dir, exist_ok=True)
    writers = {}
    plan = []
    for typ in typs:
        for mode, all_name, exp_names in _groups(image_id, typ, E, class_seg, moe):
            wa = writers[all_name] = PlyWriter(os.path.join(out_dir, all_name), mode)
            we = None
            if exp_names is not None:
                we = [PlyWriter(os.path.join(out_dir, n), mode) for n in exp_names]
                writers.update(zip(exp_names, we))
            plan.append((typ, mode, wa, we))
    R = rays.shape[0]
    rays = rays.reshape(-1, 8)
    idx = None
    if getattr(hparams, "appearance_dim", 1) > 0:
        idx = image_index if torch.is_tensor(image_index) and image_index.numel() == R else \
            torch.full((R,), int(image_index), dtype=torch.long, device=dev)
    pinned = _Pinned()
    step = int(hparams.image_pixel_batch_size)
    try:
        for i in range(0, R, step):
            r = rays[i:i + step].contiguous()
            ii = None if idx is None else idx[i:i + step].contiguous()
            res, _ = render_rays(nerf, bg_nerf, r, ii, h, sphere_center, sphere_radius, True, False, False)
            pixel = res["rgb_fine"] if "rgb_fine" in res else res["rgb_coarse"]
            for typ, mode, wa, we in plan:
                gates = res[f"moe_gates_{typ}"][..., 0, 0] if moe else None
                out_all, out_exp, counts = ops.points_pack(res[f"pts_{typ}"], res[f"pts_alpha_{typ}"], mode, skip, gates, E,
                                                           res[f"pts_rgb_{typ}"], pixel.float(), palette, want_experts=we is not None)
                wa.append(pinned.fetch(out_all))
                if we is not None:
                    cnt = counts.cpu().numpy().astype(np.int64)
                    body = pinned.fetch(out_exp[: int(cnt.sum()) * wa.rec])
                    off = 0
                    for e, w in enumerate(we):
                        w.append(body[off * w.rec:(off + cnt[e]) * w.rec])
                        off += int(cnt[e])
    except BaseException:
        for w in writers.values():
            w.abort()
        raise
    return {name: w.close() for name, w in writers.items()}


def _is_moe(nerf) -> bool:
    from .dense import DenseNeRF
    return not isinstance(nerf, DenseNeRF)
