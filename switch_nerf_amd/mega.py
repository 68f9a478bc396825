"""The reference's Mega-NeRF model (models/mega_nerf.py: class MegaNeRF, built by models/model_utils.py:89-96 when --container_path
names a merged Mega-NeRF container) on the HIP path: K dense NeRFs (dense.DenseNeRF), one per spatial cell, behind a geometric
router.  A point goes to the cell with the nearest centroid (boundary_margin == 1) or, with boundary_margin > 1, to every cell within
margin x the nearest distance, the results blended by normalised inverse distance (mega_nerf.py:21-27, :49).

Structurally a second kind of gate - geometric, multi-membership, no parameters - in front of ragged dense sub-model calls:

    weights, counts = ops.cells_assign(x, centroids, dim_start, margin)      membership + blend weights        (csrc/cells.hip)
    begin, rows, slot = ops.cells_pack(weights, counts)                      packed row space, stable
    counts.tolist()                                                          the ONE device-to-host read: sizes the sub-model calls
    xin, noise = ops.cells_gather(x, rows, total, col0, sigma_noise)         every cell's rows, contiguous per cell
    sub_out[begin[i]:begin[i + 1]] = sub_modules[i](xin[...], ...)           DenseNeRF.__call__; empty cells are skipped
    out = ops.cells_blend(weights, slot, begin, sub_out, hard)               per-point gather in ascending cell order, no atomics

Sub-models with spherical-harmonics colour (DenseNeRF cfg["sh_deg"], the workflow --sh_deg exists for): a cell returns [n, 3 B + 1] raw
rows and the reference blends THOSE before rendering.py:344-347 applies sigmoid(eval_sh(...)).  ops.cells_blend_sh does the blend of the
wide rows and the evaluation in one launch (call_rgb; render_rays), or leaves the blended rows (the module mirror, __call__).

Inside a cell the rows ascend by point index - the order x[cluster_mask] has in the reference, so sigma_noise[cluster_mask] lines up.
Inference only: joint_training (the reference's distributed-training hack), device noise and graph capture are not built.
render_rays() below is what rendering.render_rays runs for a MegaNeRF foreground.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .dense import DenseNeRF

MAX_CELLS = 64      # swn_cells_*: the centroids live in LDS, a point's membership in one 64-bit mask


def dense_cfg_from_state_dict(sd, xyz_dim: int, allow_sh: bool = False) -> dict:
    """The DenseNeRF configuration of a reference NeRF state_dict (models/nerf.py:75-143 key layout), read off the tensor shapes.
    allow_sh: also recognise the spherical-harmonics layout (rgb.weight of 3 (d + 1)^2 rows, no direction block) and return
    pos_dir_dim = 0 and sh_deg = d for it; MegaNeRF.from_state_dicts / from_container pass it.  Without it that layout raises, as it
    did before MegaNeRF took such sub-models: a caller written for the direction layout gets no cfg with keys it does not know."""
    def shape(k):
        if k not in sd:
            raise NotImplementedError(f"sub-model state_dict has no `{k}`: only the appearance NeRF (appearance_dim > 0, no affine "
                                      "transform; a direction block or spherical-harmonics colour) is built on the dense path")
        return tuple(sd[k].shape)
    W, in_xyz = shape("xyz_encodings.0.0.weight")
    layers = 0
    while f"xyz_encodings.{layers}.0.weight" in sd:
        layers += 1
    skips = tuple(i for i in range(1, layers) if shape(f"xyz_encodings.{i}.0.weight")[1] == W + in_xyz)
    if in_xyz % xyz_dim or (in_xyz // xyz_dim - 1) % 2:
        raise ValueError(f"first layer of {in_xyz} inputs is no positional encoding of {xyz_dim} coordinates")
    count, app = shape("embedding_a.weight")
    if "affine.weight" in sd:
        raise NotImplementedError("affine_appearance sub-models are not built on the dense path")
    n_rgb, in2 = shape("rgb.weight")[0], shape("dir_a_encoding.0.weight")[1]
    common = dict(layer_dim=W, layers=layers, skip_layers=skips, pos_xyz_dim=(in_xyz // xyz_dim - 1) // 2)
    if n_rgb != 3 and not allow_sh:
        raise NotImplementedError(f"rgb.weight of {n_rgb} rows: a spherical-harmonics colour (sh_deg) sub-model - pass allow_sh=True to "
                                  "read its degree off the state dict (the cfg then carries sh_deg and pos_dir_dim = 0), as "
                                  "MegaNeRF.from_state_dicts / from_container do")
    if allow_sh and (n_rgb != 3 or in2 == W + app):
        # spherical-harmonics colour (models/nerf.py:82-83, :137-143): 3 B rows, B = (d + 1)^2, and no direction block in front of the
        # appearance embedding (a 3-row head without one is degree 0)
        B = n_rgb // 3
        d = int(round(B ** 0.5)) - 1
        if n_rgb % 3 or (d + 1) ** 2 != B or not 0 <= d <= 4:
            raise ValueError(f"rgb.weight of {n_rgb} rows is no 3 (d + 1)^2 with d in 0..4: not a spherical-harmonics colour head")
        if in2 != W + app:
            raise ValueError(f"rgb.weight of {n_rgb} rows (sh_deg {d}) but dir_a_encoding of {in2} inputs is not {W} + {app}: a "
                             "spherical-harmonics model has no direction block (pos_dir_dim == 0)")
        return dict(common, pos_dir_dim=0, appearance_dim=app, appearance_count=count, xyz_dim=xyz_dim, sh_deg=d)
    in_dir = in2 - W - app
    if in_dir < 3 or (in_dir - 3) % 6:
        raise ValueError(f"dir_a_encoding of {in2} inputs does not split into {W} + PE(dir) + {app}")
    return dict(common, pos_dir_dim=(in_dir - 3) // 6, appearance_dim=app, appearance_count=count, xyz_dim=xyz_dim)


class MegaNeRF:
    is_mega_nerf = True      # what rendering.render_rays dispatches on (no import of this module on the other models' path)

    def __init__(self, sub_modules: Sequence[DenseNeRF], centroids, boundary_margin: float, xyz_real: bool, cluster_2d: bool):
        """sub_modules: one DenseNeRF per cell (xyz_dim 4 with xyz_real, the background model; 3 otherwise), all of one compute dtype;
        they are put into evaluation mode.  centroids [K, 3].  Attributes as rendering.py:52-53 reads them."""
        assert boundary_margin >= 1                              # mega_nerf.py:11
        sub_modules = list(sub_modules)
        cen = centroids if torch.is_tensor(centroids) else torch.from_numpy(np.asarray(centroids))
        if cen.dim() != 2 or cen.shape[1] != 3 or cen.shape[0] != len(sub_modules):
            raise ValueError(f"centroids {tuple(cen.shape)} for {len(sub_modules)} sub-models: expected [{len(sub_modules)}, 3]")
        if not 1 <= len(sub_modules) <= MAX_CELLS:
            raise NotImplementedError(f"{len(sub_modules)} cells: the cell kernels hold up to {MAX_CELLS} centroids")
        xd = 4 if xyz_real else 3
        for m in sub_modules:
            if not isinstance(m, DenseNeRF) or m.xyz_dim != xd:
                raise TypeError(f"sub-models must be DenseNeRF with xyz_dim {xd} (xyz_real = {bool(xyz_real)})")
            m.eval()
        degs = [m.sh_deg for m in sub_modules]
        if any(d != degs[0] for d in degs):      # one row width for every cell: the blend adds the cells' raw rows (mega_nerf.py:43-49)
            if any(d is None for d in degs):
                raise ValueError(f"sub-models mix spherical-harmonics colour and plain colour heads (sh_deg per cell: {degs})")
            raise ValueError(f"sub-models of different spherical-harmonics degrees (sh_deg per cell: {degs})")
        self.sh_deg = degs[0]                                    # None, or the degree of every cell (rendering._check_sh's rule)
        self.n_out = 4 if self.sh_deg is None else 3 * (self.sh_deg + 1) ** 2 + 1
        self.sub_modules = sub_modules
        self.dev, self.dtype = sub_modules[0].dev, sub_modules[0].dtype
        self.centroids = cen.detach().to(torch.float32).to(self.dev).contiguous()
        self.boundary_margin = float(boundary_margin)
        self.xyz_real = bool(xyz_real)
        self.xyz_dim = xd
        self.cluster_dim_start = 1 if cluster_2d else 0
        self.joint_training = False
        self.training = False
        self.moe_no_batch = False

    # ------------------------------------------------------------------------------------------ construction
    @classmethod
    def from_state_dicts(cls, state_dicts, centroids, cfg: Optional[dict] = None, boundary_margin: float = 1.15, xyz_real: bool = False,
                         cluster_2d: bool = False, dtype=torch.float32, device="cuda") -> "MegaNeRF":
        """One DenseNeRF per reference-NeRF state_dict (DenseNeRF.load_state_dict takes that key layout); cfg None: derived from the
        tensor shapes of each state_dict."""
        xd = 4 if xyz_real else 3
        subs = []
        for sd in state_dicts:
            c = dict(cfg, xyz_dim=xd) if cfg is not None else dense_cfg_from_state_dict(sd, xd, allow_sh=True)
            m = DenseNeRF(c, dtype=dtype, device=device)
            m.load_state_dict(sd)
            subs.append(m)
        return cls(subs, centroids, boundary_margin, xyz_real, cluster_2d)

    @classmethod
    def from_container(cls, path, boundary_margin: float = 1.15, background: bool = False, dtype=torch.float32,
                       device="cuda") -> "MegaNeRF":
        """A merged Mega-NeRF container (a TorchScript archive with `centroids`, `cluster_2d` and sub_module_{i} / bg_sub_module_{i},
        model_utils.py:90-96): the foreground model, or with background=True the xyz_real background model."""
        container = torch.jit.load(path, map_location="cpu")
        centroids = container.centroids
        prefix = "bg_sub_module_{}" if background else "sub_module_{}"
        sds = [{k: v.detach() for k, v in getattr(container, prefix.format(i)).state_dict().items()} for i in range(len(centroids))]
        return cls.from_state_dicts(sds, centroids, None, boundary_margin, background, bool(container.cluster_2d), dtype, device)

    def state_dicts(self) -> List[dict]:
        return [m.state_dict() for m in self.sub_modules]

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("MegaNeRF is inference only: training through the cells (joint_training) is not built")
        return self

    def eval(self):
        return self

    # ------------------------------------------------------------------------------------------ forward
    def route(self, x):
        """(weights [P, K], counts [K], begin [K + 1], rows [<= P * K], slot [P, K]) of the points x: the device part of the router."""
        hard = self.boundary_margin == 1
        weights, counts = ops.cells_assign(x, self.centroids, self.cluster_dim_start, self.boundary_margin)
        begin, rows, slot = ops.cells_pack(weights, counts, x.shape[0] if hard else None)
        return weights, counts, begin, rows, slot

    def __call__(self, x, sigma_only: bool = False, sigma_noise=None):
        """MegaNeRF.forward (mega_nerf.py:19-61): x [P, 3 + 3 + 1] (position, direction, image index; with xyz_real [P, 3 + 4 + 3 + 1],
        the real position in front of the inverted-sphere point) -> [P, 4]; sigma_only: x [P, 3] ([P, 3 + 4]) -> [P, 1].
        Sub-models with sh_deg: no direction columns (x [P, 3 + 1], [P, 3 + 4 + 1]; rendering.py:316-330) -> [P, 3 B + 1], the blended
        raw rows (coefficients, sigma) that rendering.py:344-347 evaluates; call_rgb() does both in one launch."""
        st = self._sub_outputs(x, sigma_only, sigma_noise)
        if st is None:
            return torch.empty(0, 1 if sigma_only else self.n_out, dtype=torch.float32, device=self.dev)
        weights, slot, begin, sub_out, hard = st
        if self.sh_deg is None or sigma_only:
            return ops.cells_blend(weights, slot, begin, sub_out, hard)
        P = x.shape[0]      # the module's own output is the blended rows: the evaluation's direction plays no part in them
        return ops.cells_blend_sh(weights, slot, begin, sub_out, torch.zeros(P, 3, dtype=torch.float32, device=self.dev), 1, self.sh_deg,
                                  hard, want_coef=True)[1]

    def call_rgb(self, x, dirs, rows_per_group: int = 1, sigma_noise=None):
        """Sub-models with sh_deg: x as __call__ takes it, dirs [P / rows_per_group, 3] (point p is seen along dirs[p // rows_per_group];
        not normalised) -> [P, 4] = (sigmoid(eval_sh(blended coefficients, direction)), blended sigma): what rendering.py:344-349 makes
        of the module's output, through swn_cells_blend_sh, the blended rows never written."""
        if self.sh_deg is None:
            raise NotImplementedError("call_rgb is the spherical-harmonics form (sub-models with sh_deg); __call__ returns rgb otherwise")
        P, rpg = x.shape[0], int(rows_per_group)
        if rpg < 1 or P % rpg or tuple(dirs.shape) != (P // max(rpg, 1), 3):
            raise ValueError(f"call_rgb: dirs {tuple(dirs.shape)} for {P} points in groups of {rows_per_group}: expected [{P} / rows_per_group, 3]")
        st = self._sub_outputs(x, False, sigma_noise)
        if st is None:
            return torch.empty(0, 4, dtype=torch.float32, device=self.dev)
        weights, slot, begin, sub_out, hard = st
        return ops.cells_blend_sh(weights, slot, begin, sub_out, dirs.to(torch.float32).contiguous(), rpg, self.sh_deg, hard)

    def _sub_outputs(self, x, sigma_only, sigma_noise):
        """(weights, slot, begin, sub_out [total, C], hard): the routing and every cell's packed outputs; None for no points."""
        if self.boundary_margin < 1:
            raise AssertionError("boundary_margin must be >= 1")
        col0 = 3 if self.xyz_real else 0
        expected = col0 + self.xyz_dim + (0 if sigma_only else (4 if self.sh_deg is None else 1))
        if x.dim() != 2 or x.shape[1] != expected:
            raise Exception("Unexpected input shape: {} (expected: {}, xyz_dim: {})".format(tuple(x.shape), expected, self.xyz_dim))
        P, K = x.shape[0], len(self.sub_modules)
        Cn = 1 if sigma_only else self.n_out
        if P == 0:
            return None
        x = x.to(torch.float32).contiguous()
        noise = None if sigma_noise is None else sigma_noise.reshape(-1).to(torch.float32).contiguous()
        hard = self.boundary_margin == 1
        weights, counts, begin, rows, slot = self.route(x)
        n = counts.tolist()                                    # the one synchronisation: K ints size the ragged sub-model calls
        total = sum(n)
        if total == 0:      # only non-finite positions under a soft margin get here: their weights are NaN, so no cell counts as a member
            raise ValueError("MegaNeRF: no point belongs to a cell - the positions are not finite")
        xin, nin = ops.cells_gather(x, rows, total, col0, noise)
        sub_out = torch.empty(total, Cn, dtype=torch.float32, device=self.dev)
        b = 0
        for i, child in enumerate(self.sub_modules):
            if n[i] > 0:                                       # (empty cells are skipped, :38)
                sub_out[b:b + n[i]] = child(xin[b:b + n[i]], sigma_only, None if nin is None else nin[b:b + n[i]])
            b += n[i]
        if self.sh_deg == 0 and not sigma_only:
            # rgb_dim == 3: the reference's NeRF keeps its own nn.Sigmoid on the three outputs (models/nerf.py:140-141, :187-188), so
            # at degree 0 a cell's row holds sigmoid(lin), and rendering.py:344-347 puts eval_sh and a second sigmoid on the blend.
            # DenseNeRF's sh_deg call returns lin at every degree; the degenerate degree is squared with the reference here.
            sub_out[:, :3] = torch.sigmoid(sub_out[:, :3])
        return weights, slot, begin, sub_out, hard


# ---------------------------------------------------------------------------------------------- rendering
def _points(rays, z, image_indices, with_dir=True):
    """[N * S, 3 + 3 + 1]: position o + d z, direction and image index of every sample (rendering.py:357-360); with_dir False (sh_deg):
    [N * S, 3 + 1], no direction columns (:320-323)."""
    N, S = z.shape
    pts = rays[:, None, :3] + rays[:, None, 3:6] * z[:, :, None]
    d = rays[:, None, 3:6].expand(N, S, 3)
    img = image_indices.to(torch.float32).view(N, 1, 1).expand(N, S, 1)
    return torch.cat([pts, d, img] if with_dir else [pts, img], -1).view(N * S, 7 if with_dir else 4)


def _run(nerf, x, chunk, dirs=None):
    """The model over the points x [N * S, ..] (ray-major) per model chunk -> [N * S, 4].  dirs [N, 3] (sh_deg): through call_rgb, the
    chunks cut on ray boundaries so that one direction serves the S samples of a ray (the points are independent: where the reference
    cuts, rendering.py:320, does not reach the result); a chunk shorter than a ray takes per-point directions instead."""
    if dirs is None:
        return torch.cat([nerf(x[i:i + chunk]) for i in range(0, x.shape[0], chunk)], 0)
    N, S = dirs.shape[0], x.shape[0] // dirs.shape[0]
    if chunk >= S:
        per = chunk // S
        return torch.cat([nerf.call_rgb(x[r * S:(r + per) * S], dirs[r:r + per].contiguous(), S) for r in range(0, N, per)], 0)
    d = dirs[:, None, :].expand(N, S, 3).reshape(N * S, 3)
    return torch.cat([nerf.call_rgb(x[i:i + chunk], d[i:i + chunk].contiguous(), 1) for i in range(0, N * S, chunk)], 0)


def _sphere_exit(rays, center, radius):
    """The depth [N] at which each ray leaves the foreground bound, not clamped to near: d1 + d2 of rendering.py:527-540."""
    o, d = rays[:, :3], rays[:, 3:6]
    if radius is not None:
        c = torch.tensor(list(ops._host3(center)), dtype=torch.float32, device=rays.device)
        r = torch.tensor(list(ops._host3(radius)), dtype=torch.float32, device=rays.device)
        o, d = (o - c) / r, d / r
    d1 = -torch.sum(d * o, dim=-1) / torch.sum(d * d, dim=-1)
    pn = torch.norm(o + d1.unsqueeze(-1) * d, dim=-1)
    return d1 + torch.sqrt(1. - pn * pn) * (1. / d.norm(dim=-1))


def _bg_points(rays_b, img_b, pts4, real, with_dir=True):
    """[Nb * S, 3 + 4 + 3 + 1]: the real position (the cells' routing input, rendering.py:558-565) in front of the inverted-sphere point
    pts4 [Nb * S, 4], then direction and image index.  real: [Nb, S, 3], or [Nb, 3] where it is the same for every sample of a ray.
    with_dir False (sh_deg): [Nb * S, 3 + 4 + 1], no direction columns."""
    Nb, S = rays_b.shape[0], pts4.shape[0] // rays_b.shape[0]
    if real.dim() == 2:
        real = real[:, None, :].expand(Nb, S, 3)
    d = rays_b[:, None, 3:6].expand(Nb, S, 3)
    img = img_b.to(torch.float32).view(Nb, 1, 1).expand(Nb, S, 1)
    return torch.cat([real, pts4.view(Nb, S, 4), d, img] if with_dir else [real, pts4.view(Nb, S, 4), img], -1).view(Nb * S, 11 if with_dir else 8)


def _render_background(bg_nerf, cluster_2d, rays_b, img_b, center, radius, S, F, chunk, lin):
    """The background half of a scene (rendering.py:47-75 and _get_results with flip=True) on the rays that leave the bound: S // 2
    inverse-distance samples evaluated in descending order, F // 2 fine samples; the order quirks of background.BackgroundScene.forward
    (ascending bins x flipped weights, the un-flipped coarse depth_real in the merge) are the reference's and are kept.  The real
    position in front of each point is the sample's own (cluster_2d, :559-562) or the ray's exit from the bound (:564-565).
    -> rgb [Nb, 3], depth [Nb]."""
    o = ops
    Nb, Sb = rays_b.shape[0], S // 2
    sh = bg_nerf.sh_deg is not None
    dirs = rays_b[:, 3:6].contiguous() if sh else None       # (sh_deg: one direction per ray, rows_per_group = the pass's samples)
    ro, rd = rays_b[:, None, :3], rays_b[:, None, 3:6]
    edge = None if cluster_2d else rays_b[:, :3] + rays_b[:, 3:6] * _sphere_exit(rays_b, center, radius).unsqueeze(-1)
    # (no frequencies, fp32, stride 4: the sampling op's encoding is then the inverted-sphere point itself)
    z_b, dreal_b, p4 = o.bg_sample_pe(rays_b, center, radius, Sb, 0, torch.float32, 4)
    real = ro + rd * dreal_b.flip(-1).unsqueeze(-1) if cluster_2d else edge      # (the points are flipped, depth_real is not: :302-304)
    raw_b = _run(bg_nerf, _bg_points(rays_b, img_b, p4, real, not sh), chunk, dirs)
    rgb, depth, _, w_b, _ = o.composite_bounded_fwd(raw_b, z_b, None, True, dreal_b, want_weights=F > 0)
    if F > 0:
        Fb = F // 2
        z_f = o.sample_pdf(z_b.flip(-1).contiguous(), w_b, lin(Fb).expand(Nb, Fb).contiguous(), Fb)
        _, dreal_f, p4f = o.bg_sample_pe(rays_b, center, radius, Fb, 0, torch.float32, 4, z_in=z_f)
        real = ro + rd * dreal_f.unsqueeze(-1) if cluster_2d else edge
        raw_f = _run(bg_nerf, _bg_points(rays_b, img_b, p4f, real, not sh), chunk, dirs)
        zneg, order, raw_m = o.merge_samples((-z_f).contiguous(), (-z_b).contiguous(), raw_f, raw_b)      # descending sort (:421)
        dreal_m = torch.gather(torch.cat([dreal_f, dreal_b], 1), 1, order.long())                         # :432-433
        rgb, depth, _, _, _ = o.composite_bounded_fwd(raw_m, -zneg, None, True, dreal_m)
    return rgb, depth


def render_rays(nerf: MegaNeRF, bg_nerf, rays, image_indices, hparams, sphere_center=None, sphere_radius=None, get_depth: bool = True,
                get_depth_variance: bool = True, get_bg_fg_rgb: bool = False) -> Tuple[Dict[str, torch.Tensor], bool]:
    """rendering.render_rays for a MegaNeRF foreground (evaluation): the library's ray sampling, the [P, 3 + 3 + 1] points through the
    model per model_chunk_size, the library's compositing; fine_samples > 0: importance sampling from the coarse weights, the fine pass
    and the sort-merge of both sample sets, like SwitchNeRF.forward_hier.  A MegaNeRF returns a tensor, so there is no gate loss key
    (rendering.py:385-406).
    bg_nerf: the xyz_real MegaNeRF of the same container (model_utils.py:89-96).  Every ray is clipped at the foreground bound
    (swn_fg_bounds); the rays that leave it continue through _render_background and are blended in with the foreground's leftover
    transmittance (rendering.py:104-134), like background.BackgroundScene does for a dense background model."""
    from .rendering import _point_keys
    if not isinstance(nerf, MegaNeRF):
        raise NotImplementedError("a MegaNeRF background model behind a foreground model of another kind is not built")
    if bg_nerf is not None and not (isinstance(bg_nerf, MegaNeRF) and bg_nerf.xyz_real):
        raise NotImplementedError("the background model of a MegaNeRF scene is the container's xyz_real MegaNeRF "
                                  "(MegaNeRF.from_container(path, background=True)); a background model of another kind is not built")
    if getattr(hparams, "use_cascade", False):
        raise NotImplementedError("use_cascade is outside the hot path")
    if getattr(hparams, "affine_appearance", False):
        raise NotImplementedError("affine_appearance is not built for MegaNeRF")
    want = getattr(hparams, "sh_deg", None)                       # (rendering._check_sh's rule: hparams say what the model was built with)
    for who, m in (("the model", nerf), ("the background model", bg_nerf)):
        if m is not None and m.sh_deg != want:
            raise NotImplementedError(f"hparams.sh_deg = {want} but {who} was built with sh_deg = {m.sh_deg}: build the container's "
                                      "models and the hparams with the same sh_deg")
    if getattr(hparams, "device_noise_seed", None) is not None:
        raise NotImplementedError("device_noise_seed: MegaNeRF has no seeded device noise")
    if nerf.training or getattr(nerf, "graph_eval", False) or getattr(nerf, "graph_train", False):
        raise NotImplementedError("MegaNeRF renders in evaluation mode without graph capture")
    N, S, F = rays.shape[0], hparams.coarse_samples, int(getattr(hparams, "fine_samples", 0))
    rays = rays.contiguous()
    dev = rays.device
    if image_indices is None:
        image_indices = torch.zeros(N, dtype=torch.long, device=dev)
    chunk = int(hparams.model_chunk_size)
    lin = nerf.sub_modules[0]._linspace
    sh = want is not None
    dirs = rays[:, 3:6].contiguous() if sh else None              # (fg_bounds below changes the far bound only)
    Nb, bg_rgb, has_bg = 0, None, None
    if bg_nerf is not None:
        if bg_nerf.training or bg_nerf.dev != nerf.dev:
            raise NotImplementedError("MegaNeRF renders in evaluation mode, both models on one device")
        rays_full = rays
        rays, fg_far, last0, has_bg, n_out = ops.fg_bounds(rays_full, sphere_center, sphere_radius)      # (rays: far clipped at the bound)
        idx_bg = has_bg.nonzero().view(-1)                        # rays_with_bg, rendering.py:37 (a host read, like the reference)
        if int(n_out.item()) > 0:
            from .background import BackgroundScene
            raise Exception(BackgroundScene._UNBOUNDED)
        Nb = idx_bg.numel()
        if Nb > 0:                                                # background first, the reference's order
            bg_rgb, bg_depth = _render_background(bg_nerf, nerf.cluster_dim_start == 1, rays_full.index_select(0, idx_bg).contiguous(),
                                                  image_indices.index_select(0, idx_bg).contiguous(), sphere_center, sphere_radius,
                                                  S, F, chunk, lin)
    z = ops.sample_z(rays, lin(S), None, 0.0, S)                  # evaluation: no jitter, no sigma noise (rendering.py:366)
    raw = _run(nerf, _points(rays, z, image_indices, not sh), chunk, dirs)
    res: Dict[str, torch.Tensor] = {}
    if getattr(hparams, "return_sigma", False):
        res["sigma_coarse"] = raw[:, 3].view(N, S)
    raw_c, z_c = raw, z
    if F == 0:
        typ, z_last = "coarse", z[:, -1]                          # stratified depths ascend: the last one is the maximum (:216)
    else:
        _, _, _, w = ops.composite_fwd(raw, z, want_weights=True)      # (the last delta only reaches the last weight, which :240 drops)
        u = lin(F).expand(N, F).contiguous()                      # det = (perturb == 0): linspace (rendering.py:605-609)
        z_fine = ops.sample_pdf(z, w, u, F)
        raw_f = _run(nerf, _points(rays, z_fine, image_indices, not sh), chunk, dirs)
        z, order, raw = ops.merge_samples(z_fine, z_c, raw_f, raw_c)
        typ, z_last = "fine", z_fine.max(dim=-1)[0]               # the FINE depths' maximum (:249-250)
        if getattr(hparams, "return_sigma", False):
            res["sigma_fine"] = raw_f[:, 3].view(N, F)
    if bg_nerf is None:
        ld, ld_c = 1e10, 1e10
        rgb, depth, dvar, _ = ops.composite_fwd(raw, z)
    else:
        ld = torch.where(has_bg > 0, fg_far - z_last, last0).contiguous()                                  # :216-217 / :249-250
        ld_c = ld if F == 0 else torch.where(has_bg > 0, fg_far - z_c[:, -1], last0).contiguous()
        rgb, depth, dvar, _, lam = ops.composite_bounded_fwd(raw, z, ld, False, None, want_bg_lambda=True)
        if get_bg_fg_rgb:                                                                                  # :120-121, :142
            res[f"fg_rgb_{typ}"], res[f"fg_depth_{typ}"] = rgb, depth
        if Nb > 0:                                                                                         # :111-134
            lam_b = lam.index_select(0, idx_bg)
            rgb = rgb.index_add(0, idx_bg, bg_rgb * lam_b[:, None])
            depth = depth.index_add(0, idx_bg, bg_depth * lam_b)
        if get_bg_fg_rgb:
            res[f"bg_rgb_{typ}"], res[f"bg_depth_{typ}"] = rgb - res[f"fg_rgb_{typ}"], depth - res[f"fg_depth_{typ}"]
    _point_keys(res, hparams, "coarse", rays, raw_c, z_c, raw_c, ld_c)      # (foreground keys only, like the reference)
    if F > 0:
        _point_keys(res, hparams, "fine", rays, raw_f, z, raw, ld, z_pts=z_fine, order=order)
    res[f"rgb_{typ}"] = rgb
    if get_depth:
        res[f"depth_{typ}"] = depth
    if get_depth_variance:
        res[f"depth_variance_{typ}"] = dvar
    return res, Nb > 0
