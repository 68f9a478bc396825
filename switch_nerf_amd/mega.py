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

In the code the first four lines are _gather_cells (shared by inference and training) and the loop is _cells, the one iterator over
the non-empty cells (index, sub-model, slice of the packed rows) that every forward and backward_points walks.

Inside a cell the rows ascend by point index - the order x[cluster_mask] has in the reference, so sigma_noise[cluster_mask] lines up.
render_rays() below is what rendering.render_rays runs for a MegaNeRF foreground (evaluation).

Training (--train_mega_nerf, models/model_utils.py:118-123: MegaNeRF([NeRF ...], centroids, 1, xyz_dim == 4, cluster_2d, True)) is opt-in,
MegaNeRF(..., joint_training=True); without the flag the model is inference only, as before.  The same route -> pack -> gather, then

    c_i = sub_modules[i].forward_rays(rows of cell i as one-sample rays, ..., training=True, composite=False)     a SAVING forward per cell
    out = ops.cells_blend(weights, slot, begin, sub_out, hard)                                     forward_points -> ctx
    d_sub = ops.cells_blend_bwd(weights, rows, begin, d_out, total, hard)                         the blend's adjoint (swn_cells_blend_bwd)
    sub_modules[i].backward_net(c_i, d_sub[begin[i]:begin[i + 1]])                                backward_points: into each cell's gradient

The weights depend on positions only and the router has no parameters: nothing else flows back.  grad_step / apply_step / train_step put
the library's sampling, compositing, loss and Adam around it like SwitchNeRF.train_step does (coarse only, or coarse + fine with the
sort-merge).  A cell that no point reached in a step keeps a ZERO gradient, not a missing one (the reference's joint_training branch,
mega_nerf.py:51-59), so Adam still advances it.  What training costs here and does not hide: every cell runs its own launch sequence, and
a cell's rows are not whole rays, so the per-ray feature and the head backward run per point (rows_per_group 1).

Training cells with spherical-harmonics colour (--train_mega_nerf with --sh_deg: the cells that bake into an octree) is a second opt-in,
MegaNeRF(..., joint_training=True, sh_training=True).  The reference blends the cells' raw [3 B + 1] rows and evaluates the basis on the
blend (rendering.py:344-347), so the basis is no part of a cell:

    c_i = sub_modules[i].forward_coef(rows of cell i, ..)      the heads write (3 B coefficients, sigma) into the cell's slice (swn_heads_coef_fwd)
    out = ops.cells_blend_sh(weights, slot, begin, sub_out, dirs, rows_per_group, deg, hard)      the inference kernel: blend, eval_sh, sigmoid
    q, dirs_packed = ops.cells_blend_sh_bwd(.., out, d_out, dirs, ..)                              its adjoint, factored: d_lin[c B + b] = q_c Y_b
    sub_modules[i].backward_net(c_i, q[begin[i]:begin[i + 1]])                                     swn_heads_coef_bwd, then the cell's backward

The [total, 3 B + 1] gradient is never written.  The points carry no direction columns ([P, 3 + 1]); one direction serves the
rows_per_group samples of a ray.  At degree 0 a cell's row holds sigmoid(lin) and the blend's evaluation puts a second sigmoid on it,
as in inference.

Two forms of the cells' rows in training.  The COMPACT form (default, cell_capacity=None) is the one above: counts.tolist() sizes the
ragged calls, empty cells are skipped.  The PADDED form (forward_points / grad_step / train_step with cell_capacity = C, or (C_coarse,
C_fine) for the two passes of the hierarchical step) runs EVERY cell on exactly C rows whatever the batch:

    begin, rows, slot, overflow = ops.cells_pack_padded(weights, counts, C)     cell i owns rows [i C, (i + 1) C); -1 = a padding row
    xin, noise = ops.cells_gather_padded(x, rows, centroids, C, 0, sigma_noise) a padding row: the cell's centroid, direction (0, 0, 1)
    c_i = sub_modules[i].forward_rays(rows [i C, (i + 1) C) ...)                every cell, a cell without a member included
    out = ops.cells_blend(weights, slot, begin, sub_out, hard)                  the same kernel on the fixed begin[]
    d_sub = ops.cells_blend_bwd(weights, rows, begin, d_out, K C, hard)         exactly +0 on the padding rows

A padding row's gradient is +0, so it adds exact zeros to every sum of its cell's backward.  Nothing is read on the host in forward_points,
backward_points or grad_step: ctx["counts"] is the device tensor of the true members, ctx["overflow"] the device count of memberships
that did not fit, and apply_step(res=...) reads res["cell_overflow"] once behind the step's last launch - a batch with more than C
members in a cell raises RuntimeError there, before any parameter, moment or step count is touched.  What padding costs: K C rows of
network work against the batch's P (K times the largest cell's share at the tightest C).  What it buys: static shapes, so the step is
captured into a hipGraph (graph.GraphedMegaStep).  Not built for the padded form: spherical-harmonics cells (sh_training), data
parallelism, the xyz_real background half, a grouped launch over the cells.

Seeded device noise (MegaNeRF.set_device_noise(seed, step, ray_base), opt-in, both forms): the model holds ONE noise.DeviceNoise; the
cells' own stay off.  With it on grad_step draws what it is not handed as a pure function of (seed, step, stream, global element):

    perturb_rand = rng_fill(stream 0, uniform, e = (ray_base + n) S + s)        fine_u = rng_fill(stream 2, e = (ray_base + n) F + f)
    xin, noise = ops.cells_gather_rng / cells_gather_padded_rng(x, rows, .., seed, step, stream 1 | 3, R, ray_base, sigma_noise_std)
    ops.rng_advance(step)                                                       the step's last launch (inside a captured step)

The cells consume sigma noise per PACKED row - a point's value goes to every cell that holds it (sigma_noise[cluster_mask]) - so the
gather draws it in place: packed row r of point p = rows[r] gets the normal draw of element ray_base R + p, the bits swn_rng_fill writes
there, and the [N R] noise tensor is never written or read.  The eager step, a GraphedMegaStep replay and a resumed run
(noise_state_dict) then compute the same step bit for bit.  Evaluation draws nothing: mega.render_rays refuses device_noise_seed, and
a cell with its own seeded device noise switched on is refused.

Not built for training (each raises NotImplementedError): the xyz_real background half, fp16 cells (one loss scale over K models),
graph capture of the COMPACT form (counts.tolist() sizes the ragged calls), expert / data parallelism, gradient accumulation, the
finite guard, and rendering.render_rays on a model in training mode (the autograd bridge for a MegaNeRF is a later change).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import hier, ops, optim
from .dense import DenseNeRF
from .noise import DeviceNoise

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

    def __init__(self, sub_modules: Sequence[DenseNeRF], centroids, boundary_margin: float, xyz_real: bool, cluster_2d: bool,
                 joint_training: bool = False, sh_training: bool = False):
        """sub_modules: one DenseNeRF per cell (xyz_dim 4 with xyz_real, the background model; 3 otherwise), all of one compute dtype;
        they are put into evaluation mode.  centroids [K, 3].  Attributes as rendering.py:52-53 reads them.
        joint_training (mega_nerf.py:9, the reference's last constructor argument): the model trains through its cells (forward_points /
        backward_points / train_step); model and cells then start in training mode like a fresh nn.Module, and train() / eval() switch
        every cell.  The learning rate and the step count are the model's own (taken from the first cell), shared by every cell.
        sh_training: with joint_training, cells with spherical-harmonics colour train too (forward_points then takes the directions);
        without it such cells are refused, as before."""
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
            if not joint_training:
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
        self.joint_training = bool(joint_training)
        self.sh_training = bool(sh_training)
        self.training = False
        self.moe_no_batch = False
        self.noise = DeviceNoise()      # the seeded device noise's state (set_device_noise, joint training); the cells' own stay off
        if self.joint_training:
            self._check_trainable()
            self.lr = self.base_lr = float(sub_modules[0].base_lr)
            self.step_count = int(sub_modules[0].step_count)
            for m in sub_modules:
                m._grow_bufs = True                              # a cell's row count changes every step: one buffer per name, grown
            self.train(True)

    def _check_trainable(self):
        """What training through the cells does not build, named at construction."""
        if self.sh_deg is not None and not self.sh_training:
            raise NotImplementedError("joint_training with spherical-harmonics cells (sh_deg) is opt-in - pass sh_training=True (the "
                                      "cells then emit their coefficient rows, swn_heads_coef_fwd, and the blend swn_cells_blend_sh runs "
                                      "backward through swn_cells_blend_sh_bwd; forward_points takes the ray directions)")
        if self.xyz_real:
            raise NotImplementedError("joint_training with xyz_real (the background half) is not built: it needs BackgroundScene's "
                                      "bounded compositing backward around the cells")
        if self.dtype == torch.float16:
            raise NotImplementedError("joint_training with fp16 cells is not built: one loss scale shared over the cell models is "
                                      "missing; use bfloat16 or float32")
        for m in self.sub_modules:
            if m.dtype != self.dtype or m.dev != self.dev:
                raise ValueError("joint_training: every cell must have the same compute dtype and device")
            if m.device_noise:
                raise NotImplementedError("joint_training with seeded device noise (set_device_noise) switched on on a cell is refused: "
                                          "the step's draws belong to the whole model - leave the cells' off and call "
                                          "MegaNeRF.set_device_noise(seed)")
            if m.ep is not None:
                raise NotImplementedError("joint_training with expert parallelism is not built (a cell has no experts to shard)")

    # ------------------------------------------------------------------------------------------ construction
    @classmethod
    def from_state_dicts(cls, state_dicts, centroids, cfg: Optional[dict] = None, boundary_margin: float = 1.15, xyz_real: bool = False,
                         cluster_2d: bool = False, dtype=torch.float32, device="cuda", joint_training: bool = False,
                         sh_training: bool = False) -> "MegaNeRF":
        """One DenseNeRF per reference-NeRF state_dict (DenseNeRF.load_state_dict takes that key layout); cfg None: derived from the
        tensor shapes of each state_dict.  joint_training, sh_training: the constructor's."""
        xd = 4 if xyz_real else 3
        subs = []
        for sd in state_dicts:
            c = dict(cfg, xyz_dim=xd) if cfg is not None else dense_cfg_from_state_dict(sd, xd, allow_sh=True)
            m = DenseNeRF(c, dtype=dtype, device=device)
            m.load_state_dict(sd)
            subs.append(m)
        return cls(subs, centroids, boundary_margin, xyz_real, cluster_2d, joint_training, sh_training)

    @classmethod
    def from_container(cls, path, boundary_margin: float = 1.15, background: bool = False, dtype=torch.float32,
                       device="cuda") -> "MegaNeRF":
        """A merged Mega-NeRF container (a TorchScript archive with `centroids`, `cluster_2d` and sub_module_{i} / bg_sub_module_{i},
        model_utils.py:90-96): the foreground model, or with background=True the xyz_real background model.  Inference only (a
        container is what merging trained cells produces; to train, build from_state_dicts(..., joint_training=True))."""
        container = torch.jit.load(path, map_location="cpu")
        centroids = container.centroids
        prefix = "bg_sub_module_{}" if background else "sub_module_{}"
        sds = [{k: v.detach() for k, v in getattr(container, prefix.format(i)).state_dict().items()} for i in range(len(centroids))]
        return cls.from_state_dicts(sds, centroids, None, boundary_margin, background, bool(container.cluster_2d), dtype, device)

    def state_dicts(self) -> List[dict]:
        return [m.state_dict() for m in self.sub_modules]

    def train(self, mode=True):
        if not self.joint_training:
            if mode:
                raise NotImplementedError("MegaNeRF is inference only: training through the cells (joint_training) is not built "
                                          "for this model - construct it with joint_training=True")
            return self
        self.training = bool(mode)
        for m in self.sub_modules:
            m.train(mode)
        return self

    def eval(self):
        return self.train(False)

    # ------------------------------------------------------------------------------------------ parameters (all cells)
    def named_parameters(self):
        """(key, tensor) over every cell, keys `sub_modules.{i}.` + the reference NeRF's (the ModuleList keys of mega_nerf.py:14)."""
        for i, m in enumerate(self.sub_modules):
            for k, v in m.named_parameters():
                yield f"sub_modules.{i}.{k}", v

    def parameters(self):
        return (v for _, v in self.named_parameters())

    def grad_dict(self):
        """Every cell's gradient under the keys of named_parameters()."""
        return {f"sub_modules.{i}.{k}": v for i, m in enumerate(self.sub_modules) for k, v in m.grad_dict().items()}

    def set_iteration(self, iteration: int, lr_decay_factor: float = 0.1, train_iterations: int = 500000):
        """The learning-rate schedule hook of SwitchNeRF.set_iteration, forwarded to every cell: one rate for the whole model."""
        self._need_joint("set_iteration")
        for m in self.sub_modules:
            m.base_lr = self.base_lr
            self.lr = m.set_iteration(iteration, lr_decay_factor, train_iterations)
        return self.lr

    def set_expert_parallel(self, ep):
        raise NotImplementedError("MegaNeRF: expert parallelism is not built (the cells are dense models; nothing is sharded)")

    # ------------------------------------------------------------------------------------------ seeded device noise
    def set_device_noise(self, seed, step: int = 0, ray_base: int = 0):
        """Seeded device-side noise for joint training (SwitchNeRF.set_device_noise's semantics; csrc/philox.hpp): seed = None turns it
        off (the default - no launch differs from a model that never had it on).  On, grad_step / train_step draw what they are not
        handed - the jitter (stream 0), the fine pass's u (stream 2) and, with sigma_noise_std > 0, the sigma noise of both passes
        (streams 1 and 3, drawn at the cells' packed rows by swn_cells_gather_rng / _padded_rng) - from Philox4x32-10 keyed by (seed,
        step, stream, global element): the same step eagerly and in a GraphedMegaStep replay, in the compact and the padded form, before
        and after a resume (noise_state_dict).  The step lives on the device; grad_step's last launch advances it.  ray_base: the global
        index of the batch's first ray.  An inference-only model draws nothing and refuses a seed; so does a host-resident model
        (device "cpu": parameters only, no kernel can run on it - the counter is device memory the gather kernels read)."""
        if seed is not None and not self.joint_training:
            raise NotImplementedError("MegaNeRF.set_device_noise: seeded device noise belongs to joint training (evaluation draws "
                                      "nothing) - construct the model with joint_training=True")
        if seed is not None and self.dev.type != "cuda":
            raise NotImplementedError("MegaNeRF.set_device_noise: seeded device noise needs the model on a GPU - this one is "
                                      f"host-resident (device {self.dev}) and trains nothing; its step counter is device memory")
        self.noise.set(seed, step, ray_base, self.dev)

    @property
    def device_noise(self) -> bool:
        return self.noise.on

    def set_ray_base(self, ray_base: int):
        """The global index of the next batch's first ray (SwitchNeRF.set_ray_base)."""
        self._need_joint("set_ray_base")
        self.noise.set_base(ray_base)

    def noise_state_dict(self) -> dict:
        """{"seed", "step", "ray_base"} - what a resume needs besides the cells' parameters and Adam state (seed None: off).  Reads the
        step back from the device."""
        self._need_joint("noise_state_dict")
        return self.noise.state_dict()

    def load_noise_state_dict(self, sd: dict):
        self._need_joint("load_noise_state_dict")
        self.set_device_noise(sd.get("seed"), int(sd.get("step", 0)), int(sd.get("ray_base", 0)))

    def _need_joint(self, what):
        if not self.joint_training:
            raise NotImplementedError(f"MegaNeRF.{what}: this model is inference only - construct it with joint_training=True")

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
        if x.shape[0] == 0:
            return None
        r, xin, nin = self._gather_cells(x, sigma_noise, col0)
        sub_out = torch.empty(r["total"], 1 if sigma_only else self.n_out, dtype=torch.float32, device=self.dev)
        for _i, child, sl in self._cells(r["counts"]):
            sub_out[sl] = child(xin[sl], sigma_only, None if nin is None else nin[sl])
        if self.sh_deg == 0 and not sigma_only:
            # rgb_dim == 3: the reference's NeRF keeps its own nn.Sigmoid on the three outputs (models/nerf.py:140-141, :187-188), so
            # at degree 0 a cell's row holds sigmoid(lin), and rendering.py:344-347 puts eval_sh and a second sigmoid on the blend.
            # DenseNeRF's sh_deg call returns lin at every degree; the degenerate degree is squared with the reference here.
            sub_out[:, :3] = torch.sigmoid(sub_out[:, :3])
        return r["weights"], r["slot"], r["begin"], sub_out, r["hard"]

    def _gather_cells(self, x, sigma_noise, col0=0, sigma_rng=None):
        """The prologue of every forward over the points x: route, the ONE device-to-host read, cells_gather from column col0 on ->
        (routing, xin [total, ..], noise [total] or None); routing = {weights, rows, begin, slot, counts (a host list), total, hard, P}.
        sigma_rng = (stream id, rows per ray, std): the noise is drawn at the packed rows from the model's seeded generator instead."""
        x = x.to(torch.float32).contiguous()
        noise = None if sigma_noise is None else sigma_noise.reshape(-1).to(torch.float32).contiguous()
        weights, counts, begin, rows, slot = self.route(x)
        n = counts.tolist()                                    # the one synchronisation: K ints size the ragged sub-model calls
        total = sum(n)
        if total == 0:      # only non-finite positions under a soft margin get here: their weights are NaN, so no cell counts as a member
            raise ValueError("MegaNeRF: no point belongs to a cell - the positions are not finite")
        if sigma_rng is None:
            xin, nin = ops.cells_gather(x, rows, total, col0, noise)
        else:
            xin, nin = ops.cells_gather_rng(x, rows, total, col0, *self._sigma_rng(sigma_rng))
        return dict(weights=weights, rows=rows, begin=begin, slot=slot, counts=n, total=total, hard=self.boundary_margin == 1,
                    P=x.shape[0]), xin, nin

    def _capacity(self, cell_capacity):
        """cell_capacity as forward_points / grad_step / train_step take it -> None (the compact form) or (C_coarse, C_fine)."""
        if cell_capacity is None:
            return None
        pair = tuple(cell_capacity) if isinstance(cell_capacity, (tuple, list)) else (cell_capacity, cell_capacity)
        if len(pair) != 2 or any(isinstance(c, bool) or not isinstance(c, int) or c < 1 for c in pair):
            raise ValueError(f"cell_capacity {cell_capacity!r}: expected None, an int >= 1 (rows per cell) or a pair (coarse, fine) of them")
        if self.sh_deg is not None:
            raise NotImplementedError("cell_capacity (the padded form of the cells' rows) is not built for spherical-harmonics cells "
                                      "(sh_training): train them in the compact form")
        return pair

    def _cells(self, counts, capacity=None):
        """(cell index, sub-model, its slice of the packed rows) of every non-empty cell (empty cells are skipped, mega_nerf.py:38; in
        training their gradient stays zero, :51-59).  capacity (the padded form): every cell, on its fixed range of that many rows."""
        if capacity is not None:
            for i, child in enumerate(self.sub_modules):
                yield i, child, slice(i * capacity, (i + 1) * capacity)
            return
        b = 0
        for i, (child, n) in enumerate(zip(self.sub_modules, counts)):
            if n > 0:
                yield i, child, slice(b, b + n)
            b += n

    # ------------------------------------------------------------------------------------------ training through the cells
    def _sigma_rng(self, sigma_rng):
        """(stream id, rows per ray, std) -> the draw arguments of ops.cells_gather_rng / cells_gather_padded_rng."""
        stream_id, R, std = sigma_rng
        return self.noise.seed, self.noise.step, stream_id, R, self.noise.base, std

    def _gather_cells_padded(self, x, sigma_noise, C, sigma_rng=None):
        """_gather_cells in the padded form (module doc): no host read, every cell on C rows.  routing["counts"] is the device tensor of
        the true members, routing["overflow"] [1] the device count of memberships that did not fit, routing["C"] the capacity."""
        x = x.to(torch.float32).contiguous()
        noise = None if sigma_noise is None else sigma_noise.reshape(-1).to(torch.float32).contiguous()
        weights, counts = ops.cells_assign(x, self.centroids, self.cluster_dim_start, self.boundary_margin)
        begin, rows, slot, overflow = ops.cells_pack_padded(weights, counts, C)
        if sigma_rng is None:
            xin, nin = ops.cells_gather_padded(x, rows, self.centroids, C, 0, noise)
        else:
            xin, nin = ops.cells_gather_padded_rng(x, rows, self.centroids, C, 0, *self._sigma_rng(sigma_rng))
        return dict(weights=weights, rows=rows, begin=begin, slot=slot, counts=counts, total=len(self.sub_modules) * C,
                    hard=self.boundary_margin == 1, P=x.shape[0], C=C, overflow=overflow), xin, nin

    def forward_points(self, x, sigma_noise=None, tag: str = "c", dirs=None, rows_per_group: int = 1, cell_capacity=None, sigma_rng=None):
        """The training form of __call__: x [P, 3 + 3 + 1] -> ctx with ctx["out"] [P, 4] and what backward_points needs.  Every non-empty
        cell runs a SAVING forward on its packed rows (DenseNeRF.forward_rays on one-sample rays, as DenseNeRF.__call__ does), so a cell
        holds ONE live context per tag: a second forward_points under the same tag overwrites the first one's saved activations (the
        hierarchical step runs its fine pass under tag "f").
        Cells with sh_deg (sh_training): x [P, 3 + 1] (no direction columns) and dirs [P / rows_per_group, 3], point p seen along
        dirs[p // rows_per_group] (not normalised), the training form of call_rgb: ctx["out"] = (sigmoid(eval_sh(blended coefficients,
        direction)), blended sigma).
        cell_capacity = C, or (C_coarse, C_fine) of which tag "f" takes the second: the padded form (module doc) - every cell, one
        without a member included, runs on exactly C rows; nothing is read on the host, so the pass can be captured into a hipGraph.
        ctx["counts"] is then the device int32 [K] of true members and ctx["overflow"] the device count of memberships dropped because
        a cell had more than C (apply_step(res=...) refuses such a step).  Not built for cells with sh_deg.
        sigma_rng = (stream id, R, std), with the model's device noise on (set_device_noise) and instead of sigma_noise: the sigma noise
        is drawn at the cells' packed rows - point p = n * R + s of the batch is element ray_base * R + p of stream ops.RNG_SIGMA or
        RNG_SIGMA_FINE, times std - so no [P] noise tensor exists (swn_cells_gather_rng / _padded_rng)."""
        self._need_joint("forward_points")
        cap = self._capacity(cell_capacity)
        if sigma_rng is not None:
            if sigma_noise is not None:
                raise ValueError("forward_points: sigma_noise (a tensor) and sigma_rng (a draw request) exclude each other")
            if not self.noise.on:
                raise ValueError("forward_points: sigma_rng draws from the model's seeded device noise, which is off (set_device_noise)")
        if cap is None and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise NotImplementedError("MegaNeRF: graph capture is not built - counts.tolist() sizes the ragged per-cell calls on the host")
        sh = self.sh_deg is not None
        width = 4 if sh else 7
        if x.dim() != 2 or x.shape[1] != width:
            raise Exception("Unexpected input shape: {} (expected: {}, xyz_dim: {})".format(tuple(x.shape), width, self.xyz_dim))
        P = x.shape[0]
        if P == 0:
            raise ValueError("MegaNeRF.forward_points: no points")
        if sh:
            rpg = int(rows_per_group)
            if dirs is None or rpg < 1 or P % rpg or tuple(dirs.shape) != (P // rpg, 3):
                raise ValueError(f"forward_points: cells with sh_deg need dirs [{P} / rows_per_group, 3] (got "
                                 f"{None if dirs is None else tuple(dirs.shape)}, rows_per_group {rows_per_group})")
            dirs = dirs.to(torch.float32).contiguous()
        elif dirs is not None:
            raise ValueError("forward_points: dirs belong to cells with sh_deg; these points carry their direction columns")
        C = None if cap is None else cap[1 if tag == "f" else 0]
        r, xin, nin = (self._gather_cells(x, sigma_noise, 0, sigma_rng) if C is None else
                       self._gather_cells_padded(x, sigma_noise, C, sigma_rng))
        total, cells = r["total"], [None] * len(self.sub_modules)
        if sh:
            # each cell's heads write its slice of the packed rows (degree 0: the reference NeRF's own sigmoid on its three outputs, as
            # _sub_outputs); the inference blend kernel evaluates the basis on the blend
            sub_out = torch.empty(total, self.n_out, dtype=torch.float32, device=self.dev)
            for i, child, sl in self._cells(r["counts"]):
                cells[i] = child.forward_coef(xin[sl], None if nin is None else nin[sl], sub_out[sl], self.sh_deg == 0, tag)
            out = ops.cells_blend_sh(r["weights"], r["slot"], r["begin"], sub_out, dirs, rpg, self.sh_deg, r["hard"])
            return dict(r, out=out, cells=cells, tag=tag, sub_out=sub_out, dirs=dirs, rows_per_group=rpg)
        rays = torch.cat([xin[:, :6], torch.zeros(total, 2, device=self.dev)], 1)      # o = xyz, near = far = 0 -> the sample IS the point
        img = xin[:, 6].long()
        sub_out = torch.empty(total, 4, dtype=torch.float32, device=self.dev)
        for i, child, sl in self._cells(r["counts"], C):
            c = cells[i] = child.forward_rays(rays[sl].contiguous(), img[sl].contiguous(), 1, sl.stop - sl.start, 0.0, None,
                                              None if nin is None else nin[sl], training=True, tag=tag, composite=False)
            sub_out[sl] = c["raw"]
        out = ops.cells_blend(r["weights"], r["slot"], r["begin"], sub_out, r["hard"])
        return dict(r, out=out, cells=cells, tag=tag)

    def backward_points(self, ctx, d_out):
        """Backward of forward_points given dL/d out [P, 4]: the blend's adjoint (ops.cells_blend_bwd), then every non-empty cell's
        backward_net on its rows - accumulated into that cell's gradient (nothing is zeroed here)."""
        self._need_joint("backward_points")
        if tuple(d_out.shape) != (ctx["P"], 4):
            raise ValueError(f"backward_points: d_out {tuple(d_out.shape)} for an output of [{ctx['P']}, 4]")
        d_out = d_out.to(torch.float32).contiguous()
        if self.sh_deg is not None:      # the factored adjoint: q [total, 4] and one direction per packed row cross to the cells
            d_sub, dp = ops.cells_blend_sh_bwd(ctx["weights"], ctx["rows"], ctx["begin"], ctx["out"], d_out, ctx["dirs"], ctx["rows_per_group"],
                                               self.sh_deg, ctx["total"], ctx["hard"], ctx["sub_out"] if self.sh_deg == 0 else None)
        else:
            d_sub, dp = ops.cells_blend_bwd(ctx["weights"], ctx["rows"], ctx["begin"], d_out, ctx["total"], ctx["hard"]), None
        for i, child, sl in self._cells(ctx["counts"], ctx.get("C")):      # (the form follows the context's)
            c = ctx["cells"][i]
            if dp is not None:
                c["coef_dirs"] = dp[sl]
            child.backward_net(c, d_sub[sl], None)

    def grad_step(self, rgbs, rays, image_indices, n_samples, perturb=1.0, perturb_rand=None, sigma_noise=None, fine_samples=0, fine_u=None,
                  sigma_noise_fine=None, cell_capacity=None, sigma_noise_std=0.0):
        """Forward + loss + backward of one training step (SwitchNeRF.grad_step's contract): zeroes every cell's gradient, fills it, and
        returns the metrics.  The whole batch goes through the cells in one call: a MegaNeRF's output for a point does not depend on the
        other points of its chunk, so there is no model_chunk_size loop.  fine_samples > 0: the sequence of SwitchNeRF.forward_hier
        (coarse pass with weights, sample_pdf from the detached weights, fine pass under tag "f", sort-merge, compositing of the union).
        cell_capacity: the padded form (forward_points) - no host read in the whole step; the result then holds "cell_overflow", the
        device int32 [2] of memberships dropped in the coarse and the fine pass (0 for a pass that did not run), for apply_step(res=...).
        Device noise on (set_device_noise): what is not supplied is drawn from the seeded generator - the jitter (perturb != 0; stream 0,
        element (ray_base + n) * S + s), the fine pass's u (stream 2, (ray_base + n) * F + f) and, with sigma_noise_std > 0, the sigma
        noise of both passes at the cells' packed rows (forward_points sigma_rng) - and the step's LAST launch advances the counter,
        whatever optimizer_step the caller applies it with.  A supplied tensor wins, each for its own draw."""
        self._need_joint("grad_step")
        cap = self._capacity(cell_capacity)
        dn = self.noise if self.noise.on else None
        std = float(sigma_noise_std)
        o = ops
        N, S, F = rays.shape[0], int(n_samples), int(fine_samples)
        rays = rays.to(torch.float32).contiguous()
        for m in self.sub_modules:
            m.grad.zero_()
        lin = self.sub_modules[0]._linspace
        if perturb != 0 and perturb_rand is None:
            perturb_rand = torch.rand(N, S, device=self.dev) if dn is None else dn.draw(o.RNG_JITTER, N * S, dn.base * S,
                                                                                       o.RNG_UNIFORM).view(N, S)
        z = o.sample_z(rays, lin(S), perturb_rand if perturb != 0 else None, perturb, S)
        sh = self.sh_deg is not None          # (sh_deg: no direction columns, one direction per ray: rendering.py:316-330)
        dirs = rays[:, 3:6].contiguous() if sh else None
        draw = lambda given, stream_id, R: (stream_id, R, std) if dn is not None and given is None and std > 0 else None
        c = self.forward_points(_points(rays, z, image_indices, not sh), sigma_noise, "c", dirs, S, cap, draw(sigma_noise, o.RNG_SIGMA, S))
        raw = c["out"]
        if F == 0:
            cf = None
            out = dict(raw=raw, z=z)
            out["rgb"], out["depth"], out["depth_variance"], _ = o.composite_fwd(raw, z)
        else:
            _, _, _, w = o.composite_fwd(raw, z, want_weights=True)
            if fine_u is None and perturb != 0 and dn is not None:
                fine_u = dn.draw(o.RNG_FINE_U, N * F, dn.base * F, o.RNG_UNIFORM).view(N, F)
            if fine_u is None:
                fine_u = hier.default_fine_u(lin, N, F, perturb, self.dev)
            z_fine = o.sample_pdf(z, w, fine_u, F)
            cf = self.forward_points(_points(rays, z_fine, image_indices, not sh), sigma_noise_fine, "f", dirs, F, cap,
                                     draw(sigma_noise_fine, o.RNG_SIGMA_FINE, F))
            zm, order, raw_m = o.merge_samples(z_fine, z, cf["out"], raw)
            out = dict(raw=raw_m, z=zm, order=order, z_fine=z_fine)
            out["rgb"], out["depth"], out["depth_variance"], _ = o.composite_fwd(raw_m, zm)
        # a MegaNeRF returns a tensor: no gate loss (rendering.py:385-406) - a zero operand with weight 0
        zero = torch.zeros(1, dtype=torch.float32, device=self.dev)
        out4, d_rgb, _, _ = o.step_loss(out["rgb"], rgbs.to(torch.float32).contiguous(), zero, None, 0.0, None)
        if F == 0:
            self.backward_points(c, o.composite_bwd(raw, z, d_rgb))
        else:
            d_raw_f, d_raw_c = hier.merged_bwd(out, d_rgb)
            self.backward_points(cf, d_raw_f)
            self.backward_points(c, d_raw_c)
        res = dict(loss=out4[2], photo_loss=out4[0], gate_loss=out4[1], psnr=out4[3], depth_variance=out["depth_variance"].mean(), ctx=c,
                   rgb=out["rgb"], depth=out["depth"])
        if cf is not None:
            res["ctx_fine"] = cf
        if cap is not None:
            res["cell_overflow"] = torch.cat([c["overflow"], cf["overflow"] if cf is not None else torch.zeros_like(c["overflow"])])
        self.noise.advance()               # device noise: the next step draws at step + 1 (the last launch, inside a captured step)
        return res

    def set_accumulation(self, steps: int):
        """Gradient accumulation (SwitchNeRF.set_accumulation) is not built for joint training through the cells: only 1 is taken."""
        if int(steps) < 1:
            raise ValueError(f"set_accumulation: accumulation steps must be >= 1, got {steps}")
        if int(steps) > 1:
            raise NotImplementedError("MegaNeRF: gradient accumulation (set_accumulation) is not built for joint training: a window "
                                      "would span every cell model's buffer under the container's one step count")

    _GUARD_JOINT = ("MegaNeRF: the finite guard (check_finite) is not built for joint training: the cells step under the container's "
                    "one host step count")

    def set_check_finite(self, on: bool = True):
        """The finite guard (SwitchNeRF.set_check_finite) is not built for joint training through the cells: only off is taken."""
        if on:
            raise NotImplementedError(self._GUARD_JOINT)

    def apply_step(self, grad_allreduce=None, optimizer_step=True, res=None, refresh=None):
        """One Adam step on every cell with the model's one step count and learning rate.  A cell no point reached has a zero gradient,
        not a missing one: its step count advances, its moments decay and it moves by momentum, like the reference's joint_training cells
        under one torch.optim.Adam.
        res: the result of the grad_step being applied.  A padded step's (cell_capacity) carries "cell_overflow", read here ONCE - the
        step's only device-to-host read, behind its last launch: a batch that had more members in a cell than the capacity was computed
        without the surplus rows and raises RuntimeError before any parameter, moment or step count is touched.
        refresh: a replacement for every cell's refresh_compute_copies (the replay of their captured graph), run once."""
        self._need_joint("apply_step")
        if any(getattr(m, "accum_steps", 1) > 1 for m in self.sub_modules):
            raise NotImplementedError("MegaNeRF: gradient accumulation (set_accumulation on a cell model) is not built for joint training")
        if any(getattr(m, "check_finite", False) for m in self.sub_modules):
            raise NotImplementedError(self._GUARD_JOINT)
        if grad_allreduce is not None:
            raise NotImplementedError("MegaNeRF: data parallelism (a gradient all-reduce over the cells' buffers) is not built")
        if res is not None and res.get("cell_overflow") is not None:
            dropped = res["cell_overflow"].tolist()
            if any(dropped):
                passes = [("coarse", res["ctx"])] + ([("fine", res["ctx_fine"])] if "ctx_fine" in res else [])
                what = "; ".join(f"{name}: cell capacity {c['C']}, members per cell {c['counts'].tolist()}" for name, c in passes)
                raise RuntimeError(f"MegaNeRF: {sum(dropped)} (point, cell) memberships of this batch did not fit their cell's rows ({what}): "
                                   "the step was computed without them and is not applied; raise cell_capacity")
        if not optimizer_step:
            return
        for m in self.sub_modules:
            m.step_count, m.lr = self.step_count, self.lr      # (the tail advances each cell's count, like the model's here)
        self.step_count += 1
        optim.apply_tail(self.sub_modules, refresh=refresh)

    def train_step(self, rgbs, rays, image_indices, n_samples, perturb=1.0, perturb_rand=None, sigma_noise=None, optimizer_step=True,
                   fine_samples=0, fine_u=None, sigma_noise_fine=None, cell_capacity=None, sigma_noise_std=0.0):
        """grad_step + apply_step; result keys as SwitchNeRF.train_step (loss, photo_loss, psnr, rgb, depth, depth_variance; gate_loss 0).
        cell_capacity: the padded form (module doc); a batch that overflows a cell raises RuntimeError with no parameter touched.
        sigma_noise_std: with device noise on (set_device_noise) the std of the sigma noise the step draws where none is supplied."""
        res = self.grad_step(rgbs, rays, image_indices, n_samples, perturb, perturb_rand, sigma_noise, fine_samples, fine_u, sigma_noise_fine,
                             cell_capacity, sigma_noise_std)
        self.apply_step(None, optimizer_step, res)
        return res


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
        z_f = o.sample_pdf(z_b.flip(-1).contiguous(), w_b, hier.default_fine_u(lin, Nb, Fb, 0.0, rays_b.device), Fb)
        _, dreal_f, p4f = o.bg_sample_pe(rays_b, center, radius, Fb, 0, torch.float32, 4, z_in=z_f)
        real = ro + rd * dreal_f.unsqueeze(-1) if cluster_2d else edge
        raw_f = _run(bg_nerf, _bg_points(rays_b, img_b, p4f, real, not sh), chunk, dirs)
        z_m, _, raw_m, dreal_m = hier.merge_flipped(z_f, z_b, raw_f, raw_b, dreal_f, dreal_b)
        rgb, depth, _, _, _ = o.composite_bounded_fwd(raw_m, z_m, None, True, dreal_m)
    return rgb, depth


def render_rays(nerf: MegaNeRF, bg_nerf, rays, image_indices, hparams, sphere_center=None, sphere_radius=None, get_depth: bool = True,
                get_depth_variance: bool = True, get_bg_fg_rgb: bool = False) -> Tuple[Dict[str, torch.Tensor], bool]:
    """rendering.render_rays for a MegaNeRF foreground (evaluation): the library's ray sampling, the [P, 3 + 3 + 1] points through the
    model per model_chunk_size, the library's compositing; fine_samples > 0: importance sampling from the coarse weights, the fine pass
    and the sort-merge of both sample sets, like SwitchNeRF.forward_hier.  A MegaNeRF returns a tensor, so there is no gate loss key
    (rendering.py:385-406).
    bg_nerf: the xyz_real MegaNeRF of the same container (model_utils.py:89-96).  Every ray is clipped at the foreground bound
    (swn_fg_bounds); the rays that leave it continue through _render_background and are blended in with the foreground's leftover
    transmittance (rendering.py:104-134), like background.BackgroundScene does for a dense background model.
    A model in training mode (joint_training, after train()) is refused: training runs through MegaNeRF.train_step, and the autograd
    bridge that would let this function return differentiable tensors for a MegaNeRF is a later change."""
    from .rendering import _gate_sigma_keys, _point_keys, _results
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
        raise NotImplementedError("device_noise_seed: mega.render_rays is evaluation and draws nothing - the seeded device noise of a "
                                  "MegaNeRF belongs to joint training (MegaNeRF.set_device_noise, then train_step)")
    if nerf.training or getattr(nerf, "graph_eval", False) or getattr(nerf, "graph_train", False):
        raise NotImplementedError("MegaNeRF renders in evaluation mode without graph capture (a joint_training model trains through "
                                  "MegaNeRF.train_step; call eval() before rendering)")
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
    raw_c, z_c, raw_f = raw, z, None
    if F == 0:
        typ, z_last = "coarse", z[:, -1]                          # stratified depths ascend: the last one is the maximum (:216)
    else:
        _, _, _, w = ops.composite_fwd(raw, z, want_weights=True)      # (the last delta only reaches the last weight, which :240 drops)
        z_fine = ops.sample_pdf(z, w, hier.default_fine_u(lin, N, F, 0.0, dev), F)      # evaluation: det = (perturb == 0)
        raw_f = _run(nerf, _points(rays, z_fine, image_indices, not sh), chunk, dirs)
        z, order, raw = ops.merge_samples(z_fine, z_c, raw_f, raw_c)
        typ, z_last = "fine", z_fine.max(dim=-1)[0]               # the FINE depths' maximum (:249-250)
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
    res.update(_results(typ, rgb, None, None, depth, dvar, get_depth, get_depth_variance))      # (a tensor model: no gate loss, no gates)
    _gate_sigma_keys(res, hparams, dict(raw=raw_c), None if raw_f is None else dict(raw=raw_f), N, S, F, gates=False)
    return res, Nb > 0
