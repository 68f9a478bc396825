"""The two-network cascade (--use_cascade): a coarse model that proposes depths and a separate fine model evaluated on the sorted
union of the coarse and the resampled depths, both trained.

Mirrors the reference's models/cascade.py (Cascade(coarse, fine): forward(use_coarse, x, sigma_only, sigma_noise) dispatches to a
half), built by models/model_utils.py:97-117 around two NeRFMoE or two NeRF instances, rendered by rendering.py:227-268 (the coarse
pass composited, fine depths = sort(cat[z_coarse, sample_pdf(...)]), the fine model on ALL S + F of them) and trained with
loss = (mse(rgb_fine) + mse(rgb_coarse)) / 2 (runner.py:1195-1204).  The state_dict layout is the reference's: coarse.<key>, fine.<key>.

Here the halves are two DenseNeRF instances of one cfg and dtype (SwitchNeRF halves are refused: see __init__).  A step is
    coarse.forward_rays(want_weights) -> swn_cascade_resample (the draws and their sorted union with the coarse depths, one launch)
    -> fine.forward_rays(z_in = z_union) -> swn_cascade_loss -> composite_bwd + backward_net per level, each into
    its own half's gradient buffer -> one Adam step per half.
No gradient flows through the depths (the reference detaches the weights, rendering.py:240), there is no merge and no `order`.
"""
from __future__ import annotations

import torch

from . import ops, optim
from .dense import DenseNeRF
from .model import SwitchNeRF


def _refuse(what):
    raise NotImplementedError(f"Cascade: {what} is not built for the two-network cascade")


class Cascade:
    is_cascade = True        # what rendering.render_rays dispatches on

    def __init__(self, coarse, fine=None):
        for name, half in (("coarse", coarse), ("fine", fine)):
            if half is None and name == "fine":
                continue
            if getattr(half, "is_mega_nerf", False):
                _refuse("a Mega-NeRF half (container_path / train_mega_nerf)")
            if isinstance(half, SwitchNeRF) and not isinstance(half, DenseNeRF):
                # no fixture of the reference's own MoE Cascade can pin the routing (at 10^4 points per level some top-1 / top-2 logit
                # gap always lies within the fp32 logit error), so the MoE halves would run unchecked: refused until that is solved
                _refuse("MoE halves (SwitchNeRF; the dense NeRF only)")
            if type(half) is not DenseNeRF:
                raise TypeError(f"Cascade: the {name} half must be a DenseNeRF, got {type(half).__name__}")
            if getattr(half, "sh_deg", None) is not None:
                _refuse("a half with spherical-harmonics colour (sh_deg)")
            if getattr(half, "affine", False):
                _refuse("a half with the affine colour transform (affine_appearance)")
        if fine is not None:
            if fine is coarse:
                raise ValueError("Cascade: the halves must be two models, not one model twice")
            if dict(fine.cfg) != dict(coarse.cfg):
                raise ValueError("Cascade: both halves must be built from the same cfg")
            if fine.dtype != coarse.dtype:
                raise ValueError(f"Cascade: both halves must have one compute dtype, got {coarse.dtype} and {fine.dtype}")
        self.coarse, self.fine = coarse, fine
        # fp16: ONE loss scaler for the step - both halves backward with its scale and skip a step together
        self.loss_scaler = coarse.loss_scaler
        if fine is not None and fine.loss_scaler is not None:
            fine.loss_scaler = self.loss_scaler

    # ------------------------------------------------------------------------------------------ module mirrors
    def halves(self):
        return [self.coarse] + ([self.fine] if self.fine is not None else [])

    def _named_halves(self):
        return [("coarse", self.coarse)] + ([("fine", self.fine)] if self.fine is not None else [])

    @property
    def training(self):
        return self.coarse.training

    @property
    def dtype(self):
        return self.coarse.dtype

    @property
    def dev(self):
        return self.coarse.dev

    @property
    def moe_no_batch(self):
        return self.coarse.moe_no_batch

    def train(self, mode=True):
        for h in self.halves():
            h.train(mode)
        return self

    def eval(self):
        return self.train(False)

    def modules(self):
        yield self
        for h in self.halves():
            yield from h.modules()

    def set_no_batch(self, mode=True):
        for h in self.halves():
            h.set_no_batch(mode)

    def __call__(self, use_coarse, x, sigma_only=False, sigma_noise=None):
        """Cascade.forward (models/cascade.py:13-18)."""
        if not use_coarse and self.fine is None:
            raise ValueError("Cascade: no fine half (built with fine = None for fine_samples == 0)")
        return (self.coarse if use_coarse else self.fine)(x, sigma_only, sigma_noise)

    def state_dict(self, **kw):
        sd = {}
        for name, h in self._named_halves():
            sd.update(h.state_dict(prefix=name + ".", **kw))
        return sd

    def load_state_dict(self, sd):
        from . import checkpoint
        sd = checkpoint.strip_module_prefix(sd)
        for name, h in self._named_halves():
            part = {k[len(name) + 1:]: v for k, v in sd.items() if k.startswith(name + ".")}
            if not part:
                raise KeyError(f"Cascade.load_state_dict: no '{name}.' keys")
            h.load_state_dict(part)
        if self.fine is None and any(k.startswith("fine.") for k in sd):
            raise ValueError("Cascade.load_state_dict: the state has a fine half, this cascade was built without one")

    def named_parameters(self):
        for name, h in self._named_halves():
            for k, v in h.named_parameters():
                yield name + "." + k, v

    def parameters(self):
        return (v for _, v in self.named_parameters())

    def trainable_parameters(self):
        """The two flat_param leaves (coarse, fine): what torch.optim.Adam is given."""
        return [h.flat_param for h in self.halves()]

    # ------------------------------------------------------------------------------------------ what stays refused
    def _check_runtime(self):
        for h in self.halves():
            if getattr(h, "device_noise", False) or getattr(getattr(h, "noise", None), "owner", None) is not None:
                _refuse("seeded device noise (set_device_noise)")
            if getattr(h, "graph_train", False) or getattr(h, "graph_eval", False):
                _refuse("graph capture (graph_train / graph_eval)")
            if getattr(h, "ep", None) is not None:
                _refuse("expert or data parallelism (set_expert_parallel)")

    def set_device_noise(self, *a, **k):
        _refuse("seeded device noise (set_device_noise)")

    def set_expert_parallel(self, *a, **k):
        _refuse("expert or data parallelism (set_expert_parallel)")

    def forward_mip(self, *a, **k):
        _refuse("the mip path (forward_mip / render_rays_mip)")

    train_step_mip = forward_mip

    # ------------------------------------------------------------------------------------------ forward
    def forward_cascade(self, rays, image_indices, n_samples, fine_samples, seg_tokens, perturb=0.0, perturb_rand=None, fine_u=None,
                        sigma_noise=None, sigma_noise_fine=None, no_batch=False, training=True, sigma_noise_std=0.0):
        """_get_results with use_cascade (rendering.py:199-274) -> (coarse ctx, fine ctx), each composited on its own rows; the fine
        ctx is None with fine_samples == 0.  sigma_noise_fine has N (S + F) entries.  The fine ctx also holds "z_union"."""
        self._check_runtime()
        if sigma_noise_std:
            _refuse("seeded device noise (sigma_noise_std)")
        N, S, F = rays.shape[0], int(n_samples), int(fine_samples)
        c = self.coarse.forward_rays(rays, image_indices, S, seg_tokens, perturb, perturb_rand, sigma_noise, training, None,
                                     no_batch=no_batch, want_weights=F > 0)
        if F == 0:
            return c, None
        if self.fine is None:
            raise ValueError("Cascade: fine_samples > 0 needs a fine half")
        fm = self.fine
        if fine_u is None and perturb != 0:                               # det = (perturb == 0): the kernel's linspace (rendering.py:605-609)
            fine_u = torch.rand(N, F, device=rays.device)
        zu, _ = ops.cascade_resample(c["z"], c["weights"], fine_u, F)
        cf = fm.forward_rays(rays, image_indices, S + F, min(seg_tokens, N * (S + F)), 0.0, None, sigma_noise_fine, training, None,
                             no_batch=no_batch, z_in=zu, tag="f")
        cf["z_union"] = zu
        return c, cf

    # ------------------------------------------------------------------------------------------ training step
    def grad_step(self, rgbs, rays, image_indices, n_samples, seg_tokens, perturb=1.0, perturb_rand=None, sigma_noise=None,
                  routing_override=None, fine_samples=0, fine_u=None, sigma_noise_fine=None, split=False, sigma_noise_std=0.0,
                  coarse_photo=True):
        """Forward + loss + backward of one cascade step: each half's gradient buffer is zeroed and filled.  SwitchNeRF.grad_step's
        result keys, plus coarse_loss and rgb_coarse; with fine_samples == 0 it IS the coarse half's step."""
        if split:
            _refuse("grad_step(split=True)")
        if routing_override is not None:
            _refuse("routing_override")
        if fine_samples <= 0:
            self._check_runtime()
            return self.coarse.grad_step(rgbs, rays, image_indices, n_samples, seg_tokens, perturb, perturb_rand, sigma_noise)
        cm, fm = self.coarse, self.fine
        cm.grad.zero_()
        fm.grad.zero_()
        c, cf = self.forward_cascade(rays, image_indices, n_samples, fine_samples, seg_tokens, perturb, perturb_rand, fine_u, sigma_noise,
                                     sigma_noise_fine, training=True, sigma_noise_std=sigma_noise_std)
        ls = optim.sync_loss_scale((cm, fm))      # (each half's record of the scale the backward uses: what its Adam step divides by)
        out5, d_f, d_c, d_lf, d_lc = ops.cascade_loss(cf["rgb"], c["rgb"], rgbs.to(torch.float32).contiguous(), cf["l_aux"], c["l_aux"],
                                                      cm.wt, coarse_photo, ls)
        fm.backward(cf, d_f, d_lf)
        cm.backward(c, d_c, d_lc)
        guard = dict(step_ok=cm._finite_guard(out5, 4)) if cm.check_finite else {}      # ONE check over both halves' metrics
        return dict(**guard, loss=out5[3], photo_loss=out5[0], coarse_loss=out5[1], gate_loss=out5[2], psnr=out5[4],
                    depth_variance=cf["depth_variance"].mean(), ctx=c, ctx_fine=cf, rgb=cf["rgb"], rgb_coarse=c["rgb"], depth=cf["depth"])

    @property
    def accum_steps(self) -> int:
        return self.coarse.accum_steps

    def set_accumulation(self, steps: int):
        """SwitchNeRF.set_accumulation on both halves: ONE window (the coarse half's micro-step index) and one scale over the two,
        each half with its own buffer."""
        for h in self.halves():
            h.set_accumulation(steps)

    @property
    def check_finite(self) -> bool:
        return self.coarse.check_finite

    def set_check_finite(self, on: bool = True):
        """SwitchNeRF.set_check_finite over the halves: ONE flag and one counter (the coarse half's) for the step's five metrics, as the
        reference's single check; each half keeps its own device step count."""
        self.coarse.set_check_finite(on)
        if self.fine is not None:
            self.fine.set_check_finite(on, share=self.coarse)

    def skipped_steps(self) -> int:
        return self.coarse.skipped_steps()

    def finite_guard_state_dict(self) -> dict:
        return {name: h.finite_guard_state_dict() for name, h in self._named_halves()}

    def load_finite_guard_state_dict(self, sd: dict):
        self.set_check_finite(bool(sd["coarse"].get("check_finite", False)))
        for name, h in self._named_halves():
            h.step_count = int(sd[name].get("step_count", h.step_count))
        if self.check_finite:
            self.coarse._guard["skipped"].fill_(int(sd["coarse"].get("skipped_steps", 0)))

    def apply_step(self, grad_allreduce=None, optimizer_step=True, should_accumulate=None):
        """One Adam step per half, each with its own step count (optim.apply_tail over the halves).  fp16: found-inf is the OR over
        the halves, the one scaler is updated once and both halves skip - or take - the step together.  With gradient accumulation on
        (set_accumulation) -> whether the optimizers stepped (should_accumulate: SwitchNeRF.apply_step)."""
        if grad_allreduce is not None:
            _refuse("expert or data parallelism (grad_allreduce)")
        stepped = optim.apply_tail(self.halves(), skip_together=True, optimizer_step=optimizer_step, should_accumulate=should_accumulate)
        return stepped if self.accum_steps > 1 else None

    def train_step(self, rgbs, rays, image_indices, n_samples, seg_tokens, perturb=1.0, perturb_rand=None, sigma_noise=None,
                   optimizer_step=True, routing_override=None, grad_allreduce=None, fine_samples=0, fine_u=None, sigma_noise_fine=None,
                   sigma_noise_std=0.0, coarse_photo=True, should_accumulate=None):
        if fine_samples <= 0:
            if grad_allreduce is not None:
                _refuse("expert or data parallelism (grad_allreduce)")
            self._check_runtime()
            return self.coarse.train_step(rgbs, rays, image_indices, n_samples, seg_tokens, perturb, perturb_rand, sigma_noise,
                                          optimizer_step, should_accumulate=should_accumulate)
        res = self.grad_step(rgbs, rays, image_indices, n_samples, seg_tokens, perturb, perturb_rand, sigma_noise, routing_override,
                             fine_samples, fine_u, sigma_noise_fine, sigma_noise_std=sigma_noise_std, coarse_photo=coarse_photo)
        stepped = self.apply_step(grad_allreduce, optimizer_step, should_accumulate=should_accumulate)
        if self.accum_steps > 1:
            res["optimizer_stepped"] = stepped
        return res
