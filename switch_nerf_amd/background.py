"""Foreground model + background model rendering: render_rays' bg_nerf branch
(/root/reference/switch_nerf/rendering.py:32-159; the default of the Mega-NeRF scenes, opts.py:89, with the ellipsoidal
bound the runner derives from the camera positions, runner.py:221-243).

  * every ray is clipped at the foreground bound (swn_fg_bounds); the foreground network (SwitchNeRF) samples
    [near, min(far, fg_far)] and its last sample's delta is the distance left to the bound (:42, :216-217);
  * rays with far > fg_far continue into the background model - the reference's dense NeRF over the NeRF++ inverted-sphere
    parametrisation (4-D points, DenseNeRF with xyz_dim 4) - on coarse_samples // 2 inverse-distance samples evaluated
    in descending order (swn_bg_sample_pe, flip);
  * rgb / depth of both are blended with the foreground's leftover transmittance bg_lambda (:104-131), whose gradient
    flows back into the foreground densities (swn_composite_bounded_bwd).

With fine_samples > 0 both models run the hierarchical pass (fine_samples // 2 for the background, :241).  One reference
quirk is mirrored deliberately: the background's importance sampling pairs the ASCENDING bin mid points (:238 uses
_get_results' own un-flipped z_vals) with the coarse weights in FLIPPED order (computed by _inference on its flipped
copy, :302-304), and its depth map reads the un-flipped depth_real (:483-484); tests/golden/bg_train_*.npz pin both.

Seeded device noise (BackgroundScene.set_device_noise; csrc/philox.hpp): the scene owns the state and ONE device step counter for both
models.  The foreground model draws its own streams through that counter exactly as it does without a background; the background's
draws live in the generator's second domain and are addressed through each background ray's position in the batch (idx_bg), so a
background ray's noise depends on (seed, step, global ray) only - not on which other rays of the batch leave the bound.

Two forms of the background rows.  The COMPACT form (default, bg_capacity=None) mirrors the reference: the background rays are found
with nonzero() and every background tensor has exactly Nb rows - a host read per step, so the step cannot be captured into a hipGraph.
The PADDED form (bg_capacity=C, 1 <= C <= N) runs the background model on C rows whatever the batch: swn_bg_compact puts the batch's
n_bg background rays into the first rows in ascending ray order and fills the rest with a benign ray; n_bg stays on the device.  A
padding row's activations are finite and its dL/d rgb is exactly 0 (swn_bg_blend_bwd), so it adds exact zeros to every gradient sum;
swn_bg_blend_fwd skips it.  Nothing is read on the host until ONE 8-byte readback of (n_bg, n_out) behind the step's last launch
(apply_step) - which is what graph.GraphedBackgroundStep captures.  C < N saves the padding's work on scenes where few rays leave the
bound; a batch with n_bg > C is refused (RuntimeError) before any parameter is touched.
"""
from __future__ import annotations

import torch

from . import hier, ops, optim
from .noise import DeviceNoise


class BackgroundScene:
    """nerf: SwitchNeRF (foreground), bg_nerf: DenseNeRF with cfg xyz_dim = 4; sphere_center / sphere_radius: 3 floats each
    (tensors or sequences) or both None for the unit sphere."""

    def __init__(self, nerf, bg_nerf, sphere_center=None, sphere_radius=None):
        assert getattr(bg_nerf, "xyz_dim", 3) == 4, "the background model takes the 4-D inverted-sphere points (get_bg_nerf: xyz_dim 4)"
        if getattr(nerf, "affine", False):      # (the reference builds BOTH models from hparams.affine_appearance: model_utils.py:90-120)
            raise NotImplementedError("affine_appearance is not built for scenes with a background model: the dense background NeRF "
                                      "(models/nerf.py:117) has no affine branch")
        if getattr(nerf, "sh_deg", None) is not None or getattr(bg_nerf, "sh_deg", None) is not None:
            raise NotImplementedError("sh_deg: spherical-harmonics colour is not built for scenes with a background model")
        self.nerf, self.bg = nerf, bg_nerf
        self.center, self.radius = sphere_center, sphere_radius
        bg_nerf._grow_bufs = True           # the number of background rays changes every batch
        self.dev = nerf.dev
        self.noise, self._fg_noise = DeviceNoise(), None      # the ONE noise state of both models (set_device_noise)
        # ONE loss scaler over both models (the reference's single GradScaler over both optimizers, runner.py:483, 679-690): when either
        # model computes in fp16, both hold the SAME LossScaler object - one scale multiplies the loss gradient, both unscale by it, one
        # growth tracker is checkpointed whichever model's state_dict is asked (a 16-bit-float foreground beside an fp16 background included)
        # This MUTATES both models (documented contract of a scene): a model that had no scaler gains one, the background's own
        # scaler state is replaced by the foreground's.  Build the scene BEFORE capturing graphs on its models (a graph captured on a
        # scaler-less model does not read the scale); detach() hands the models back their own scalers.
        self._own_scalers = (nerf.loss_scaler, bg_nerf.loss_scaler)
        self.loss_scaler = nerf.loss_scaler if nerf.loss_scaler is not None else bg_nerf.loss_scaler
        if self.loss_scaler is not None:
            for m in (nerf, bg_nerf):
                if m.loss_scaler is not self.loss_scaler and getattr(m, "_train_graphs", None):
                    raise RuntimeError("BackgroundScene: a model whose training graphs were captured before the scene was built would keep "
                                       "running without the shared loss scale; build the scene first")
            nerf.loss_scaler = bg_nerf.loss_scaler = self.loss_scaler

    def detach(self):
        """Undo the scaler sharing: each model gets back the LossScaler (or None) it had before the scene was built; a model that owned
        one continues from the shared scale.  The foreground model gets back the noise state it had before set_device_noise."""
        self.set_device_noise(None)
        for m, own in zip((self.nerf, self.bg), self._own_scalers):
            if own is not None and self.loss_scaler is not None and own is not self.loss_scaler:
                own.load_state_dict(self.loss_scaler.state_dict())
            m.loss_scaler = own
            if own is None:
                m._ls_dev = None

    # ------------------------------------------------------------------------------------------ seeded device noise
    def set_device_noise(self, seed, step: int = 0, ray_base: int = 0):
        """Seeded device-side noise for both models (SwitchNeRF.set_device_noise has the contract); seed = None switches it off and hands
        the foreground model back the noise state it had.  On: the foreground model is switched on with the same seed and the SAME counter
        tensor, so it draws its streams as it does without a background; a TRAINING forward draws what the caller does not supply for the
        background model - jitter, coarse / fine sigma noise (noise_std > 0), fine u - from the generator's background domain, background
        row j being global ray ray_base + idx_bg[j].  train_step ends in one advance of the counter.  While it is on the model holds a
        lent copy of self.noise (DeviceNoise.lend) and self._fg_noise keeps the model's own object, from before the FIRST switch-on."""
        nerf, was_on = self.nerf, self.noise.on
        self.noise.set(seed, step, ray_base, self.dev)
        if seed is None:
            if was_on:
                nerf.noise = self._fg_noise
            self._fg_noise = None
            return
        if not was_on:
            self._fg_noise = nerf.noise
        nerf.noise = self.noise.lend(self)       # (rendering._device_noise: this model's noise is the scene's business)

    @property
    def device_noise(self) -> bool:
        return self.noise.on

    def set_ray_base(self, ray_base: int):
        """The global index of this process's first ray (parallel.shard_rays(..., model=scene)), for both models.  Nothing to set while
        the noise is off: set_device_noise takes the ray_base it starts with."""
        self.noise.set_base(ray_base)
        if self.noise.on:
            self.nerf.set_ray_base(ray_base)

    def noise_state_dict(self) -> dict:
        """{"seed", "step", "ray_base"} of the scene (both models): what a resume needs besides the parameters.  Reads the step back."""
        return self.noise.state_dict()

    def load_noise_state_dict(self, sd: dict):
        self.set_device_noise(sd.get("seed"), int(sd.get("step", 0)), int(sd.get("ray_base", 0)))

    def _noise_advance(self):
        """The one advance of the shared step counter that ends a training step.  Nothing with the noise off."""
        self.noise.advance()

    def _check_noise_sources(self):
        """Never mix the two noise sources silently: a model drawing seeded noise of its own inside a scene that draws the background's
        from the framework generator (or from another counter) is an error."""
        nerf, bg = self.nerf, self.bg
        if getattr(bg, "device_noise", False):
            raise RuntimeError("BackgroundScene: the background model's own device noise is on (bg_nerf.set_device_noise): the scene "
                               "carries the noise of both models - turn it off there and call BackgroundScene.set_device_noise(seed)")
        if not self.noise.on and getattr(nerf, "device_noise", False):
            raise RuntimeError("BackgroundScene: the foreground model's device noise is on but the scene's is not, so the background "
                               "would draw from the framework generator - call BackgroundScene.set_device_noise(seed) instead of "
                               "the model's set_device_noise (or turn the model's off)")
        if self.noise.on and (nerf.noise.step is not self.noise.step or not nerf.noise.on or nerf.noise.seed != self.noise.seed):
            raise RuntimeError("BackgroundScene: the foreground model's device noise was changed behind the scene's back "
                               "(SwitchNeRF.set_device_noise after BackgroundScene.set_device_noise): set it on the scene")

    # ------------------------------------------------------------------------------------------ forward
    def forward(self, rays, image_indices, n_samples, seg_tokens, perturb=0.0, perturb_rand=None, perturb_rand_bg=None,
                sigma_noise=None, sigma_noise_bg=None, fine_samples=0, fine_u=None, fine_u_bg=None, sigma_noise_fine=None,
                sigma_noise_bg_fine=None, no_batch=False, noise_std=0.0, training=True, ray_index=None, bg_capacity=None,
                ray_index_limit=None):
        """sigma_noise_bg / sigma_noise_bg_fine: [Nb * samples] tensors, or the string "randn" to draw noise_std * N(0,1)
        here (the number of background rays is only known inside).
        The scene's device noise on (set_device_noise) and a training pass: what is not supplied is drawn from the seeded generator -
        the foreground's as SwitchNeRF does it (sigma noise of std noise_std), the background's jitter inside swn_bg_sample_pe_rng, its
        sigma noise (noise_std > 0; "randn" or None) and fine u through swn_rng_fill_rows; the drawn tensors are kept in ctx["bg"]
        ("sigma_noise", "fine_u", "sigma_noise_fine").  Supplied tensors win.
        ray_index (int64 [N], optional): the position in the full batch of each ray of this call - the BACKGROUND's draws are addressed
        by ray_base + ray_index[i] instead of ray_base + i (a call on a subset of a batch reproduces that batch's background draws).
        bg_capacity = C (an int, 1 <= C <= N): the padded form (module doc) - the background tensors, supplied noise included
        (perturb_rand_bg [C, Sb], sigma_noise_bg [C * Sb], fine_u_bg [C, Fb], sigma_noise_bg_fine [C * Fb]), have C rows of which the
        first n_bg are meaningful; ctx carries "C", "n_bg_dev", "n_out_dev", and ctx["Nb"] stays None until the host has read the
        count (read_counts).  The out-of-bound and overflow checks happen there, not here.  ray_index then needs ray_index_limit (an
        exclusive upper bound of its entries, e.g. the full batch's rays) instead of a host read of its maximum."""
        o, nerf, bg = ops, self.nerf, self.bg
        self._check_noise_sources()
        dn = self.noise if training and self.noise.on else None
        N, S, Fn = rays.shape[0], n_samples, int(fine_samples)
        padded = bg_capacity is not None
        if padded:
            Nb = int(bg_capacity)                # the ROW count of every background tensor below
            if not 1 <= Nb <= N:
                raise ValueError(f"bg_capacity {Nb} outside [1, {N} rays]")
            if ray_index is not None and ray_index_limit is None:
                raise ValueError("bg_capacity with ray_index needs ray_index_limit (the padded form reads nothing on the host)")
            counts = torch.zeros(2, dtype=torch.int32, device=self.dev)           # (n_bg, n_out): read back together, once
            rays_fg, fg_far, last0, has_bg, n_out = o.fg_bounds(rays, self.center, self.radius, n_out=counts[1:])
            idx_bg, n_bg_dev, rays_b, img_b = o.bg_compact(has_bg, rays, image_indices.contiguous(), Nb,
                                                           o.bg_pad_ray(self.center, self.radius), n_bg=counts[:1])
            ctx = dict(N=N, S=S, F=Fn, idx_bg=idx_bg, Nb=None, C=Nb, n_bg_dev=n_bg_dev, n_out_dev=n_out, counts_dev=counts,
                       fg_far=fg_far, has_bg=has_bg)
        else:
            rays_fg, fg_far, last0, has_bg, n_out = o.fg_bounds(rays, self.center, self.radius)
            idx_bg = has_bg.nonzero().view(-1)                      # rays_with_bg, rendering.py:36 (host sync, like the reference)
            if int(n_out.item()) > 0:
                raise Exception(self._UNBOUNDED)
            Nb = idx_bg.numel()
            ctx = dict(N=N, S=S, F=Fn, idx_bg=idx_bg, Nb=Nb, fg_far=fg_far, has_bg=has_bg)
        # ---- background first (the reference's order, and so the order of its random draws)
        if Nb > 0:
            Sb = S // 2
            if not padded:
                rays_b = rays.index_select(0, idx_bg).contiguous()
                img_b = image_indices.index_select(0, idx_bg).contiguous()
            drawn = {}
            if dn is not None:               # background row j is global ray ray_base + rows[j]; every entry < lim
                if ray_index is None:
                    rows, lim = idx_bg, N
                else:
                    rows = ray_index.index_select(0, idx_bg)
                    lim = int(ray_index_limit) if ray_index_limit is not None else int(ray_index.max().item()) + 1
                draw = lambda stream, per_row, kind, scale=1.0: o.rng_fill_rows(
                    Nb, per_row, dn.base, rows, kind, dn.seed, dn.step, stream, o.RNG_DOMAIN_BG, scale, lim)
            if dn is not None and perturb > 0 and perturb_rand_bg is None:
                z_b, dreal_b, pe_b = o.bg_sample_pe_rng(rays_b, self.center, self.radius, Sb, bg.cfg["pos_xyz_dim"], bg.dtype, bg.KP,
                                                        dn.seed, dn.step, dn.base, rows, lim, float(perturb),
                                                        pe_out=bg._buf("c:pe", (Nb * Sb, bg.KP), bg.dtype))
            else:
                if perturb > 0 and perturb_rand_bg is None:
                    perturb_rand_bg = torch.rand(Nb, Sb, device=self.dev)
                z_b, dreal_b, pe_b = o.bg_sample_pe(rays_b, self.center, self.radius, Sb, bg.cfg["pos_xyz_dim"], bg.dtype, bg.KP,
                                                    perturb_rand_bg, float(perturb), pe_out=bg._buf("c:pe", (Nb * Sb, bg.KP), bg.dtype))
            pe_dir_b = bg._dir_pe(rays_b)
            if dn is not None and noise_std > 0 and (sigma_noise_bg is None or isinstance(sigma_noise_bg, str)):
                sigma_noise_bg = drawn["sigma_noise"] = draw(o.RNG_SIGMA, Sb, o.RNG_NORMAL, float(noise_std)).view(-1)
            if isinstance(sigma_noise_bg, str):
                sigma_noise_bg = torch.randn(Nb * Sb, device=self.dev) * noise_std
            cb = bg._net_forward(pe_b, pe_dir_b, img_b, Nb, Sb, Nb * Sb, sigma_noise_bg, None, False, "c", saving=bool(training))
            cb["z"], cb["depth_real"] = z_b, dreal_b
            rgb_b, depth_b, _, w_b, _ = o.composite_bounded_fwd(cb["raw"], z_b, None, True, dreal_b, want_weights=Fn > 0)
            b = dict(c=cb, raw=cb["raw"], z=z_b)
            if Fn > 0:
                Fb = Fn // 2
                if dn is not None and fine_u_bg is None and perturb != 0:
                    fine_u_bg = drawn["fine_u"] = draw(o.RNG_FINE_U, Fb, o.RNG_UNIFORM)
                if fine_u_bg is None:
                    fine_u_bg = hier.default_fine_u(bg._linspace, Nb, Fb, perturb, self.dev)
                if dn is not None and noise_std > 0 and (sigma_noise_bg_fine is None or isinstance(sigma_noise_bg_fine, str)):
                    sigma_noise_bg_fine = drawn["sigma_noise_fine"] = draw(o.RNG_SIGMA_FINE, Fb, o.RNG_NORMAL, float(noise_std)).view(-1)
                if isinstance(sigma_noise_bg_fine, str):
                    sigma_noise_bg_fine = torch.randn(Nb * Fb, device=self.dev) * noise_std
                z_f = o.sample_pdf(z_b.flip(-1).contiguous(), w_b, fine_u_bg, Fb)        # ascending bins x flipped weights (see module doc)
                _, dreal_f, pe_f = o.bg_sample_pe(rays_b, self.center, self.radius, Fb, bg.cfg["pos_xyz_dim"], bg.dtype, bg.KP,
                                                  z_in=z_f, pe_out=bg._buf("f:pe", (Nb * Fb, bg.KP), bg.dtype))
                cfb = bg._net_forward(pe_f, pe_dir_b, img_b, Nb, Fb, Nb * Fb, sigma_noise_bg_fine, None, False, "f", saving=bool(training))
                z_m, order, raw_m, dreal_m = hier.merge_flipped(z_f, z_b, cfb["raw"], cb["raw"], dreal_f, dreal_b)
                rgb_b, depth_b, _, _, _ = o.composite_bounded_fwd(raw_m, z_m, None, True, dreal_m)
                b.update(cf=cfb, raw=raw_m, z=z_m, order=order, z_fine=z_f)
            b.update(rgb=rgb_b, depth=depth_b, **drawn)       # (the draws of this pass, for inspection; a supplied tensor is the caller's)
            ctx["bg"] = b
        # ---- foreground on the clipped rays
        std_fg = float(noise_std) if dn is not None else 0.0       # device noise: the foreground draws its own sigma noise (streams 1 / 3)
        if Fn == 0:
            c = ctx["c"] = nerf.forward_rays(rays_fg, image_indices, S, seg_tokens, perturb, perturb_rand, sigma_noise, training, None,
                                             no_batch=no_batch, composite=False, sigma_noise_std=std_fg)
            raw, z, z_last = c["raw"], c["z"], c["z"][:, -1]              # stratified depths ascend: the last one is the maximum (:217)
        else:                    # (the fine u is drawn - stream 2 - or defaulted as SwitchNeRF.forward_hier does it)
            c, cf, z_fine, z, order, raw = nerf.hier_passes(rays_fg, image_indices, S, Fn, seg_tokens, perturb, perturb_rand, fine_u,
                                                            sigma_noise, sigma_noise_fine, None, no_batch, training, std_fg)
            z_last = z_fine.max(dim=-1)[0]                               # the FINE depths' maximum (:249-250)
            ctx.update(c=c, cf=cf, order=order, z_fine=z_fine)
        last_delta = torch.where(has_bg > 0, fg_far - z_last, last0).contiguous()          # :216-217 / :249-250
        rgb, depth, dvar, _, lam = o.composite_bounded_fwd(raw, z, last_delta, False, None, want_bg_lambda=True)
        ctx.update(raw=raw, z=z, last_delta=last_delta, bg_lambda=lam, fg_rgb=rgb, fg_depth=depth, depth_variance=dvar)
        if padded:                                                        # :104-131 on the first n_bg rows (swn_bg_blend_fwd)
            rgb, depth = o.bg_blend_fwd(rgb.clone(), depth.clone(), idx_bg, ctx["n_bg_dev"], lam, ctx["bg"]["rgb"], ctx["bg"]["depth"])
        elif Nb > 0:                                                      # :104-131
            lam_b = lam.index_select(0, idx_bg)
            rgb = rgb.index_add(0, idx_bg, ctx["bg"]["rgb"] * lam_b[:, None])
            depth = depth.index_add(0, idx_bg, ctx["bg"]["depth"] * lam_b)
        ctx.update(rgb=rgb, depth=depth)
        return ctx

    # ------------------------------------------------------------------------------------------ backward
    def backward(self, ctx, d_rgb, wt_coarse, wt_fine=0.0, loss_scale_dev=None, bg_capacity=None):
        """Accumulates both models' parameter gradients given dL/d rgb [N,3]; wt_* = the weight of each level's mean gate loss.
        loss_scale_dev: a device scalar the gate-loss weights are multiplied by (the loss scale of a step that reads nothing on the
        host; d_rgb then carries it already).  The form follows the context's; bg_capacity, when given, must be the forward's."""
        o, nerf, bg = ops, self.nerf, self.bg
        S, Fn, idx_bg = ctx["S"], ctx["F"], ctx["idx_bg"]
        padded = ctx.get("C") is not None
        if bg_capacity is not None and int(bg_capacity) != ctx.get("C"):
            raise ValueError(f"backward: bg_capacity {bg_capacity} but the forward ran with {ctx.get('C')}")
        d_lam = None
        if padded or ctx["Nb"] > 0:
            b = ctx["bg"]
            if padded:                       # dL/d rgb of a padding row is exactly 0: the row adds zeros to every sum behind it
                d_lam, d_rgb_b = o.bg_blend_bwd(d_rgb, idx_bg, ctx["n_bg_dev"], ctx["bg_lambda"], b["rgb"])
            else:
                d_rgb_sel = d_rgb.index_select(0, idx_bg)
                d_lam = torch.zeros(ctx["N"], dtype=torch.float32, device=self.dev)
                d_lam.index_copy_(0, idx_bg, (d_rgb_sel * b["rgb"]).sum(-1))
                d_rgb_b = (d_rgb_sel * ctx["bg_lambda"].index_select(0, idx_bg)[:, None]).contiguous()
            d_raw_b = o.composite_bounded_bwd(b["raw"], b["z"], d_rgb_b, None, True, None)
            if Fn > 0:
                d_f, d_c = o.unmerge_grad(d_raw_b, b["order"], Fn // 2, S // 2)
                bg.backward_net(b["cf"], d_f)
                bg.backward_net(b["c"], d_c)
            else:
                bg.backward_net(b["c"], d_raw_b)
        d_raw = o.composite_bounded_bwd(ctx["raw"], ctx["z"], d_rgb, ctx["last_delta"], False, d_lam)
        c = ctx["c"]
        def full(cc, w):
            t = torch.full((cc["n_seg"],), w / cc["n_seg"], dtype=torch.float32, device=self.dev)
            return t if loss_scale_dev is None else t * loss_scale_dev
        if Fn > 0:
            d_f, d_c = o.unmerge_grad(d_raw, ctx["order"], Fn, S)
            nerf.backward_net(ctx["cf"], d_f, full(ctx["cf"], wt_fine))
            nerf.backward_net(c, d_c, full(c, wt_coarse))
        else:
            nerf.backward_net(c, d_raw, full(c, wt_coarse))

    # ------------------------------------------------------------------------------------------ training step
    _UNBOUNDED = "Not all your cameras are bounded by the unit sphere; please make sure the cameras are normalized properly!"

    def train_step(self, rgbs, rays, image_indices, n_samples, seg_tokens, perturb=1.0, optimizer_step=True, grad_allreduce=None,
                   fine_samples=0, bg_capacity=None, should_accumulate=None, **kw):
        """Runner._training_step with a background model (runner.py:1077-1123): loss = mse(rgb) + wt * gate loss of the
        foreground MoE (the dense background model has none); both models take an Adam step (runner.py:305-318 builds one
        optimizer over the parameters of both).  = grad_step + apply_step.  bg_capacity: the padded form (module doc).
        should_accumulate: with gradient accumulation on (set_accumulation), see apply_step."""
        if self.accum_steps > 1 and bg_capacity is not None:
            raise NotImplementedError(self._ACCUM_PADDED)
        if self.check_finite and bg_capacity is not None:
            raise NotImplementedError(self._GUARD_PADDED)
        res = self.grad_step(rgbs, rays, image_indices, n_samples, seg_tokens, perturb, fine_samples, bg_capacity, **kw)
        return self.apply_step(res, optimizer_step, grad_allreduce, should_accumulate=should_accumulate)

    # ------------------------------------------------------------------------------------------ gradient accumulation
    _ACCUM_PADDED = ("BackgroundScene: gradient accumulation (set_accumulation) is built for the compact eager step only, not for the "
                     "padded form (bg_capacity=) or GraphedBackgroundStep")

    @property
    def accum_steps(self) -> int:
        return self.nerf.accum_steps

    # ------------------------------------------------------------------------------------------ finite guard
    _GUARD_PADDED = ("BackgroundScene: the finite guard (check_finite) is built for the compact eager step only, not for the padded "
                     "form (bg_capacity=) or GraphedBackgroundStep")

    @property
    def check_finite(self) -> bool:
        return self.nerf.check_finite

    def set_check_finite(self, on: bool = True):
        """SwitchNeRF.set_check_finite over both models: ONE flag and one counter (the foreground model's) for the step's metrics,
        each model with its own device step count.  The compact eager step only."""
        self.nerf.set_check_finite(on)
        self.bg.set_check_finite(on, share=self.nerf)

    def skipped_steps(self) -> int:
        return self.nerf.skipped_steps()

    def finite_guard_state_dict(self) -> dict:
        return dict(nerf=self.nerf.finite_guard_state_dict(), bg_nerf=self.bg.finite_guard_state_dict())

    def load_finite_guard_state_dict(self, sd: dict):
        self.set_check_finite(bool(sd["nerf"].get("check_finite", False)))
        for name, m in (("nerf", self.nerf), ("bg_nerf", self.bg)):
            m.step_count = int(sd[name].get("step_count", m.step_count))
        if self.check_finite:
            self.nerf._guard["skipped"].fill_(int(sd["nerf"].get("skipped_steps", 0)))

    def set_accumulation(self, steps: int):
        """SwitchNeRF.set_accumulation on both models: one window over the two, each with its own buffer."""
        for m in (self.nerf, self.bg):
            m.set_accumulation(steps)

    def grad_step(self, rgbs, rays, image_indices, n_samples, seg_tokens, perturb=1.0, fine_samples=0, bg_capacity=None, **kw):
        """Forward + loss + backward of both models: fills both gradients (zeroed first) and returns train_step's dict without
        "bg_nerf_rays_present".  In the padded form nothing here reads the host - the loss scale reaches the backward through the
        models' device scalar - so the launch sequence can be captured (graph.GraphedBackgroundStep)."""
        nerf, bg = self.nerf, self.bg
        nerf.grad.zero_()
        bg.grad.zero_()
        ctx = self.forward(rays, image_indices, n_samples, seg_tokens, perturb, fine_samples=fine_samples, bg_capacity=bg_capacity, **kw)
        fine = fine_samples > 0
        gate_loss = ctx["c"]["l_aux"].mean()
        if fine:
            gate_loss = (ctx["cf"]["l_aux"].mean() + gate_loss) / 2.0
        diff = ctx["rgb"] - rgbs
        photo = (diff * diff).mean()
        loss = photo + nerf.wt * gate_loss
        # fp16 (the reference's single GradScaler over both optimizers, runner.py:483, 679-690): one loss scale - the foreground model's
        # scaler - multiplies the loss gradient; both models unscale by it, and a non-finite gradient in either skips that model's step
        ls, ls_dev = 1.0, None
        if self.loss_scaler is not None:
            optim.sync_loss_scale((nerf, bg))             # (records the scale this backward uses: _found_inf divides by it)
            if bg_capacity is None:
                ls = float(self.loss_scaler.scale)
            else:
                ls_dev = nerf._ls_dev                     # the padded form reads the scale on the device (a replay follows it)
        d_rgb = diff * (2.0 * ls / diff.numel())
        if ls_dev is not None:
            d_rgb = d_rgb * ls_dev
        self.backward(ctx, d_rgb.contiguous(), ls * nerf.wt * (0.5 if fine else 1.0), ls * nerf.wt * 0.5, loss_scale_dev=ls_dev)
        psnr = -10.0 * torch.log10(photo)
        guard = {}
        if self.check_finite:                # ONE check for both models: the metrics of the blended image (a background ray's poison is in them)
            if bg_capacity is not None:
                raise NotImplementedError(self._GUARD_PADDED)
            guard["step_ok"] = nerf._finite_guard(torch.stack([photo, gate_loss, loss, psnr]).to(torch.float32), 3)
        return dict(**guard, loss=loss, photo_loss=photo, gate_loss=gate_loss, psnr=psnr, rgb=ctx["rgb"],
                    depth=ctx["depth"], depth_variance=ctx["depth_variance"].mean(), ctx=ctx)

    def read_counts(self, ctx):
        """Padded form: the ONE readback of (n_bg, n_out) - 8 bytes, behind everything enqueued so far - into ctx["Nb"] / ctx["n_out"],
        and the two checks the compact form makes inside forward.  Nothing to do for a compact context."""
        if ctx.get("C") is None:
            return
        if ctx["Nb"] is None:
            ctx["Nb"], ctx["n_out"] = (int(v) for v in ctx["counts_dev"].tolist())
        if ctx["n_out"] > 0:
            raise Exception(self._UNBOUNDED)
        if ctx["Nb"] > ctx["C"]:
            raise RuntimeError(f"BackgroundScene: n_bg = {ctx['Nb']} rays of this batch leave the foreground bound but bg_capacity = "
                               f"{ctx['C']}: the step was computed without the surplus rays and is not applied; raise bg_capacity "
                               f"(at most the batch's {ctx['N']} rays)")

    def apply_step(self, res, optimizer_step=True, grad_allreduce=None, refresh=None, advance=True, should_accumulate=None):
        """The tail both forms of the step share: gradient all-reduce, the shared loss scaler, both Adam steps under the bg_present
        rule (optim.apply_tail over the two models), the advance of the noise counter.  -> res with "bg_nerf_rays_present".
        Padded form: starts with the noise advance (advance=False: it was captured with the step) and the readback of (n_bg, n_out);
        a batch with cameras outside the bound or with n_bg > bg_capacity raises before any parameter of either model is touched
        (the noise counter has advanced: that step's draws are skipped).
        refresh: a replacement for BOTH models' refresh_compute_copies (the replay of their captured graph), run once.
        With gradient accumulation on (set_accumulation; the compact eager form only) -> res also holds "optimizer_stepped".  The window
        is the foreground model's.  An accumulating micro-step adds the background's gradient only when the batch had background rays
        (it is zero otherwise).  On the last micro-step the reference's rule is kept exactly: THAT batch's bg_nerf_rays_present decides
        whether the background optimizer steps (runner.py:683); if it does not, the window's accumulated background gradient is
        discarded, because zero_grad follows anyway (:689-690)."""
        nerf, bg = self.nerf, self.bg
        ctx = res["ctx"]
        padded = ctx.get("C") is not None
        if self.accum_steps > 1 and (refresh is not None or not advance or padded):
            raise NotImplementedError(self._ACCUM_PADDED)
        if self.check_finite and (refresh is not None or not advance or padded):
            raise NotImplementedError(self._GUARD_PADDED)
        if padded:
            if advance:
                self._noise_advance()
            self.read_counts(ctx)
        # the reference skips the background optimizer on batches without background rays (runner.py:683: `if key == 'bg_nerf'
        # and not bg_nerf_rays_present: continue`): no Adam step, no moment decay, no step-counter increment - in a SINGLE-process
        # run.  In a distributed run ('RANK' in os.environ) render_rays makes a dummy background forward on a rank without background
        # rays and reports bg_nerf_rays_present = True (rendering.py:162-194), so there the background Adam steps on EVERY iteration
        # (with a zero gradient when no rank had background rays: moments decay, step count grows).  Same rule here.
        import torch.distributed as dist
        distributed = grad_allreduce is not None or (dist.is_available() and dist.is_initialized())
        bg_present = True if distributed else ctx["Nb"] > 0
        # fp16: the reference holds ONE GradScaler over both optimizers (runner.py:483, 686-690).  GradScaler.step skips an optimizer on
        # ITS OWN non-finite gradient; GradScaler.update backs the shared scale off when EITHER optimizer found one (and only then
        # resets the growth tracker).  The foreground model's LossScaler is that shared scaler; the background's mirrors its scale.
        stepped = optim.apply_tail([nerf, bg], stepping=[nerf, bg] if bg_present else [nerf], zero_grad=() if ctx["Nb"] > 0 else (bg,),
                                   grad_allreduce=grad_allreduce, optimizer_step=optimizer_step, refresh=refresh,
                                   should_accumulate=should_accumulate)
        if not padded and advance:
            self._noise_advance()          # device noise: ONE advance per step, with or without background rays / a background Adam step
        res["bg_nerf_rays_present"] = bg_present
        if self.accum_steps > 1:
            res["optimizer_stepped"] = stepped
        return res
