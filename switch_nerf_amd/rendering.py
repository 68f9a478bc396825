"""Mirror of the reference's rendering.render_rays (/root/reference/switch_nerf/rendering.py:15-196): SwitchNeRF (or
DenseNeRF) model, optional dense background model behind the foreground bound (background.py), or a two-network cascade.Cascade
(hparams.use_cascade: _render_rays_cascade);
fine_samples = 0 (coarse pass composited) or fine_samples > 0 (hierarchical: coarse weights -> importance samples -> fine
pass -> merged compositing).

    results, bg_nerf_rays_present = render_rays(nerf, None, rays, image_indices, hparams, None, None,
                                                get_depth, get_depth_variance, get_bg_fg_rgb)

Result keys follow the reference: rgb_coarse, depth_coarse, depth_variance_coarse, gate_loss_coarse
([chunks * moe layers], rendering.py:388-390), moe_gates_coarse [N, S, 1, 1], sigma_coarse (hparams.return_sigma);
with fine_samples > 0: rgb_fine, depth_fine, depth_variance_fine, gate_loss_fine, gate_loss_coarse (and no rgb_coarse,
exactly like the reference's composite_rgb=False coarse pass, rendering.py:227).
Per-sample point outputs (hparams.return_pts / return_pts_rgb / return_pts_alpha / return_alpha, rendering.py:299, :413-417,
:443-452) for typ in coarse and fine: pts_{typ} [N,S,3], pts_rgb_{typ} [N,S,3], pts_alpha_{typ} [N,S] and alpha_{typ} ([N,S] for
the coarse pass, [N,S+F] in merged order for the fine pass); computed by swn_point_fields, off the compositing kernels.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

_POINT_FLAGS = ("return_pts", "return_pts_rgb", "return_pts_alpha", "return_alpha")


def _want_points(hparams) -> bool:
    return any(getattr(hparams, f, False) for f in _POINT_FLAGS)


def _point_keys(res, hparams, typ, rays, raw_pass, z, raw, last_delta=1e10, z_pts=None, order=None):
    """The point results of one pass: raw_pass [N*n,4] the pass's own network outputs, z [N,T] / raw [N*T,4] what it composites
    (merged with `order` for the fine pass, z_pts [N,n] its own depths then), last_delta of its last sample (float or per ray)."""
    from . import ops
    if not _want_points(hparams):
        return
    N = z.shape[0]
    n = (z if z_pts is None else z_pts).shape[1]
    want_pts, want_pa = bool(getattr(hparams, "return_pts", False)), bool(getattr(hparams, "return_pts_alpha", False))
    want_alpha = bool(getattr(hparams, "return_alpha", False))
    if want_pts or want_pa or want_alpha:
        pts, alpha, pa = ops.point_fields(rays.contiguous(), z.contiguous(), raw, last_delta, z_pts, order, want_pts, want_alpha, want_pa)
        if want_pts:
            res[f"pts_{typ}"] = pts
        if want_alpha:
            res[f"alpha_{typ}"] = alpha
        if want_pa:
            res[f"pts_alpha_{typ}"] = pa
    if getattr(hparams, "return_pts_rgb", False):
        res[f"pts_rgb_{typ}"] = raw_pass[:, :3].detach().view(N, n, 3)



def _device_noise(nerf, bg_nerf, hparams) -> bool:
    """hparams.device_noise_seed (absent / None: off): seeded device-side noise (SwitchNeRF.set_device_noise), switched on ONCE per model
    with the seed - the step counter then runs on.  An optional hparams.ray_base (the global index of this process's first ray) is
    honoured on every call; absent (or None), the model keeps the ray_base it has (parallel.shard_rays(..., model=nerf), set_ray_base).
    Returns whether the model draws its own noise.  A model whose noise is carried by a BackgroundScene (BackgroundScene.set_device_noise
    marks it) does not: the scene draws for both models and advances the one counter (_render_rays_bg)."""
    seed = getattr(hparams, "device_noise_seed", None)
    by_scene = getattr(getattr(nerf, "noise", None), "owner", None) is not None
    if seed is None and (by_scene or not getattr(nerf, "device_noise", False)):
        return False
    if by_scene:
        raise RuntimeError("device_noise_seed: this model's noise is carried by a BackgroundScene (BackgroundScene.set_device_noise); "
                           "switch that off (set_device_noise(None) / detach()) before seeding the model on its own")
    if bg_nerf is not None:
        raise NotImplementedError("device_noise_seed with a background model (bg_nerf) is not switched on through hparams: the scene "
                                  "owns the noise state of both models - call rendering.background_scene(nerf, bg_nerf, sphere_center, "
                                  "sphere_radius).set_device_noise(seed) (BackgroundScene.set_device_noise) and leave "
                                  "device_noise_seed unset")
    if not hasattr(nerf, "set_device_noise"):
        raise NotImplementedError("device_noise_seed: the model has no seeded device noise")
    if seed is None:                      # (switched on by the caller: SwitchNeRF.set_device_noise)
        return True
    ray_base = getattr(hparams, "ray_base", None)
    if not nerf.device_noise or nerf.noise.seed != int(seed):      # (the base outlives a switch-off: set_ray_base ahead of this)
        nerf.set_device_noise(int(seed), 0, nerf.noise.base if ray_base is None else int(ray_base))
    elif ray_base is not None:
        nerf.set_ray_base(int(ray_base))
    return True


def _check_affine(nerf, hparams):
    """hparams.affine_appearance (opts.py:55) must say what the model was built with (cfg["affine_appearance"]): a model with the other
    layer "2" width and parameter set is never used silently."""
    want, have = bool(getattr(hparams, "affine_appearance", False)), bool(getattr(nerf, "affine", False))
    if want != have:
        raise NotImplementedError(f"hparams.affine_appearance = {want} but the model was built with affine_appearance = {have}: "
                                  "build the model from a cfg with the same switch")


def _check_sh(nerf, bg_nerf, hparams):
    """hparams.sh_deg (opts.py:69) must say what the model was built with (cfg["sh_deg"]), the rule of _check_affine.  Only the dense
    NeRF carries the coefficients: NeRFMoE asserts a 4-channel sigma layer when pos_dir_dim == 0 (models/nerf_moe.py:186-189)."""
    want, have = getattr(hparams, "sh_deg", None), getattr(nerf, "sh_deg", None)
    if want is not None and not hasattr(nerf, "n_color"):
        raise NotImplementedError(f"hparams.sh_deg = {want}: spherical-harmonics colour is the dense NeRF's; NeRFMoE asserts a 4-channel "
                                  "sigma layer when pos_dir_dim == 0 (models/nerf_moe.py:186-189), so a SwitchNeRF cannot carry it")
    if want != have:
        raise NotImplementedError(f"hparams.sh_deg = {want} but the model was built with sh_deg = {have}: build the model from a cfg "
                                  "with the same sh_deg")
    if (have is not None and bg_nerf is not None) or getattr(bg_nerf, "sh_deg", None) is not None:
        raise NotImplementedError("sh_deg: a background model (bg_nerf) with spherical-harmonics colour is not built")


def _host_noise(hparams, training, N, rows, rows_fine, dev, device_noise, jitter=True):
    """The noise a render call draws from the framework generator -> perturb, std (of the sigma noise; 0.0: none), perturb_rand [N, S],
    sigma_noise [rows], sigma_noise_fine [rows_fine] (rows_fine None: no fine level), in the reference's order (rendering.py:582, :366).
    Evaluation draws nothing; nor does a call whose passes draw for themselves (device_noise: seeded device noise, captured graphs).
    jitter False: the callee draws the jitter itself (BackgroundScene.forward)."""
    perturb = hparams.perturb if training else 0
    use_noise = bool(getattr(hparams, "use_sigma_noise", False) and hparams.sigma_noise_std > 0 and training)
    pr = noise = noise_f = None
    if not device_noise:
        if jitter and perturb > 0:
            pr = torch.rand(N, hparams.coarse_samples, device=dev)
        if use_noise:
            noise = torch.randn(rows, device=dev) * hparams.sigma_noise_std
            if rows_fine is not None:
                noise_f = torch.randn(rows_fine, device=dev) * hparams.sigma_noise_std
    return perturb, float(hparams.sigma_noise_std) if use_noise else 0.0, pr, noise, noise_f


def _results(typ, rgb, gate_c, gate_f, depth, dvar, get_depth, get_depth_variance, take=lambda t: t):
    """The keys every branch returns for its top level `typ`; a gate loss of None has no key.  take: what a value goes through on its
    way out (a captured graph's outputs are cloned out of its static memory)."""
    res = {f"rgb_{typ}": take(rgb)}
    if gate_c is not None:
        res["gate_loss_coarse"] = take(gate_c)
    if gate_f is not None:
        res["gate_loss_fine"] = take(gate_f)
    if get_depth:
        res[f"depth_{typ}"] = take(depth)
    if get_depth_variance:
        res[f"depth_variance_{typ}"] = take(dvar)
    return res


def _gate_sigma_keys(res, hparams, c, cf, N, rows_c, rows_f, gates=True, sigma=True, take=lambda t: t):
    """moe_gates_{typ} [N, rows, 1, 1] (hparams.moe_return_gates) and sigma_{typ} [N, rows] (hparams.return_sigma) of the levels that ran
    (cf None: one level), from each level's "idx" and "raw"; gates / sigma False: the branch has no such key."""
    for typ, lvl, rows in (("coarse", c, rows_c), ("fine", cf, rows_f)):
        if lvl is None:
            continue
        if gates and getattr(hparams, "moe_return_gates", False):
            res[f"moe_gates_{typ}"] = lvl["idx"].long().view(N, rows, 1, 1)
        if sigma and getattr(hparams, "return_sigma", False):
            res[f"sigma_{typ}"] = take(lvl["raw"][:, 3].view(N, rows))


def render_rays(nerf, bg_nerf, rays: torch.Tensor, image_indices: Optional[torch.Tensor], hparams, sphere_center=None,
                sphere_radius=None, get_depth: bool = True, get_depth_variance: bool = True,
                get_bg_fg_rgb: bool = False) -> Tuple[Dict[str, torch.Tensor], bool]:
    is_mega = getattr(nerf, "is_mega_nerf", False) or getattr(bg_nerf, "is_mega_nerf", False)      # (mega.render_rays refuses use_cascade itself)
    if getattr(nerf, "is_cascade", False) or (getattr(hparams, "use_cascade", False) and not is_mega):      # the two-network cascade: cascade.py
        return _render_rays_cascade(nerf, bg_nerf, rays, image_indices, hparams, get_depth, get_depth_variance), False
    if getattr(nerf, "is_mega_nerf", False) or getattr(bg_nerf, "is_mega_nerf", False):      # the spatial-cell model (--container_path): mega.py
        from . import mega
        return mega.render_rays(nerf, bg_nerf, rays, image_indices, hparams, sphere_center, sphere_radius, get_depth,
                                get_depth_variance, get_bg_fg_rgb)
    _check_affine(nerf, hparams)
    _check_sh(nerf, bg_nerf, hparams)
    F = int(getattr(hparams, "fine_samples", 0))
    N = rays.shape[0]
    S = hparams.coarse_samples
    dn = _device_noise(nerf, bg_nerf, hparams) and nerf.training
    if bg_nerf is not None:
        return _render_rays_bg(nerf, bg_nerf, rays, image_indices, hparams, sphere_center, sphere_radius, get_depth,
                               get_depth_variance, get_bg_fg_rgb)
    P = N * S
    chunk = min(hparams.model_chunk_size, P)
    # (a ragged last model chunk - P % chunk != 0 - is routed on its own like the reference's loop, rendering.py:354-383, in
    #  evaluation and in training)
    training = nerf.training
    under_autograd = training and torch.is_grad_enabled() and hasattr(nerf, "flat_param") and getattr(nerf, "hash", None) is None
    # forward / backward replayed from captured graphs (graph.GraphedRenderTrain): jitter and sigma noise are drawn inside them
    graphed = under_autograd and getattr(nerf, "graph_train", False) and getattr(nerf, "ep", None) is None
    perturb, std, pr, noise, noise_f = _host_noise(hparams, training, N, P, N * F if F > 0 else None, rays.device, dn or graphed)
    if image_indices is None:
        image_indices = torch.zeros(N, dtype=torch.long, device=rays.device)
    typ = "fine" if F > 0 else "coarse"
    if under_autograd:
        # training under autograd (the reference's Runner loop: loss.backward() + torch optimizer, runner.py:679-693): one autograd
        # node over the HIP forward; its backward runs the HIP backward and fills nerf.flat_param.grad (autograd.py).  Where the passes
        # draw the noise themselves (captured graphs, seeded device noise) the std stands in for the noise tensor
        from .autograd import RenderRaysFunction
        rgb, gl_c, gl_f, depth, dvar = RenderRaysFunction.apply(nerf.flat_param, nerf, rays.contiguous(), image_indices, S, F, chunk,
                                                                float(perturb), "graph" if graphed else pr,
                                                                std if (dn or graphed) else noise, noise_f)
        c, cf, out = nerf._last_ctx
        res = _results(typ, rgb, gl_c, gl_f if F > 0 else None, depth, dvar, get_depth, get_depth_variance)
    elif not training and getattr(nerf, "graph_eval", False) and getattr(nerf, "ep", None) is None and not _want_points(hparams):
        return _render_rays_graphed(nerf, rays, image_indices, hparams, N, S, F, chunk, get_depth, get_depth_variance), False
    else:          # (seeded device noise: the passes draw jitter / sigma noise / fine u themselves, then the step advances)
        c, cf, out = nerf.render_forward(rays.contiguous(), image_indices, S, F, chunk, float(perturb), pr, None, noise, noise_f,
                                         training=training, no_batch=nerf.moe_no_batch, sigma_noise_std=std if dn else 0.0)
        if dn:
            nerf._noise_advance()
        res = _results(typ, out["rgb"], c["l_aux"], cf["l_aux"] if cf is not None else None, out["depth"], out["depth_variance"],
                       get_depth, get_depth_variance)
    _gate_sigma_keys(res, hparams, c, cf, N, S, F)
    _point_keys(res, hparams, "coarse", rays, c["raw"], c["z"], c["raw"])
    if F > 0:
        _point_keys(res, hparams, "fine", rays, cf["raw"], out["z"], out["raw"], z_pts=out["z_fine"], order=out["order"])
    return res, False


def _render_rays_cascade(nerf, bg_nerf, rays, image_indices, hparams, get_depth, get_depth_variance):
    """hparams.use_cascade (rendering.py:227-268, :333-342): nerf is a cascade.Cascade.  Result keys are the reference's: rgb_coarse,
    gate_loss_coarse and, with fine_samples > 0, rgb_fine, depth_fine, depth_variance_fine, gate_loss_fine (sigma_fine in the [N, S + F]
    shape); with fine_samples == 0 the coarse keys only, depth_coarse / depth_variance_coarse among them."""
    if not getattr(nerf, "is_cascade", False):
        raise NotImplementedError("hparams.use_cascade needs the two-network model: wrap the coarse and the fine model in "
                                  "switch_nerf_amd.cascade.Cascade(coarse, fine)")
    if not getattr(hparams, "use_cascade", False):
        raise NotImplementedError("the model is a Cascade but hparams.use_cascade is off: a Cascade renders with use_cascade only")
    if bg_nerf is not None:
        raise NotImplementedError("Cascade: a background model (bg_nerf) is not built for the two-network cascade")
    if _want_points(hparams):
        raise NotImplementedError("Cascade: the per-sample point outputs (return_pts*) are not built for the two-network cascade")
    if getattr(hparams, "device_noise_seed", None) is not None:
        raise NotImplementedError("Cascade: seeded device noise (device_noise_seed) is not built for the two-network cascade")
    for h in nerf.halves():
        _check_affine(h, hparams)
        _check_sh(h, None, hparams)
    N, S, F = rays.shape[0], hparams.coarse_samples, int(getattr(hparams, "fine_samples", 0))
    training = nerf.training
    chunk = min(hparams.model_chunk_size, N * S)
    perturb, _, pr, noise, noise_f = _host_noise(hparams, training, N, N * S, N * (S + F) if F > 0 else None, rays.device, False)
    if image_indices is None:
        image_indices = torch.zeros(N, dtype=torch.long, device=rays.device)
    rays = rays.contiguous()
    nerf._check_runtime()
    if training and torch.is_grad_enabled() and any(getattr(h, "hash", None) is not None for h in nerf.halves()):
        raise NotImplementedError("Cascade: training hash-grid halves under autograd is not built (the autograd bridge carries no table "
                                  "gradient); use Cascade.train_step, or render under torch.no_grad()")
    if F > 0 and nerf.fine is None:
        raise ValueError("Cascade: fine_samples > 0 needs a fine half")
    if training and torch.is_grad_enabled():
        # training under autograd (autograd.py): one node over both levels' HIP forward; its backward fills each half's flat_param.grad
        from .autograd import CascadeRenderFunction, RenderRaysFunction
        if F > 0:
            rgb_f, rgb_c, gl_c, gl_f, depth, dvar = CascadeRenderFunction.apply(nerf.coarse.flat_param, nerf.fine.flat_param, nerf, rays,
                                                                                image_indices, S, F, chunk, float(perturb), pr, noise, noise_f)
            c, cf = nerf._last_ctx
        else:
            rgb_c, gl_c, _, depth, dvar = RenderRaysFunction.apply(nerf.coarse.flat_param, nerf.coarse, rays, image_indices, S, 0, chunk,
                                                                   float(perturb), pr, noise, None)
            c, cf, rgb_f, gl_f = nerf.coarse._last_ctx[0], None, rgb_c, None
    else:
        c, cf = nerf.forward_cascade(rays, image_indices, S, F, chunk, float(perturb), pr, None, noise, noise_f,
                                     no_batch=nerf.moe_no_batch, training=training)
        rgb_c, gl_c = c["rgb"], c["l_aux"]
        top = cf if cf is not None else c
        rgb_f, gl_f, depth, dvar = top["rgb"], top["l_aux"], top["depth"], top["depth_variance"]
    res = _results("fine" if F > 0 else "coarse", rgb_f, gl_c, gl_f if F > 0 else None, depth, dvar, get_depth, get_depth_variance)
    if F > 0:
        res["rgb_coarse"] = rgb_c
    _gate_sigma_keys(res, hparams, c, cf, N, S, S + F, gates=False)
    return res


def _render_rays_graphed(nerf, rays, image_indices, hparams, N, S, F, chunk, get_depth, get_depth_variance, fill=None):
    """Evaluation with `nerf.graph_eval = True`: the forward of this batch shape is captured once (graph.GraphedRender, cached on the
    model per (rays, samples, fine samples, chunk, no_batch)) and replayed - Runner.render_image's pixel-batch loop
    (runner.py:2835-2885) is ~60 launches per call otherwise.  Results are cloned out of the graph's static memory.
    fill (render_image's hook; rays and image_indices are None then): fill(rays_buffer, index_buffer) writes the batch straight into
    the graph's static inputs, so nothing is copied in."""
    from .graph import GraphedRender, cached_graph
    cache = nerf.__dict__.setdefault("_render_graphs", {})
    key = (N, S, F, int(chunk), bool(nerf.moe_no_batch), nerf.dtype)
    nerf._sync_compute_copies()
    if fill is not None and key not in cache:      # the capture wants a batch to warm up on
        rays = torch.empty(N, 8, dtype=torch.float32, device=nerf.dev)
        image_indices = torch.empty(N, dtype=torch.long, device=nerf.dev)
        fill(rays, image_indices)
    g = cached_graph(cache, key, lambda: GraphedRender(nerf, rays.contiguous(), image_indices, S, chunk, F, nerf.moe_no_batch))
    if fill is None:
        o = g(rays, image_indices)
    else:
        fill(g.rays, g.idx)
        o = g()
    res = _results("fine" if F > 0 else "coarse", o["rgb"], o["l_aux_coarse"], o.get("l_aux_fine"), o["depth"], o["depth_variance"],
                   get_depth, get_depth_variance, take=torch.clone)
    _gate_sigma_keys(res, hparams, dict(idx=o["idx_coarse"], raw=o["raw_coarse"]),
                     dict(idx=o["idx_fine"], raw=o["raw_fine"]) if F > 0 else None, N, S, F, take=torch.clone)
    return res


def background_scene(nerf, bg_nerf, sphere_center=None, sphere_radius=None):
    """The BackgroundScene render_rays uses for (nerf, bg_nerf): built on first use and cached on the foreground model.  Seeded device
    noise for a scene with a background model is switched on here: background_scene(...).set_device_noise(seed) - a training
    render_rays then passes no framework-drawn noise and advances the scene's step counter after its forward."""
    from .background import BackgroundScene
    scene = getattr(nerf, "_bg_scene", None)
    if scene is None or scene.bg is not bg_nerf:
        if scene is not None:
            scene.set_device_noise(None)       # (the replaced scene hands the foreground model its own noise state back)
        scene = nerf._bg_scene = BackgroundScene(nerf, bg_nerf, sphere_center, sphere_radius)
    scene.center, scene.radius = sphere_center, sphere_radius
    return scene


def _render_rays_bg(nerf, bg_nerf, rays, image_indices, hparams, sphere_center, sphere_radius, get_depth, get_depth_variance,
                    get_bg_fg_rgb):
    """The bg_nerf branch (rendering.py:32-159) through background.BackgroundScene."""
    N, S, F = rays.shape[0], hparams.coarse_samples, int(getattr(hparams, "fine_samples", 0))
    if image_indices is None:
        image_indices = torch.zeros(N, dtype=torch.long, device=rays.device)
    scene = background_scene(nerf, bg_nerf, sphere_center, sphere_radius)
    dn = scene.device_noise and nerf.training      # seeded device noise: the scene draws what is not supplied (std = the sigma noise's)
    perturb, std, _, noise, noise_f = _host_noise(hparams, nerf.training, N, N * S, N * F if F > 0 else None, rays.device, dn, jitter=False)
    kw = {}
    if noise is not None:           # rendering.py:366: randn per evaluated chunk, for either model
        kw = dict(sigma_noise=noise, sigma_noise_bg="randn", sigma_noise_bg_fine="randn", sigma_noise_fine=noise_f)
    cap = getattr(hparams, "bg_capacity", None)     # the padded form of the background rows (background.py), when the recipe asks for it
    if cap is not None:
        kw["bg_capacity"] = max(1, min(int(cap), N))
    ctx = scene.forward(rays.contiguous(), image_indices, S, min(hparams.model_chunk_size, N * S), float(perturb), fine_samples=F,
                        no_batch=nerf.moe_no_batch, noise_std=std, training=nerf.training, **kw)
    if dn:
        scene._noise_advance()
    scene.read_counts(ctx)                          # (padded form: the one readback and the checks the compact form made inside forward)
    typ = "fine" if F > 0 else "coarse"
    res = _results(typ, ctx["rgb"], ctx["c"]["l_aux"], ctx["cf"]["l_aux"] if F > 0 else None, ctx["depth"], ctx["depth_variance"],
                   get_depth, get_depth_variance)
    if get_bg_fg_rgb:                                                    # :111-112, :124-125
        res[f"fg_rgb_{typ}"] = ctx["fg_rgb"]
        res[f"bg_rgb_{typ}"] = ctx["rgb"] - ctx["fg_rgb"]
        res[f"fg_depth_{typ}"] = ctx["fg_depth"]
        res[f"bg_depth_{typ}"] = ctx["depth"] - ctx["fg_depth"]
    _gate_sigma_keys(res, hparams, ctx["c"], ctx.get("cf"), N, S, F, sigma=False)
    if _want_points(hparams):                                            # foreground keys only, like the reference
        c = ctx["c"]
        if F > 0:
            # the coarse pass was composited (for its weights) with the 1e10 last delta; its alpha takes the reference's
            # fg_far - max(z_coarse) on rays with a background (rendering.py:214-220)
            ld_c = torch.where(ctx["has_bg"] > 0, ctx["fg_far"] - c["z"].max(dim=-1)[0], torch.full_like(ctx["fg_far"], 1e10))
            _point_keys(res, hparams, "coarse", rays, c["raw"], c["z"], c["raw"], ld_c.contiguous())
            _point_keys(res, hparams, "fine", rays, ctx["cf"]["raw"], ctx["z"], ctx["raw"], ctx["last_delta"], z_pts=ctx["z_fine"],
                        order=ctx["order"])
        else:
            _point_keys(res, hparams, "coarse", rays, c["raw"], ctx["z"], ctx["raw"], ctx["last_delta"])
    return res, ctx["Nb"] > 0


def render_rays_mip(nerf, rays: torch.Tensor, radii: torch.Tensor, image_indices: Optional[torch.Tensor], hparams,
                    get_depth: bool = True, get_depth_variance: bool = True) -> Tuple[Dict[str, torch.Tensor], bool]:
    """Mirror of rendering_mip.render_rays (/root/reference/switch_nerf/rendering_mip.py:133-172) for MipNeRFMoE-style models:
    results carry rgb_coarse, gate_loss_coarse and, with fine_samples > 0, rgb_fine, depth_fine, depth_variance_fine,
    gate_loss_fine (the coarse level reports depth only when it is the last one, :207-208)."""
    _check_affine(nerf, hparams)
    N = rays.shape[0]
    S, F = hparams.coarse_samples, int(getattr(hparams, "fine_samples", 0))
    dn = _device_noise(nerf, None, hparams) and nerf.training      # seeded device noise: forward_mip draws what is not supplied
    perturb, std, pr, noise, noise_f = _host_noise(hparams, nerf.training, N, N * (S - 1), N * max(F - 1, 0) if F > 0 else None,
                                                   rays.device, dn)
    chunk = hparams.model_chunk_size
    if image_indices is None:
        image_indices = torch.zeros(N, dtype=torch.long, device=rays.device)
    c, cf = nerf.forward_mip(rays.contiguous(), radii, image_indices, S, F, chunk, float(perturb), pr, None, noise, noise_f,
                             no_batch=nerf.moe_no_batch, rgb_padding=float(getattr(hparams, "rgb_padding", 0.001) or 0.0),
                             resample_padding=float(getattr(hparams, "weights_resample_padding", 0.01)), training=nerf.training,
                             fine_randomized=bool(hparams.perturb),      # rendering_mip.py:227: randomized=hparams.perturb, also in eval
                             sigma_noise_std=std if dn else 0.0)
    if dn:
        nerf._noise_advance()
    top, typ = (c, "coarse") if cf is None else (cf, "fine")
    res = _results(typ, top["rgb"], c["l_aux"], None if cf is None else cf["l_aux"], top["depth"], top["depth_variance"], get_depth,
                   get_depth_variance)
    if cf is not None:
        res["rgb_coarse"] = c["rgb"]
    _gate_sigma_keys(res, hparams, c, cf, N, S - 1, F - 1, sigma=False)
    return res, False


def render_image_rays(nerf, bg_nerf, rays: torch.Tensor, image_index, hparams, sphere_center=None, sphere_radius=None,
                      radii: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """The pixel-batch loop of Runner.render_image / render_image_blocknerf (/root/reference/switch_nerf/runner.py:2835-2885,
    :2887-2950) over rays that are already built ([R, 8], R = H * W; ray construction from camera metadata is dataset code):
    batches of hparams.image_pixel_batch_size rays through render_rays (or render_rays_mip when radii are given) with
    get_depth=True, get_depth_variance=False, get_bg_fg_rgb=True, results concatenated on the host like the reference.
    The last batch of an image - and the last model chunk inside a batch - may be ragged."""
    R = rays.shape[0]
    rays = rays.reshape(-1, 8)
    idx = None
    if getattr(hparams, "appearance_dim", 1) > 0:
        idx = image_index if torch.is_tensor(image_index) and image_index.numel() == R else \
            torch.full((R,), int(image_index), dtype=torch.long, device=rays.device)
    results: Dict[str, list] = {}
    step = int(hparams.image_pixel_batch_size)
    for i in range(0, R, step):
        r = rays[i:i + step].contiguous()
        ii = None if idx is None else idx[i:i + step].contiguous()
        if radii is not None:
            batch, _ = render_rays_mip(nerf, r, radii.reshape(-1, 1)[i:i + step].contiguous(), ii, hparams, True, False)
        else:
            batch, _ = render_rays(nerf, bg_nerf, r, ii, hparams, sphere_center, sphere_radius, True, False, True)
        for k, v in batch.items():
            results.setdefault(k, []).append(v.cpu())
    return {k: torch.cat(v) for k, v in results.items()}


def _takes_graph_eval(nerf, bg_nerf, hparams) -> bool:
    """Whether render_rays, in evaluation, ends in its graph_eval branch for these models (its own dispatch, in its order)."""
    if getattr(nerf, "is_cascade", False) or getattr(hparams, "use_cascade", False):
        return False
    if getattr(nerf, "is_mega_nerf", False) or getattr(bg_nerf, "is_mega_nerf", False) or bg_nerf is not None:
        return False
    return bool(getattr(nerf, "graph_eval", False)) and getattr(nerf, "ep", None) is None and not _want_points(hparams)


def _graphed_image_batch(nerf, hparams, n, fill):
    """render_rays' steps down to its graph_eval branch (get_depth, no depth variance) for a batch of n rays that `fill` writes into the
    graph's static inputs (_render_rays_graphed)."""
    _check_affine(nerf, hparams)
    _check_sh(nerf, None, hparams)
    _device_noise(nerf, None, hparams)
    S, F = hparams.coarse_samples, int(getattr(hparams, "fine_samples", 0))
    return _render_rays_graphed(nerf, None, None, hparams, n, S, F, min(hparams.model_chunk_size, n * S), True, False, fill=fill)


def _model_device(nerf):
    dev = getattr(nerf, "dev", None)
    return dev if dev is not None else nerf.halves()[0].dev


def render_image(nerf, bg_nerf, camera, hparams, near: float, far: float, ray_altitude_range=None, sphere_center=None,
                 sphere_radius=None) -> Tuple[Dict[str, torch.Tensor], torch.Tensor]:
    """Runner.render_image (/root/reference/switch_nerf/runner.py:2835-2885) from a rays.Camera: the image is walked in batches of
    hparams.image_pixel_batch_size pixels (a ragged last batch, no padding), each batch's rays come from ONE launch (rays.camera_rays,
    hparams.center_pixels, default on) and go through render_rays(..., get_depth=True, get_depth_variance=False, get_bg_fg_rgb=True).
    -> (results, rays [H * W, 8]), everything on the device: a per-ray value is written into its slice of a [H * W, ...] tensor
    allocated when its key first appears, a 0-dim value is stacked to [n_batches], the gate losses ([chunks * moe layers] per batch) are
    concatenated in batch order as the reference concatenates them.  Image indices are an int64 tensor of camera.image_index, or None
    with hparams.appearance_dim == 0.  Every model render_rays accepts in evaluation works and every refusal is render_rays' own.
    With nerf.graph_eval = True on the plain path the rays (and indices) are generated directly into the cached GraphedRender's static
    inputs and the graph is replayed; the last batch has its own cached graph.  The rays are fp32 also where the reference builds them
    inside autocast."""
    from . import rays as raygen
    for m, who in ((nerf, "nerf"), (bg_nerf, "bg_nerf")):
        if m is not None and getattr(m, "training", False):
            raise RuntimeError(f"render_image: {who} is in training mode; validation images are rendered in evaluation (call .eval())")
    dev = _model_device(nerf)
    P = camera.W * camera.H
    center = bool(getattr(hparams, "center_pixels", True))
    spans = raygen.batches(P, hparams.image_pixel_batch_size)
    with_index = getattr(hparams, "appearance_dim", 1) > 0
    gen = lambda begin, n, out, idx=None: raygen.camera_rays(camera, near, far, ray_altitude_range, center, begin, n, out, idx)
    graphed = _takes_graph_eval(nerf, bg_nerf, hparams)
    if graphed:
        rays = gen(0, P, torch.empty(P, 8, dtype=torch.float32, device=dev))
    else:
        rays = torch.empty(P, 8, dtype=torch.float32, device=dev)
        indices = torch.full((P,), camera.image_index, dtype=torch.long, device=dev) if with_index else None
    results: Dict[str, torch.Tensor] = {}
    loose: Dict[str, list] = {}
    with torch.no_grad():
        for begin, n in spans:
            if graphed:
                def fill(rays_buf, idx_buf, begin=begin, n=n):
                    own = with_index and idx_buf.dtype == torch.long      # (the fused launch fills an int64 index buffer)
                    gen(begin, n, rays_buf, idx_buf if own else None)
                    if not own:
                        idx_buf.fill_(camera.image_index if with_index else 0)
                batch = _graphed_image_batch(nerf, hparams, n, fill)
            else:
                r = gen(begin, n, rays[begin:begin + n])
                batch, _ = render_rays(nerf, bg_nerf, r, indices[begin:begin + n] if with_index else None, hparams, sphere_center,
                                       sphere_radius, True, False, True)
            for k, v in batch.items():
                if v.dim() >= 1 and v.shape[0] == n and not k.startswith("gate_loss"):
                    if k not in results:
                        results[k] = torch.empty(P, *v.shape[1:], dtype=v.dtype, device=v.device)
                    results[k][begin:begin + n] = v
                else:
                    loose.setdefault(k, []).append(v)
    for k, v in loose.items():
        results[k] = torch.stack(v) if v[0].dim() == 0 else torch.cat(v)
    return results, rays


def validate_image(nerf, bg_nerf, camera, target, hparams, near: float, far: float, ray_altitude_range=None, sphere_center=None,
                   sphere_radius=None, valid_mask=None):
    """One validation image from a camera, scored where it lies: render_image, the top level's rgb as [H, W, 3], metrics.image_metrics
    against target [H, W, 3] (valid_mask [H, W]: the cell's mask) -> (the metrics as device tensors, the image).  No host read."""
    from . import metrics
    results, _ = render_image(nerf, bg_nerf, camera, hparams, near, far, ray_altitude_range, sphere_center, sphere_radius)
    typ = "fine" if "rgb_fine" in results else "coarse"
    image = results[f"rgb_{typ}"].view(camera.H, camera.W, 3)
    return metrics.image_metrics(image, target, valid_mask=valid_mask), image


def _render_image_nerf_loop(who, nerf, camera, hparams, gen, render):
    """The walk Runner.render_image_nerf / render_image_nerf_mip share: batches of hparams.image_pixel_batch_size pixels (a ragged last
    batch), gen(begin, n) makes the batch's rays on the device, render(...) is the batch's render_rays / render_rays_mip call; the
    results are assembled on the device as render_image assembles them."""
    from . import nerf_rays
    if getattr(nerf, "training", False):
        raise RuntimeError(f"{who}: nerf is in training mode; validation images are rendered in evaluation (call .eval())")
    P = camera.W * camera.H
    results: Dict[str, torch.Tensor] = {}
    loose: Dict[str, list] = {}
    with torch.no_grad():
        for begin, n in nerf_rays.batches(P, hparams.image_pixel_batch_size):
            batch, _ = render(*gen(begin, n))
            for k, v in batch.items():
                if v.dim() >= 1 and v.shape[0] == n and not k.startswith("gate_loss"):
                    if k not in results:
                        results[k] = torch.empty(P, *v.shape[1:], dtype=v.dtype, device=v.device)
                    results[k][begin:begin + n] = v
                else:
                    loose.setdefault(k, []).append(v)
    for k, v in loose.items():
        results[k] = torch.stack(v) if v[0].dim() == 0 else torch.cat(v)
    return results


def render_image_nerf(nerf, camera, hparams, near: float, far: float, mode: str = "normalized", focal: Optional[float] = None,
                      near_ndc: float = 1.0) -> Dict[str, torch.Tensor]:
    """Runner.render_image_nerf (runner.py:2943-2974) from a nerf_rays.PinholeCamera: the image is walked in
    batches of hparams.image_pixel_batch_size pixels, each batch's rays come from ONE launch (nerf_rays.camera_rays in `mode`:
    "normalized" for Blender / LLFF no_ndc, "ndc" for forward-facing LLFF, "raw") and go through render_rays(nerf, None, rays,
    image_indices=None, ..., get_depth=True, get_depth_variance=False, get_bg_fg_rgb=False).  -> the reference's result keys as device
    tensors: a per-ray value in its slice of a [H * W, ...] tensor, the gate losses concatenated in batch order."""
    from . import nerf_rays
    dev = _model_device(nerf) if not getattr(nerf, "training", False) else None
    gen = lambda begin, n: (nerf_rays.camera_rays(camera, mode, near, far, focal, near_ndc, begin, n, device=dev),)
    render = lambda r: render_rays(nerf, None, r, None, hparams, None, None, True, False, False)
    return _render_image_nerf_loop("render_image_nerf", nerf, camera, hparams, gen, render)


def render_image_nerf_mip(nerf, camera, hparams, scene_scaling_factor: float, scene_origin, ray_nearfar: str) -> Dict[str, torch.Tensor]:
    """Runner.render_image_nerf_mip (runner.py:2977-3008) from a nerf_rays.PinholeCamera: each batch's rays
    and mip radii come from ONE launch (nerf_rays.bungee_rays: per-ray near / far of the "sphere" or "flat" form) and go through
    render_rays_mip(nerf, rays, radii, image_indices=None, hparams, get_depth=True, get_depth_variance=False)."""
    from . import nerf_rays
    dev = _model_device(nerf) if not getattr(nerf, "training", False) else None
    gen = lambda begin, n: nerf_rays.bungee_rays(camera, scene_scaling_factor, scene_origin, ray_nearfar, begin, n, device=dev)
    render = lambda r, radii: render_rays_mip(nerf, r, radii, None, hparams, True, False)
    return _render_image_nerf_loop("render_image_nerf_mip", nerf, camera, hparams, gen, render)
