"""torch.autograd bridge: lets the reference's training loop drive the HIP path unchanged.

Runner.train does, per step (runner.py:604-693):
    metrics = self._training_step(rgbs, rays, image_indices)          # calls render_rays(nerf, ...)
    scaler.scale(metrics['loss']).backward()
    scaler.step(optimizer); scaler.update(); scheduler.step()          # torch.optim.Adam over nerf.parameters(), ExponentialLR
so render_rays must return tensors with a grad_fn and `nerf.parameters()` must be real leaf Parameters that receive `.grad`.
Here the model's whole parameter set is ONE leaf Parameter (`nerf.flat_param`, sharing storage with the flat fp32 master buffer
the kernels read - Adam is elementwise, one flat tensor is equivalent to the reference's per-module tensors), and the rendering of a
ray batch is one autograd node whose backward runs the HIP backward kernels and hands the flat gradient to autograd (which
accumulates it into `.grad`: gradient accumulation over micro-batches, loss scaling and torch's finite checks all work as usual).
"""
from __future__ import annotations

import torch


def render_outputs(c, cf, out):
    """What a render pass (SwitchNeRF.render_forward) hands to autograd: rgb, both gate losses (the fine one empty for one level), depth,
    depth variance."""
    gl_f = cf["l_aux"] if cf is not None else torch.zeros(0, device=out["rgb"].device)
    return out["rgb"], c["l_aux"], gl_f, out["depth"], out["depth_variance"]


class RenderRaysFunction(torch.autograd.Function):
    """(flat_param, nerf, rays, image_indices, S, F, chunk, perturb, perturb_rand, sigma_noise, sigma_noise_fine)
    -> (rgb [N,3], gate_loss_coarse [n_seg], gate_loss_fine [n_seg_f] or empty, depth [N], depth_variance [N]).
    perturb_rand = "graph" (with sigma_noise = the noise std): the forward and the backward are replayed from the captured graphs of
    graph.GraphedRenderTrain (`nerf.graph_train = True`), which draw the jitter and the noise on the device themselves.
    sigma_noise = a float with perturb_rand = None (the model's device noise on): the passes draw jitter and noise from the seeded
    generator, sigma noise with that std; the forward ends in the step counter's advance."""

    @staticmethod
    def forward(ctx, flat_param, nerf, rays, image_indices, S, F, chunk, perturb, perturb_rand, sigma_noise, sigma_noise_fine):
        nerf._sync_compute_copies()
        ctx.nerf = nerf
        ctx.graph = None
        std = 0.0
        if isinstance(sigma_noise, float) and perturb_rand is None:      # the model's seeded device noise is on (set_device_noise): the std
            if not getattr(nerf, "device_noise", False):                 # of the sigma noise the passes draw themselves
                raise ValueError("RenderRaysFunction: sigma_noise given as a std (float) needs the model's device noise on "
                                 "(set_device_noise); pass a noise tensor or None otherwise")
            std, sigma_noise = sigma_noise, None
        if isinstance(perturb_rand, str) and perturb_rand == "graph":
            from .graph import GraphedRenderTrain, cached_graph
            cache = nerf.__dict__.setdefault("_train_graphs", {})
            dn = nerf.noise                                  # (a captured graph holds the seed and ray_base it was captured with)
            key = (rays.shape[0], S, F, int(chunk), float(perturb), float(sigma_noise or 0.0), bool(nerf.moe_no_batch), nerf.dtype,
                   dn.seed, dn.base if dn.on else None)
            g = cached_graph(cache, key, lambda: GraphedRenderTrain(nerf, rays, image_indices, S, F, chunk, float(perturb),
                                                                    float(sigma_noise or 0.0)))
            state, outs = g.forward(rays, image_indices)
            ctx.graph, ctx.state, ctx.generation = g, state, g.generation
            res = (outs[0].clone(), outs[1].clone(), outs[2].clone(), outs[3].clone(), outs[4].clone())
        else:
            ctx.state = nerf.render_forward(rays, image_indices, S, F, chunk, perturb, perturb_rand, None, sigma_noise, sigma_noise_fine,
                                            training=True, no_batch=nerf.moe_no_batch, sigma_noise_std=std)
            nerf._noise_advance()
            res = render_outputs(*ctx.state)
        ctx.mark_non_differentiable(res[3], res[4])
        nerf._last_ctx = ctx.state
        return res

    @staticmethod
    def backward(ctx, d_rgb, d_laux_c, d_laux_f, _d_depth, _d_var):
        nerf = ctx.nerf
        if ctx.graph is not None:
            # every replay of the forward graph returns the SAME state object (static buffers): the replay counter tells whether the
            # buffers still hold this node's activations
            if ctx.graph.generation != ctx.generation or nerf._last_ctx is not ctx.state:
                raise RuntimeError("graph_train: backward() must follow the forward it belongs to (the captured graphs share one set of "
                                   "static activation buffers per batch shape)")
            g = ctx.graph.backward(d_rgb.to(torch.float32), d_laux_c.to(torch.float32), d_laux_f.to(torch.float32))
            ctx.state = None
            return (g.clone(),) + (None,) * 10
        nerf.grad.zero_()
        f32 = lambda t: t.to(torch.float32).contiguous()
        nerf.render_backward(*ctx.state, f32(d_rgb), f32(d_laux_c), f32(d_laux_f))
        ctx.state = None
        return (nerf.grad.clone(),) + (None,) * 10


class CascadeRenderFunction(torch.autograd.Function):
    """The two-network cascade (cascade.Cascade) under autograd, over the two flat_param leaves:
    (flat_coarse, flat_fine, cascade, rays, image_indices, S, F, chunk, perturb, perturb_rand, sigma_noise, sigma_noise_fine)
    -> (rgb_fine [N,3], rgb_coarse [N,3], gate_loss_coarse [n_seg], gate_loss_fine [n_seg_f], depth_fine [N], depth_variance_fine [N]).
    The backward runs each level's HIP backward into its own half's gradient buffer and hands each leaf its flat gradient, so the
    reference's Runner loop (loss.backward() + torch.optim.Adam over both leaves) drives the cascade.  No gradient crosses the levels:
    the fine depths come from the detached coarse weights (rendering.py:240)."""

    @staticmethod
    def forward(ctx, flat_coarse, flat_fine, cascade, rays, image_indices, S, F, chunk, perturb, perturb_rand, sigma_noise, sigma_noise_fine):
        c, cf = cascade.forward_cascade(rays, image_indices, S, F, chunk, perturb, perturb_rand, None, sigma_noise, sigma_noise_fine,
                                        no_batch=cascade.moe_no_batch, training=True)
        ctx.cascade, ctx.state = cascade, (c, cf)
        cascade._last_ctx = ctx.state
        res = (cf["rgb"], c["rgb"], c["l_aux"], cf["l_aux"], cf["depth"], cf["depth_variance"])
        ctx.mark_non_differentiable(res[4], res[5])
        return res

    @staticmethod
    def backward(ctx, d_rgb_f, d_rgb_c, d_laux_c, d_laux_f, _d_depth, _d_var):
        c, cf = ctx.state
        f32 = lambda t: t.to(torch.float32).contiguous()
        grads = []
        for half, lvl, d_rgb, d_laux in ((ctx.cascade.coarse, c, d_rgb_c, d_laux_c), (ctx.cascade.fine, cf, d_rgb_f, d_laux_f)):
            half.grad.zero_()
            half.backward(lvl, f32(d_rgb), f32(d_laux))
            grads.append(half.grad.clone())
        ctx.state = None
        return (grads[0], grads[1]) + (None,) * 10
