"""hipGraph capture of the training step's launch sequence.

A train step of the hot path is ~150 kernel launches.  At the reference's multi-GPU batch (8192 rays split over 8 ranks = 1024 rays
per GPU, runner.py:573-575) they hold ~2.5 ms of GPU work while the Python host needs ~3.7 ms to enqueue them: the step is
launch-bound.  Nothing in forward + loss + backward depends on host state that changes between steps (shapes, capacities and
buffer addresses are static; the random draws are device-side), so the sequence is captured once into a hipGraph and replayed:
one host call per step, kernels back to back.  The gradient all-reduce (RCCL) and Adam (its bias correction takes the step count
as a launch argument) stay outside the graph; the refresh of the compute copies of the weights is a second small graph.
"""
from __future__ import annotations

import torch

MAX_CACHED_GRAPHS = 8


def _refuse_sh(model, who: str):
    """Graph capture of a spherical-harmonics model is not built (its per-pass directions are handed over on the host side)."""
    if getattr(model, "sh_deg", None) is not None:
        raise NotImplementedError(f"{who}: graph capture of an sh_deg model is not built; run it eagerly")
    if getattr(model, "is_cascade", False):      # (cascade.Cascade: two models, two optimizer states)
        raise NotImplementedError(f"{who}: graph capture of a two-network Cascade is not built; run it eagerly")


def cached_graph(cache: dict, key, make):
    """cache[key], created with make() on a miss; the cache holds at most MAX_CACHED_GRAPHS captured graphs (least recently used one
    dropped: a graph owns a private memory pool with every activation of its batch shape).  Dropping a graph is safe - the buffers a
    capture bakes in besides its own pool (the model's cached buffers, the library workspaces of ops.py) are never freed."""
    g = cache.pop(key, None)
    if g is None:
        while len(cache) >= MAX_CACHED_GRAPHS:
            cache.pop(next(iter(cache)))
        g = make()
    cache[key] = g              # (re-inserted: dict order = recency)
    return g


class GraphedTrainStep:
    """step = GraphedTrainStep(model, rgbs, rays, image_indices, n_samples, seg_tokens, ...); res = step(rgbs, rays, image_indices)

    Same result dict as SwitchNeRF.train_step (tensors live in static graph memory: read them before the next call).  The inputs
    are copied into static buffers; stratified jitter (perturb > 0) and the sigma noise (noise_std > 0) are drawn inside the
    graph from the device generator, like rendering.py:582 / :366 - or, with the model's device noise on (set_device_noise), from the
    seeded generator: the replays then equal the eager steps bit for bit.  Only the plain (non-hierarchical, non-mip) step is graphed.

    split_backward (default: on when torch.distributed runs more than one rank): the step is captured as TWO graphs cut behind the
    expert weight gradients (SwitchNeRF.backward_net_a / _b).  Between the replays the all-reduce of the expert block of the flat
    gradient - final at that point, 14.7 of 15.8 MB - is issued on the model's side stream and travels while the second graph (router
    backward, front backward chain, dense weight gradients: a quarter of the step) runs; the dense prefix follows behind it.  This is
    the overlap DDP's buckets give the reference (runner.py:203-207); with one all-reduce behind the whole backward nothing hides it
    at 1024 rays per GPU.  Results are bit-identical to the single-graph step (same sums over the same ranks).

    Finite guard (model.set_check_finite, switched on before the capture): the guard's launch is part of the captured step and the
    guarded optimizer launches behind the replay read its device flag, so ONE capture drops the step on a bad batch and takes it on a
    good one, with no host read in between; res["step_ok"] is the flag of the last replay."""

    def __init__(self, model, rgbs, rays, image_indices, n_samples: int, seg_tokens: int, perturb: float = 1.0, noise_std: float = 1.0,
                 routing_override=None, warmup: int = 2, split_backward=None):
        _refuse_sh(model, "GraphedTrainStep")
        N, S = rays.shape[0], int(n_samples)
        if model.ep is not None:
            seg_payload = model.E * model.capacity(min(int(seg_tokens), N * S)) * model.M * (4 if model.dtype == torch.float32 else 2)
            if not (model.ep.capturable and model.ep.use_padded(seg_payload)):
                raise ValueError("GraphedTrainStep: the expert-parallel step with unequal splits reads their sizes on the host and cannot be "
                                 "captured; use SwitchNeRF.train_step, or ExpertParallel(..., padded=True) (equal, capacity-padded splits)")
        self.model = model
        dev = model.dev
        self.rgbs, self.rays, self.idx = rgbs.clone(), rays.clone(), image_indices.clone()
        P = N * S
        if split_backward is None:
            import torch.distributed as dist
            split_backward = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        self.split = bool(split_backward) and model.ep is None
        if model.loss_scaler is not None:
            model._loss_scale_tensor()                     # exists before the capture (it is read, not created, inside the graph)
        ro = None if routing_override is None else routing_override.to(dev).int().contiguous()

        # device noise on (SwitchNeRF.set_device_noise): no noise tensors are passed - the step draws from the seeded generator and its
        # last launch advances the step counter, so the captured step holds the draws AND the advance
        dn = model.device_noise

        def run():
            pr = torch.rand(N, S, device=dev) if perturb > 0 and not dn else None
            noise = torch.randn(P, device=dev) * noise_std if noise_std > 0 and not dn else None
            return model.grad_step(self.rgbs, self.rays, self.idx, S, min(int(seg_tokens), P), perturb=perturb, perturb_rand=pr,
                                   sigma_noise=noise, routing_override=ro, split=self.split, sigma_noise_std=noise_std if dn else 0.0)

        was_profile, model.profile = model.profile, False
        step0 = model.noise_state_dict()["step"]           # the warm-up steps advance the noise counter like real ones: put it back
        skipped0 = model._guard["skipped"].clone() if model.check_finite else None      # (and may count as skipped: put back too)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                      # warm-up on a side stream: allocates every cached buffer / workspace
            for _ in range(max(1, warmup)):
                r_ = run()
                if self.split:
                    model.backward_net_b(r_["bwd_b"])
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        if dn:
            model.noise.rewind(step0)
            torch.cuda.synchronize()
        if skipped0 is not None:
            model._guard["skipped"].copy_(skipped0)
            torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=side):
            self.res = run()
        self.captures = 1                                  # captures of the step so far: replays never add one
        self.graph_b = None
        if self.split:
            self.graph_b = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph_b, stream=side, pool=self.graph.pool()):
                model.backward_net_b(self.res["bwd_b"])
        self.copies = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.copies, stream=side):
            model.refresh_compute_copies()
        model.profile = was_profile

    def __call__(self, rgbs=None, rays=None, image_indices=None, grad_allreduce=None, optimizer_step=True, should_accumulate=None):
        """should_accumulate: gradient accumulation (SwitchNeRF.set_accumulation) - passed to apply_step; the captured graphs are the
        same, the accumulate launch and the fused last step run eagerly behind the replay."""
        m = self.model
        if rgbs is not None:
            self.rgbs.copy_(rgbs)
        if rays is not None:
            self.rays.copy_(rays)
        if image_indices is not None:
            self.idx.copy_(image_indices)
        self.graph.replay()
        ar = grad_allreduce
        # finite guard: the ranks' MIN over the flag is the all-reduce OBJECT's; the split backward below hands apply_step a closure
        flag_ar = getattr(grad_allreduce, "all_ranks_ok", None) if m.check_finite else None
        if self.graph_b is not None:
            if ar is not None and hasattr(ar, "begin") and m.accum_steps == 1:      # (accumulating: ONE all-reduce, of the buffer, in apply_step)
                ar.begin(m.grad[m.n_dense:], m.side)       # the expert block is final: it travels under the second backward graph
                ar = lambda _view, f=grad_allreduce: f.finish(m.grad[: m.n_dense])
            self.graph_b.replay()
        # all-reduce, loss-scale handling (fp16: inf check, skipped step, scale update - the captured step reads the scale from a
        # device scalar), Adam and the refresh of the compute copies (a second small graph): SwitchNeRF.apply_step
        stepped = m.apply_step(ar, optimizer_step, refresh=self.copies.replay, should_accumulate=should_accumulate,
                               **(dict(flag_allreduce=flag_ar) if flag_ar is not None else {}))
        if m.accum_steps > 1:
            self.res["optimizer_stepped"] = stepped
        return self.res


class GraphedRender:
    """The inference forward of ONE ray-batch shape (render_rays in eval mode: no jitter, no noise, no activation saves), captured
    once and replayed: Runner.render_image (runner.py:2835-2885) calls render_rays for every image_pixel_batch_size rays of every
    image with the same shapes - ~60 launches per call that the host otherwise enqueues slower than the GPU runs them.

        g = GraphedRender(model, rays, image_indices, n_samples, seg_tokens, fine_samples=F, no_batch=model.moe_no_batch)
        out = g(rays, image_indices)     # dict: rgb, depth, depth_variance, l_aux_coarse, idx_coarse, sigma_coarse, raw_coarse (+ *_fine)

    The returned tensors live in the graph's static memory: consume (or clone) them before the next call.  Expert-parallel
    evaluation reads split sizes on the host (list_all_to_all) and cannot be captured."""

    def __init__(self, model, rays, image_indices, n_samples: int, seg_tokens: int, fine_samples: int = 0, no_batch: bool = False,
                 warmup: int = 2):
        _refuse_sh(model, "GraphedRender")
        if model.ep is not None and not model.ep.local:
            raise ValueError("GraphedRender: expert-parallel evaluation exchanges host-sized splits and cannot be captured")
        self.model = model
        dev = model.dev
        self.rays, self.idx = rays.clone().contiguous(), image_indices.clone().contiguous()
        N, S, F = rays.shape[0], int(n_samples), int(fine_samples)
        self.key = (N, S, F, int(seg_tokens), bool(no_batch))

        def run():
            with torch.no_grad():
                chunk = min(int(seg_tokens), N * S)
                c, cf, o = model.render_forward(self.rays, self.idx, S, F, chunk, 0.0, None, None, None, None, training=False,
                                                no_batch=no_batch)
                res = dict(rgb=o["rgb"], depth=o["depth"], depth_variance=o["depth_variance"], l_aux_coarse=c["l_aux"],
                           idx_coarse=c["idx"], sigma_coarse=c["raw"][:, 3], raw_coarse=c["raw"])
                if cf is not None:
                    res.update(l_aux_fine=cf["l_aux"], idx_fine=cf["idx"], sigma_fine=cf["raw"][:, 3], raw_fine=cf["raw"])
                return res

        was_profile, model.profile = model.profile, False
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                      # warm-up on the capture stream: allocates every cached buffer / workspace
            for _ in range(max(1, warmup)):
                run()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=side):
            self.out = run()
        model.profile = was_profile

    def __call__(self, rays=None, image_indices=None):
        if rays is not None:
            self.rays.copy_(rays)
        if image_indices is not None:
            self.idx.copy_(image_indices)
        self.graph.replay()
        return self.out


class GraphedRenderTrain:
    """The TRAINING render of one ray-batch shape as two captured graphs - forward and backward - behind autograd.RenderRaysFunction,
    so that the reference's own loop (runner.py:604-693: `render_rays` under autograd, `scaler.scale(loss).backward()`, torch.optim.Adam,
    ExponentialLR) runs the hot path with two host calls per step instead of ~150 launches:

        forward graph : [jitter / sigma noise drawn on the device] -> forward_rays / forward_hier (training=True, activations saved
                        into static buffers) -> rgb, gate losses, depth, depth variance
        backward graph: static d_rgb, d_gate_loss -> grad.zero_() + compositing backward + backward_net -> the flat gradient

    Enabled per model with `nerf.graph_train = True` (rendering.render_rays then takes this path in training mode; one instance is
    cached per batch shape).  The loss itself, the optimizer and the scheduler stay ordinary torch code between the two replays.
    Not for expert-parallel models (their step issues collectives between its kernels)."""

    def __init__(self, model, rays, image_indices, n_samples: int, fine_samples: int, seg_tokens: int, perturb: float, noise_std: float,
                 warmup: int = 2):
        _refuse_sh(model, "GraphedRenderTrain")
        if model.ep is not None and not model.ep.local:
            raise ValueError("GraphedRenderTrain: expert-parallel training is not captured")
        from .autograd import render_outputs
        self.model = model
        dev = model.dev
        N, S, F = rays.shape[0], int(n_samples), int(fine_samples)
        self.rays, self.idx = rays.clone().contiguous(), image_indices.clone().contiguous()
        self.d_rgb = torch.zeros(N, 3, dtype=torch.float32, device=dev)
        chunk = min(int(seg_tokens), N * S)

        dn = model.device_noise          # seeded device noise: the passes draw it themselves; the forward graph ends in the counter's advance
        std = noise_std if dn else 0.0

        def fwd():
            pr = torch.rand(N, S, device=dev) if perturb > 0 and not dn else None                        # rendering.py:582
            noise = torch.randn(N * S, device=dev) * noise_std if noise_std > 0 and not dn else None     # rendering.py:366
            noise_f = torch.randn(N * F, device=dev) * noise_std if F > 0 and noise_std > 0 and not dn else None
            state = model.render_forward(self.rays, self.idx, S, F, chunk, perturb, pr, None, noise, noise_f, training=True,
                                         no_batch=model.moe_no_batch, sigma_noise_std=std)
            model._noise_advance()
            return state, render_outputs(*state)

        def bwd(state):
            model.grad.zero_()
            model.render_backward(*state, self.d_rgb, self.d_laux_c, self.d_laux_f)

        was_profile, model.profile = model.profile, False
        step0 = model.noise_state_dict()["step"]           # the warm-up passes advance the noise counter: put it back before the capture
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                      # warm-up on the capture stream: allocates every cached buffer / workspace
            for _ in range(max(1, warmup)):
                st, outs = fwd()
                self.d_laux_c = torch.zeros_like(outs[1])
                self.d_laux_f = torch.zeros_like(outs[2])
                bwd(st)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        if dn:
            model.noise.rewind(step0)
            torch.cuda.synchronize()
        self.fwd_graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.fwd_graph, stream=side):
            self.state, self.outs = fwd()
        self.bwd_graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.bwd_graph, stream=side, pool=self.fwd_graph.pool()):
            bwd(self.state)
        model.profile = was_profile

    generation = 0           # forward replays so far: the static activation buffers belong to the LAST one (autograd.py checks it)

    def forward(self, rays, image_indices):
        self.rays.copy_(rays)
        self.idx.copy_(image_indices)
        self.fwd_graph.replay()
        self.generation += 1
        return self.state, self.outs

    def backward(self, d_rgb, d_laux_c, d_laux_f):
        self.d_rgb.copy_(d_rgb)
        self.d_laux_c.copy_(d_laux_c)
        if self.d_laux_f.numel():
            self.d_laux_f.copy_(d_laux_f)
        self.bwd_graph.replay()
        return self.model.grad


class GraphedBackgroundStep:
    """step = GraphedBackgroundStep(scene, rgbs, rays, image_indices, n_samples, seg_tokens, ...); res = step(rgbs, rays, image_indices)

    The training step of a background.BackgroundScene in its padded form (bg_capacity = C rows for the background model, default the
    batch's N rays) captured once and replayed - built like GraphedTrainStep: static input buffers, warm-up on a side stream, the
    device-noise counter put back behind the warm-up, ONE capture of grad.zero_() + forward + loss + backward of both models + the
    noise advance (BackgroundScene.grad_step), and a second small graph for both models' refresh_compute_copies.  The tail
    (BackgroundScene.apply_step: the 8-byte readback of (n_bg, n_out), all-reduce, the shared loss scaler, both Adam steps) runs outside
    the graph.  Same result dict as BackgroundScene.train_step (tensors live in static graph memory: read them before the next call).

    One capture serves every batch of its shape, whatever share of its rays leaves the bound - up to C of them: a batch with more
    raises RuntimeError, one with cameras outside the bound raises like the eager step, in both cases with no parameter touched (the
    noise counter has advanced, as in the eager padded step).  With the scene's device noise on (BackgroundScene.set_device_noise) the
    replays equal the eager padded steps bit for bit; without it the jitter and the sigma noise of both models are drawn inside the graph
    from the framework's device generator.  Only the plain step (fine_samples = 0) is graphed; the hierarchical padded step stays eager."""

    def __init__(self, scene, rgbs, rays, image_indices, n_samples: int, seg_tokens: int, perturb: float = 1.0, noise_std: float = 1.0,
                 bg_capacity=None, warmup: int = 2):
        nerf, bg = scene.nerf, scene.bg
        N, S = rays.shape[0], int(n_samples)
        P = N * S
        if nerf.ep is not None:
            seg_payload = nerf.E * nerf.capacity(min(int(seg_tokens), P)) * nerf.M * (4 if nerf.dtype == torch.float32 else 2)
            if not (nerf.ep.capturable and nerf.ep.use_padded(seg_payload)):
                raise ValueError("GraphedBackgroundStep: the expert-parallel foreground step with unequal splits reads their sizes on the "
                                 "host and cannot be captured; use BackgroundScene.train_step, or ExpertParallel(..., padded=True)")
        scene._check_noise_sources()
        if scene.accum_steps > 1:
            raise NotImplementedError(scene._ACCUM_PADDED)
        if scene.check_finite:
            raise NotImplementedError(scene._GUARD_PADDED)
        self.scene = scene
        dev = scene.dev
        C = self.bg_capacity = N if bg_capacity is None else int(bg_capacity)
        if not 1 <= C <= N:
            raise ValueError(f"GraphedBackgroundStep: bg_capacity {C} outside [1, {N} rays]")
        self.rgbs, self.rays, self.idx = rgbs.clone().contiguous(), rays.clone().contiguous(), image_indices.clone().contiguous()
        if scene.loss_scaler is not None:
            for m in (nerf, bg):
                m._loss_scale_tensor()                     # exist before the capture (read, not created, inside the graph)
        dn = scene.device_noise                            # on: the step draws from the seeded generator, nothing is passed
        Sb = S // 2

        def run():
            kw = {}
            if not dn:
                if perturb > 0:
                    kw.update(perturb_rand=torch.rand(N, S, device=dev), perturb_rand_bg=torch.rand(C, Sb, device=dev))
                if noise_std > 0:
                    kw.update(sigma_noise=torch.randn(P, device=dev) * noise_std, sigma_noise_bg="randn")
            res = scene.grad_step(self.rgbs, self.rays, self.idx, S, min(int(seg_tokens), P), perturb, 0, C, noise_std=noise_std, **kw)
            scene._noise_advance()
            return res

        profiles = (nerf.profile, bg.profile)
        nerf.profile = bg.profile = False
        step0 = scene.noise_state_dict()["step"]           # the warm-up steps advance the noise counter like real ones: put it back
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                      # warm-up on a side stream: allocates every cached buffer / workspace
            for _ in range(max(1, warmup)):
                run()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        if dn:
            scene.noise.rewind(step0)
            torch.cuda.synchronize()
        # the background model's cached buffers grow with the largest row count seen (a later eager compact step on a larger batch
        # replaces them): the capture keeps the ones it baked in alive
        self._held = list(bg._bufs.values()) + [getattr(bg, "_ones", None)]
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=side):
            self.res = run()
        self.copies = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.copies, stream=side):
            nerf.refresh_compute_copies()
            bg.refresh_compute_copies()
        nerf.profile, bg.profile = profiles

    def __call__(self, rgbs=None, rays=None, image_indices=None, grad_allreduce=None, optimizer_step=True):
        scene = self.scene
        if rgbs is not None:
            self.rgbs.copy_(rgbs)
        if rays is not None:
            self.rays.copy_(rays)
        if image_indices is not None:
            self.idx.copy_(image_indices)
        if scene.loss_scaler is not None:
            for m in (scene.nerf, scene.bg):
                m._loss_scale_tensor()                     # a scale the caller set on the host reaches the device scalar the replay reads
        self.graph.replay()
        ctx = self.res["ctx"]
        ctx["Nb"] = ctx["n_out"] = None                    # the counts of THIS replay are read in apply_step
        return scene.apply_step(self.res, optimizer_step, grad_allreduce, refresh=self.copies.replay, advance=False)


class GraphedMegaStep:
    """step = GraphedMegaStep(model, rgbs, rays, image_indices, n_samples, cell_capacity, ...); res = step(rgbs, rays, image_indices)

    The joint training step of a mega.MegaNeRF in its padded form (cell_capacity = C rows per cell, or (C_coarse, C_fine)) captured once
    and replayed - built like GraphedBackgroundStep: static input buffers, warm-up on a side stream, ONE capture of every cell's
    grad.zero_() + the padded grad_step (coarse only, or coarse + fine with fine_samples > 0), and a second small graph for every cell's
    refresh_compute_copies.  The tail (MegaNeRF.apply_step(res=...): the 8-byte readback of the overflow counts, one Adam step per cell
    through optim.apply_tail, the copies graph) runs outside the graph.  Same result dict as MegaNeRF.train_step (tensors live in
    static graph memory: read them before the next call).

    One capture serves every batch of its shape, however its points fall over the cells - up to C per cell: a batch with more in a cell
    raises RuntimeError from the tail with no parameter touched, and the next replay is unaffected.  The jitter (perturb > 0) and the
    sigma noise of both passes (noise_std > 0) are drawn inside the graph from the framework's device generator - or, with the model's
    seeded device noise on (MegaNeRF.set_device_noise before the capture), by the step itself: no noise tensor is passed, the captured
    launches read the device step counter and the step's last captured launch advances it.  The counter is put back behind the warm-up
    runs, so the first replay is the step it was set to and the replays equal the eager padded steps bit for bit.
    Not built: spherical-harmonics cells, data parallelism (no gradient all-reduce), the xyz_real background half, a grouped launch
    over the cells."""

    def __init__(self, model, rgbs, rays, image_indices, n_samples: int, cell_capacity, perturb: float = 1.0, noise_std: float = 1.0,
                 fine_samples: int = 0, warmup: int = 2):
        model._need_joint("GraphedMegaStep")
        if cell_capacity is None:
            raise ValueError("GraphedMegaStep: cell_capacity is required - the compact form reads the cells' row counts on the host and "
                             "cannot be captured")
        self.cell_capacity = model._capacity(cell_capacity)
        self.model = model
        dev = model.dev
        N, S, F = rays.shape[0], int(n_samples), int(fine_samples)
        self.rgbs, self.rays, self.idx = rgbs.clone().contiguous(), rays.clone().contiguous(), image_indices.clone().contiguous()

        dn = model.device_noise          # seeded device noise: nothing is passed - the step draws, and its last launch advances the counter

        def run():
            pr = torch.rand(N, S, device=dev) if perturb > 0 and not dn else None
            noise = torch.randn(N * S, device=dev) * noise_std if noise_std > 0 and not dn else None
            noise_f = torch.randn(N * F, device=dev) * noise_std if noise_std > 0 and F > 0 and not dn else None
            return model.grad_step(self.rgbs, self.rays, self.idx, S, perturb, pr, noise, F, None, noise_f, self.cell_capacity,
                                   sigma_noise_std=noise_std if dn else 0.0)

        profiles = [m.profile for m in model.sub_modules]
        for m in model.sub_modules:
            m.profile = False
        step0 = model.noise_state_dict()["step"]           # the warm-up steps advance the noise counter like real ones: put it back
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                      # warm-up on a side stream: allocates every cached buffer / workspace
            for _ in range(max(1, warmup)):
                run()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        if dn:
            model.noise.rewind(step0)
            torch.cuda.synchronize()
        # a cell's cached buffers grow with the largest row count seen (a later eager compact step with more rows in a cell replaces
        # them): the capture keeps the ones it baked in alive
        self._held = [list(m._bufs.values()) + [getattr(m, "_ones", None)] for m in model.sub_modules]
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=side):
            self.res = run()
        self.captures = 1                                  # captures of the step so far: replays never add one
        self.copies = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.copies, stream=side):
            for m in model.sub_modules:
                m.refresh_compute_copies()
        for m, p in zip(model.sub_modules, profiles):
            m.profile = p

    def __call__(self, rgbs=None, rays=None, image_indices=None, optimizer_step=True):
        if rgbs is not None:
            self.rgbs.copy_(rgbs)
        if rays is not None:
            self.rays.copy_(rays)
        if image_indices is not None:
            self.idx.copy_(image_indices)
        self.graph.replay()
        self.model.apply_step(None, optimizer_step, self.res, refresh=self.copies.replay)
        return self.res
