"""CPU-only: what rendering.render_rays / render_rays_mip hand back on every branch a host model can take - the sorted result keys,
each value's shape and dtype, the `bg_nerf_rays_present` flag - and how much of the framework generator the call consumed (after
torch.manual_seed(k): the value of the next torch.rand(1) behind the call), which a launch trace cannot see.  The library is mocked
(install_mock: every C-ABI call is a no-op, torch.empty returns zeros, three host decisions get consistent fakes); the mock goes in
through monkeypatch, so it is undone after each test.  scripts/step_launch_trace.py installs the same mock with a recording call
and traces the same cases (CASES, run_case).

EXPECTED holds literal values, written down from a run of this file on the commit BEFORE the render passes and the result assembly were
factored (five hand-written render passes, seven hand-written result dictionaries); they are not to be regenerated from the code under
test."""
import ctypes as C
from argparse import Namespace

import numpy as np
import pytest
import torch

import synth

CELL = dict(layer_dim=64, layers=2, skip_layers=(1,), pos_xyz_dim=3, pos_dir_dim=2, appearance_dim=8, appearance_count=10, xyz_dim=3)
CEN = np.array([[-0.5, -0.4, 0.1], [0.5, -0.3, -0.2], [0.0, 0.5, 0.3]], np.float32)
SEED = 11


def install_mock(setattr, call=None, p=None, pv=None):
    """The library mock on host tensors, through setattr(object, name, value) (monkeypatch.setattr, or the builtin for a script that
    exits afterwards).  call(name, *args) stands in for every C-ABI call (default: nothing), p / pv for ops._p / ops._pv (default: the
    address, no device check).  The mock's outputs are zeros, so three host decisions get consistent fakes: every token of a segment
    is routed to expert 0, every second ray continues into the background, point p belongs to cell p % K.  A host-resident model packs
    no compute copies, so refresh_compute_copies runs with the model's device reading as "cuda"."""
    from switch_nerf_amd import _lib, ops
    from switch_nerf_amd.model import SwitchNeRF

    class FakeLib:
        def __getattr__(self, k):
            return lambda *a: 4096

    class Stream:
        cuda_stream = 0

    class AsCuda:
        type = "cuda"

    def ptr(t):
        assert t is None or t.is_contiguous()
        return None if t is None else C.c_void_p(t.data_ptr())

    route, fg_bounds, cells_assign, cells_pack = ops.route_top1, ops.fg_bounds, ops.cells_assign, ops.cells_pack
    refresh = SwitchNeRF.refresh_compute_copies
    sched = torch.zeros(16, dtype=torch.int32)

    def fake_route(idx, gmax, gates, seg_tokens, n_experts, capacity, bpr, want_perm=True, want_drops=False, **kw):
        r = list(route(idx, gmax, gates, seg_tokens, n_experts, capacity, bpr, want_perm=want_perm, want_drops=want_drops, **kw))
        P = idx.shape[0]
        n_seg = P // seg_tokens
        loc, counts = r[0], r[1]
        loc.copy_(torch.arange(P, dtype=loc.dtype) % seg_tokens)
        counts.zero_()
        counts.view(n_seg, n_experts)[:, 0] = seg_tokens
        if want_drops:
            nd = max(seg_tokens - capacity, 0)
            r[5].copy_(torch.clamp(torch.arange(n_seg * n_experts + 1) + n_experts - 1, min=0) // n_experts * nd)
            tok = torch.arange(P).view(n_seg, seg_tokens)[:, capacity:].reshape(-1).to(torch.int32)
            r[6][: tok.numel()] = tok
        return tuple(r)

    def fake_fg_bounds(rays, center, radius, n_out=None):
        rays_fg, fg_far, last_delta, has_bg, n_out = fg_bounds(rays, center, radius, n_out)
        rays_fg.copy_(rays)
        fg_far.copy_(rays[:, 7])
        has_bg[::2] = 1
        return rays_fg, fg_far, last_delta, has_bg, n_out

    def fake_cells_assign(x, centroids, dim_start, margin):
        weights, counts = cells_assign(x, centroids, dim_start, margin)
        P, K = weights.shape
        weights[torch.arange(P), torch.arange(P) % K] = 1.0
        counts.copy_(torch.bincount(torch.arange(P) % K, minlength=K))
        return weights, counts

    def fake_cells_pack(weights, counts, rows_capacity=None):
        begin, rows, slot = cells_pack(weights, counts, rows_capacity)
        P, K = weights.shape
        cell = torch.arange(P) % K
        begin[1:] = torch.cumsum(counts, 0)
        rows[:P] = torch.sort(cell, stable=True)[1].to(torch.int32)
        slot.fill_(-1)
        slot[torch.arange(P), cell] = (torch.arange(P) // K).to(torch.int32)
        return begin, rows, slot

    def refresh_on_host(self):
        real = self.dev
        self.dev = AsCuda()
        try:
            refresh(self)
        finally:
            self.dev = real

    setattr(torch, "empty", torch.zeros)
    setattr(torch, "empty_like", torch.zeros_like)
    setattr(torch.cuda, "current_stream", lambda *a: Stream())
    setattr(_lib, "load", lambda: FakeLib())
    setattr(ops, "call", call or (lambda name, *args: None))
    setattr(ops, "_stream", lambda: C.c_void_p(0))
    setattr(ops, "_p", p or ptr)
    setattr(ops, "_pv", pv or (lambda t: C.c_void_p(t.data_ptr())))
    setattr(ops, "chain_sched", lambda dev, key: sched)
    setattr(ops, "route_top1", fake_route)
    setattr(ops, "fg_bounds", fake_fg_bounds)
    setattr(ops, "cells_assign", fake_cells_assign)
    setattr(ops, "cells_pack", fake_cells_pack)
    setattr(SwitchNeRF, "refresh_compute_copies", refresh_on_host)


def _hparams(S, F, **kw):
    return Namespace(**dict(dict(coarse_samples=S, fine_samples=F, model_chunk_size=4096, perturb=1.0, use_sigma_noise=True,
                                 sigma_noise_std=1.0, moe_return_gates=True, return_sigma=True), **kw))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# kind: the model and the entry point; train: the model's mode; grad: under autograd, with loss.backward() behind the call (else under
# torch.no_grad()); dn: the model's / the scene's seeded device noise on; F: fine samples; flags: (get_depth, get_depth_variance,
# get_bg_fg_rgb)
CASES = {
    "plain_eval_coarse": dict(kind="plain", F=0),
    "plain_eval_fine": dict(kind="plain", F=8),
    "plain_eval_fine_no_depth": dict(kind="plain", F=8, flags=(False, False, False)),
    "plain_train_nograd_coarse": dict(kind="plain", F=0, train=True),
    "plain_train_nograd_fine": dict(kind="plain", F=8, train=True),
    "plain_train_nograd_fine_dn": dict(kind="plain", F=8, train=True, dn=True),
    "plain_autograd_coarse": dict(kind="plain", F=0, train=True, grad=True),
    "plain_autograd_fine": dict(kind="plain", F=8, train=True, grad=True),
    "plain_autograd_coarse_dn": dict(kind="plain", F=0, train=True, grad=True, dn=True),
    "plain_autograd_fine_dn": dict(kind="plain", F=8, train=True, grad=True, dn=True),
    "plain_autograd_fine_points": dict(kind="plain", F=8, train=True, grad=True,
                                       hp=dict(return_pts=True, return_pts_rgb=True, return_pts_alpha=True, return_alpha=True)),
    "bg_eval_coarse": dict(kind="bg", F=0, flags=(True, True, True)),
    "bg_eval_fine": dict(kind="bg", F=8, flags=(True, True, True)),
    "bg_train_fine": dict(kind="bg", F=8, train=True, flags=(True, True, True)),
    "bg_train_fine_dn": dict(kind="bg", F=8, train=True, dn=True),
    "cascade_eval_coarse": dict(kind="cascade", F=0),
    "cascade_eval_fine": dict(kind="cascade", F=8),
    "cascade_train_nograd_fine": dict(kind="cascade", F=8, train=True),
    "cascade_autograd_fine": dict(kind="cascade", F=8, train=True, grad=True),
    "mip_eval_coarse": dict(kind="mip", F=0),
    "mip_eval_fine": dict(kind="mip", F=8),
    "mip_train_fine": dict(kind="mip", F=8, train=True),
    "mip_train_fine_dn": dict(kind="mip", F=8, train=True, dn=True),
    "mega_eval_coarse": dict(kind="mega", F=0),
    "mega_eval_fine": dict(kind="mega", F=8),
    "mega_bg_eval_fine": dict(kind="mega_bg", F=8, flags=(True, True, True)),
}


def run_case(kind, F, train=False, grad=False, dn=False, flags=(True, True, False), hp=None, N=12, S=8):
    """One render call on freshly built host models (the mock installed by the caller) -> (results, bg_nerf_rays_present, the models
    whose buffers a trace names).  The framework generator is seeded with SEED right before the call."""
    from switch_nerf_amd import rendering
    from switch_nerf_amd.cascade import Cascade
    from switch_nerf_amd.dense import DenseNeRF
    from switch_nerf_amd.mega import MegaNeRF
    from switch_nerf_amd.model import SwitchNeRF
    f32 = torch.float32
    h = _hparams(S, F, **(hp or {}))
    bg, center, radius, radii = None, None, None, None
    rays, img, _ = (synth.make_bg_rays if kind in ("bg", "mega_bg") else synth.make_rays)(401, N)
    if kind in ("plain", "mip"):
        nerf = SwitchNeRF(synth.BUILDING, dtype=torch.bfloat16, device="cpu")
        models = [nerf]
        if kind == "mip":
            radii = torch.full((N, 1), 0.01)
    elif kind == "bg":
        nerf, bg = SwitchNeRF(synth.BUILDING, dtype=torch.bfloat16, device="cpu"), DenseNeRF(synth.DENSE_BG, dtype=f32, device="cpu")
        models, center, radius = [nerf, bg], synth.SPHERE_CENTER, synth.SPHERE_RADIUS
    elif kind == "cascade":
        models = [DenseNeRF(CELL, dtype=f32, device="cpu", seed=i) for i in range(2 if F else 1)]
        nerf = Cascade(*models)
        h.use_cascade, h.moe_return_gates = True, False
    else:
        models = [DenseNeRF(CELL, dtype=f32, device="cpu", seed=i) for i in range(3)]
        nerf = MegaNeRF(models, CEN, 1.15, False, False)
        h.moe_return_gates = False
        if kind == "mega_bg":
            cells = [DenseNeRF(dict(CELL, xyz_dim=4), dtype=f32, device="cpu", seed=3 + i) for i in range(3)]
            bg, center, radius = MegaNeRF(cells, CEN, 1.15, True, False), synth.SPHERE_CENTER, synth.SPHERE_RADIUS
            models = models + cells
    if kind not in ("mega", "mega_bg"):
        nerf.train(train)
        if bg is not None:
            bg.train(train)
    if dn:
        (rendering.background_scene(nerf, bg, center, radius) if bg is not None else nerf).set_device_noise(7)
    torch.manual_seed(SEED)
    with torch.enable_grad() if grad else torch.no_grad():
        if kind == "mip":
            res, present = rendering.render_rays_mip(nerf, _t(rays), radii, _t(img), h, *flags[:2])
        else:
            res, present = rendering.render_rays(nerf, bg, _t(rays), _t(img), h, center, radius, *flags)
        if grad:
            typ = "fine" if F else "coarse"
            loss = res[f"rgb_{typ}"].sum() + res["gate_loss_coarse"].sum() + (res["gate_loss_fine"].sum() if F else 0.0)
            if kind == "cascade":
                loss = loss + res["rgb_coarse"].sum()
            loss.backward()
    return res, present, models


def describe(res, present):
    """("key[shape]dtype" of every result in key order, bg_nerf_rays_present, the next draw of the framework generator)"""
    short = {torch.float32: "f", torch.int64: "i"}
    keys = " ".join("%s%s%s" % (k, list(v.shape), short[v.dtype]) for k, v in sorted(res.items()))
    return keys, bool(present), "%.8f" % torch.rand(1).item()


# f = float32, i = int64; N = 12 rays, S = 8 coarse and F = 8 fine samples
_D = lambda typ: f"depth_{typ}[12]f depth_variance_{typ}[12]f "
_BGFG = lambda typ: f"bg_depth_{typ}[12]f bg_rgb_{typ}[12, 3]f " + _D(typ) + f"fg_depth_{typ}[12]f fg_rgb_{typ}[12, 3]f "
_GATES_C, _GATES_F = "moe_gates_coarse[12, 8, 1, 1]i ", "moe_gates_fine[12, 8, 1, 1]i "
_PLAIN_C = _D("coarse") + "gate_loss_coarse[1]f " + _GATES_C + "rgb_coarse[12, 3]f sigma_coarse[12, 8]f"
_PLAIN_F_TAIL = "gate_loss_coarse[1]f gate_loss_fine[1]f " + _GATES_C + _GATES_F + "rgb_fine[12, 3]f sigma_coarse[12, 8]f sigma_fine[12, 8]f"
_PLAIN_F = _D("fine") + _PLAIN_F_TAIL
_BG_F_TAIL = "gate_loss_coarse[1]f gate_loss_fine[1]f " + _GATES_C + _GATES_F + "rgb_fine[12, 3]f"
_CASCADE_F = _D("fine") + "gate_loss_coarse[1]f gate_loss_fine[2]f rgb_coarse[12, 3]f rgb_fine[12, 3]f sigma_coarse[12, 8]f sigma_fine[12, 16]f"
_MIP_F = (_D("fine") + "gate_loss_coarse[1]f gate_loss_fine[1]f moe_gates_coarse[12, 7, 1, 1]i moe_gates_fine[12, 7, 1, 1]i "
          "rgb_coarse[12, 3]f rgb_fine[12, 3]f")
_NONE = "0.14904171"          # nothing drawn from the framework generator
EXPECTED = {
    "plain_eval_coarse": (_PLAIN_C, False, _NONE),
    "plain_eval_fine": (_PLAIN_F, False, _NONE),
    "plain_eval_fine_no_depth": (_PLAIN_F_TAIL, False, _NONE),
    "plain_train_nograd_coarse": (_PLAIN_C, False, "0.63078296"),
    "plain_train_nograd_fine": (_PLAIN_F, False, "0.41347688"),
    "plain_train_nograd_fine_dn": (_PLAIN_F, False, _NONE),
    "plain_autograd_coarse": (_PLAIN_C, False, "0.63078296"),
    "plain_autograd_fine": (_PLAIN_F, False, "0.41347688"),
    "plain_autograd_coarse_dn": (_PLAIN_C, False, _NONE),
    "plain_autograd_fine_dn": (_PLAIN_F, False, _NONE),
    "plain_autograd_fine_points": ("alpha_coarse[12, 8]f alpha_fine[12, 16]f " + _D("fine") + "gate_loss_coarse[1]f gate_loss_fine[1]f "
                                   + _GATES_C + _GATES_F + "pts_alpha_coarse[12, 8]f pts_alpha_fine[12, 8]f pts_coarse[12, 8, 3]f "
                                   "pts_fine[12, 8, 3]f pts_rgb_coarse[12, 8, 3]f pts_rgb_fine[12, 8, 3]f rgb_fine[12, 3]f "
                                   "sigma_coarse[12, 8]f sigma_fine[12, 8]f", False, "0.41347688"),
    "bg_eval_coarse": (_BGFG("coarse") + "gate_loss_coarse[1]f " + _GATES_C + "rgb_coarse[12, 3]f", True, _NONE),
    "bg_eval_fine": (_BGFG("fine") + _BG_F_TAIL, True, _NONE),
    "bg_train_fine": (_BGFG("fine") + _BG_F_TAIL, True, "0.51652741"),
    "bg_train_fine_dn": (_D("fine") + _BG_F_TAIL, True, _NONE),
    "cascade_eval_coarse": (_D("coarse") + "gate_loss_coarse[1]f rgb_coarse[12, 3]f sigma_coarse[12, 8]f", False, _NONE),
    "cascade_eval_fine": (_CASCADE_F, False, _NONE),
    "cascade_train_nograd_fine": (_CASCADE_F, False, "0.00107002"),
    "cascade_autograd_fine": (_CASCADE_F, False, "0.00107002"),
    "mip_eval_coarse": (_D("coarse") + "gate_loss_coarse[1]f moe_gates_coarse[12, 7, 1, 1]i rgb_coarse[12, 3]f", False, _NONE),
    "mip_eval_fine": (_MIP_F, False, "0.91107416"),          # (the fine level resamples with randomized = hparams.perturb in eval too)
    "mip_train_fine": (_MIP_F, False, "0.01534671"),
    "mip_train_fine_dn": (_MIP_F, False, _NONE),
    "mega_eval_coarse": (_D("coarse") + "rgb_coarse[12, 3]f sigma_coarse[12, 8]f", False, _NONE),
    "mega_eval_fine": (_D("fine") + "rgb_fine[12, 3]f sigma_coarse[12, 8]f sigma_fine[12, 8]f", False, _NONE),
    "mega_bg_eval_fine": (_BGFG("fine") + "rgb_fine[12, 3]f sigma_coarse[12, 8]f sigma_fine[12, 8]f", True, _NONE),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_render_results(name, monkeypatch):
    install_mock(monkeypatch.setattr)
    res, present, _ = run_case(**CASES[name])
    keys, present, nxt = describe(res, present)
    want_keys, want_present, want_next = EXPECTED[name]
    assert keys == want_keys
    assert present == want_present
    assert nxt == want_next


def test_mock_is_undone():
    """The torch.empty -> zeros substitution and the library mock do not outlive a test."""
    from switch_nerf_amd import _lib, ops
    assert torch.empty is not torch.zeros and torch.empty_like is not torch.zeros_like
    assert ops.call is _lib.call
