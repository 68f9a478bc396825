"""CPU launch trace of the step's host-side orchestration: every C-ABI call a step makes (entry point, every scalar argument, every
descriptor field; pointers named after the model buffer / context key they fall into, `tmp` otherwise) with the library mocked, so no
GPU is needed.  For host-side refactors: record the trace on two checkouts and compare - equal traces = the same kernels with the same
arguments in the same order.  Not covered: the side-stream sections and the profile hooks (a CPU model has no side stream).

    python scripts/step_launch_trace.py OUT.json [ROOT [COUNTER]]     record (ROOT: the checkout whose switch_nerf_amd is traced, default
                                                                      this one; COUNTER: the attribute path of a noise holder's step
                                                                      counter there, default noise.step)
    python scripts/step_launch_trace.py --diff A.json B.json

Every tensor whose address goes into a call is kept alive until its case ends, so no later buffer can take a freed temporary's address:
a temporary always reads `tmp`, and two traces of one tree are equal.  A pointer that is `tmp` on one side and a named buffer on the other
is therefore a buffer that one side keeps under a model or context key and the other does not.

The mock is install_mock of tests/test_render_results_cpu.py (zeros for every output, consistent fakes for the routing, the foreground
bound and the cell membership, refresh_compute_copies run as if on the device) with a recording call.  A context's "head" record is not
named: it holds no buffer of its own, only the caller's tensors, which the context also keeps under the keys the backward reads.

The `tail_*` cases trace apply_step alone, over every owner (model, cascade, scene, cells), with a loss scaler attached by hand to the
fp32 host models; the torch calls of the tail (the inf check, accum.zero_(), the device scalar's fill_) are no library calls and do
not show here: tests/test_optim_tail_cpu.py pins what they leave behind.  The `render_*` cases are the calls of
tests/test_render_results_cpu.py through rendering.render_rays / render_rays_mip (autograd cases with their loss.backward()); that file
pins the result dictionaries and the framework generator's consumption.  Captured-graph paths need a device and are not traced.

The `noise_*` cases run with seeded device noise on (a seed, a nonzero starting step, a nonzero ray_base) through the public API only
and supply no noise tensors: the draws (seed, base, stream id, domain, scale), the in-kernel jitter and the counter's advance show with
the counter named `c*.noise_step`.  tests/test_noise_state_cpu.py pins the host state behind them."""
import ctypes as C
import functools
import json
import sys

import numpy as np
import torch

import os

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
if sys.argv[1] == "--diff":
    a, b = json.load(open(sys.argv[2])), json.load(open(sys.argv[3]))

    def walk(u, v, path, out):
        if isinstance(u, dict) and isinstance(v, dict):
            for f in u:
                walk(u[f], v.get(f), path + "." + f, out)
        elif isinstance(u, list) and isinstance(v, list) and len(u) == len(v):
            for i, (x, y) in enumerate(zip(u, v)):
                walk(x, y, path + "[%d]" % i, out)
        elif u != v:
            out.append((path, u, v))
    for k in a:
        out = []
        walk(a[k], b.get(k), "", out)
        print(k, "identical" if not out else "DIFFERENT in %d places" % len(out), len(a[k]), "calls")
        for p, u, v in out[:12]:
            print("   ", a[k][int(p.split("]")[0][1:])][0], p, str(u)[:120], "|", str(v)[:120])
    sys.exit(0)
out_path, root = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else HERE
COUNTER = sys.argv[3] if len(sys.argv) > 3 else "noise.step"
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(HERE, "tests"))
import synth  # noqa: E402

trace, ptr_ids = [], {}


def pid(v):
    if not v:
        return None
    return "@%d" % int(v)


def name_ptrs(obj, ranges):
    if isinstance(obj, str) and obj.startswith("@"):
        p = int(obj[1:])
        for a, b, n in ranges:
            if a <= p < b:
                return "%s+%d" % (n, p - a)
        return "tmp"
    if isinstance(obj, list):
        return [name_ptrs(x, ranges) for x in obj]
    if isinstance(obj, dict):
        return {k: name_ptrs(v, ranges) for k, v in obj.items()}
    return obj


def ranges_of(models, ctxs):
    r = []

    def add(t, n):
        if torch.is_tensor(t):
            if t.numel():
                r.append((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), n))
        elif isinstance(t, (list, tuple)):
            for i, x in enumerate(t):
                add(x, "%s.%d" % (n, i))
        elif isinstance(t, dict):
            for k, x in t.items():
                if k != "head":
                    add(x, "%s.%s" % (n, k))
    for mi, m in enumerate(models if isinstance(models, (list, tuple)) else [models]):
        pre = "m%d." % mi if mi else ""
        for k, t in m._bufs.items():
            for i, x in enumerate(t if isinstance(t, tuple) else (t,)):
                add(x, pre + "buf%r.%d" % (k, i))
        for k, t in m.wf.items():
            add(t, pre + "wf." + k)
        for k, t in m.wb.items():
            add(t, pre + "wb." + k)
        add(m.flat, pre + "flat"); add(m.grad, pre + "grad"); add(m.m, pre + "adam_m"); add(m.v, pre + "adam_v")
        add(getattr(m, "accum", None), pre + "accum")
    for ci, c in enumerate(ctxs):
        add(c, "c%d" % ci)
    return r


def ser(a):
    if a is None:
        return None
    if isinstance(a, C.c_void_p):
        return pid(a.value)
    if isinstance(a, (int, float, str, bool)):
        return a
    if isinstance(a, C.Structure):
        return {f[0]: (pid(getattr(a, f[0])) if f[1] is C.c_void_p else ser(getattr(a, f[0]))) for f in a._fields_}
    if isinstance(a, C.Array):
        return [ser(x) for x in a]
    if hasattr(a, "_obj"):
        return ser(a._obj)
    if hasattr(a, "value"):
        return a.value
    return repr(type(a))


def fake_call(name, *args):
    s = [ser(a) for a in args]
    if name == "swn_mlp_chain":      # only the used layers
        d = s[0]
        d["layers"] = d["layers"][: d["n_layers"]]
    trace.append([name, s])


_alive = []


def _ptr(t):
    assert t is None or t.is_contiguous()
    _alive.append(t)
    return None if t is None else C.c_void_p(t.data_ptr())


def _ptr_view(t):      # (the address of a strided view: heads_coef_fwd's output slice)
    _alive.append(t)
    return C.c_void_p(t.data_ptr())


import test_render_results_cpu as render_cases  # noqa: E402

render_cases.install_mock(setattr, fake_call, _ptr, _ptr_view)      # (the mock of tests/test_render_results_cpu.py, with the recording call)
from switch_nerf_amd.model import SwitchNeRF  # noqa: E402
from switch_nerf_amd.dense import DenseNeRF  # noqa: E402

from switch_nerf_amd.background import BackgroundScene  # noqa: E402
from switch_nerf_amd.mega import MegaNeRF  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def train(N=64, S=64, chunk=2048, dtype=BF16, switches=None, ep=None, fine=0, dense=False, infer=False, **kw):
    if dense:
        m = DenseNeRF(synth.DENSE, dtype=dtype, device="cpu")
    else:
        m = SwitchNeRF(synth.BUILDING, dtype=dtype, device="cpu", **kw)
    if switches:
        m.set_kernel_switches(**switches)
    if ep is not None:
        from switch_nerf_amd.parallel import ExpertParallel
        m.set_expert_parallel(ExpertParallel(0, 1, m.E, **ep))
    rays, img, rgbs = synth.make_rays(301, N)
    g = torch.Generator().manual_seed(302)
    pr, noise = torch.rand(N, S, generator=g), torch.randn(N * S, generator=g)
    if infer:
        c = m.forward_rays(dev(rays), dev(img), S, chunk, training=False, no_batch=True)
        return m, [c]
    more = {}
    if fine:
        more = dict(fine_samples=fine, fine_u=torch.rand(N, fine, generator=g), sigma_noise_fine=torch.randn(N * fine, generator=g))
    st = m.grad_step(dev(rgbs), dev(rays), dev(img), S, chunk, perturb=1.0, perturb_rand=pr, sigma_noise=noise, **more)
    ctxs = [st["ctx"]] + ([st["ctx_fine"]] if "ctx_fine" in st else [])
    for c in list(ctxs):
        ctxs += list(c.get("parts") or ())
    return m, ctxs


CASES = {
    "fused": dict(),
    "fused_big": dict(N=2100, S=256, chunk=131072),
    "fused_tail_off": dict(switches=dict(fused_tail=False)),
    "fused_tail_off_big": dict(N=2100, S=256, chunk=131072, switches=dict(fused_tail=False)),
    "fused_tail_bwd_off": dict(switches=dict(fused_tail_bwd=False)),
    "tail_geom7": dict(switches=dict(fused_tail=False, tail_geom=7)),
    "no_fused_heads": dict(switches=dict(fused_heads=False)),
    "fp32": dict(dtype=F32),
    "cf0_packed": dict(capacity_factor=0.0),
    "cf0_packed_unfused": dict(capacity_factor=0.0, switches=dict(fused_tail=False)),
    "cf050_drops": dict(N=128, chunk=4096, capacity_factor=0.5),
    "ragged": dict(N=80, chunk=4096),
    "hierarchical": dict(fine=64),
    "no_batch_inference": dict(N=96, infer=True, capacity_factor=0.75),
    "no_batch_inference_unfused": dict(N=96, infer=True, switches=dict(fused_tail=False)),
    "ep_padded": dict(ep=dict(padded=True)),
    "ep_kept_rows": dict(ep=dict()),
    "ep_owner_tail": dict(ep=dict(owner_tail=True)),
    "ep_owner_tail_drops": dict(N=128, chunk=4096, capacity_factor=0.5, ep=dict(owner_tail=True)),
    "dense": dict(dense=True, chunk=4096),
    "dense_fp32_infer": dict(dense=True, chunk=4096, dtype=F32),
}


SH2 = dict(synth.DENSE, pos_dir_dim=0, sh_deg=2)
CELL = dict(layer_dim=64, layers=2, skip_layers=(1,), pos_xyz_dim=3, pos_dir_dim=2, appearance_dim=8, appearance_count=10, xyz_dim=3)
CELL_SH = dict(CELL, pos_dir_dim=0, sh_deg=2)
CEN = np.array([[-0.5, -0.4, 0.1], [0.5, -0.3, -0.2], [0.0, 0.5, 0.3]], np.float32)


def dense_sh_train(N=8, S=8):
    m = DenseNeRF(SH2, dtype=F32, device="cpu")
    rays, img, rgbs = synth.make_rays(301, N)
    g = torch.Generator().manual_seed(302)
    st = m.grad_step(dev(rgbs), dev(rays), dev(img), S, N * S, perturb=1.0, perturb_rand=torch.rand(N, S, generator=g),
                     sigma_noise=torch.randn(N * S, generator=g))
    return m, [st["ctx"]]


def points_call(cfg=synth.DENSE, sigma_only=False, xyz_dim=3, coef=False, training=False, P=40):
    """DenseNeRF.__call__ / forward_coef on P explicit points; the context does not leave the call, so only the model's buffers are named"""
    m = DenseNeRF(dict(cfg, xyz_dim=xyz_dim), dtype=F32, device="cpu")
    m.train(training)
    g = torch.Generator().manual_seed(303)
    sh = cfg.get("sh_deg") is not None
    x = torch.rand(P, xyz_dim if sigma_only else xyz_dim + (1 if sh else 4), generator=g)
    noise = torch.randn(P, generator=g)
    if coef:
        return m, [m.forward_coef(x, noise, torch.zeros(P, 3 * 9 + 1))]
    m(x, sigma_only, noise)
    return m, []


def bg_scene(fine=0, training=True, N=16, S=8):
    m, b = DenseNeRF(synth.DENSE, dtype=F32, device="cpu"), DenseNeRF(synth.DENSE_BG, dtype=F32, device="cpu")
    scene = BackgroundScene(m, b, synth.SPHERE_CENTER, synth.SPHERE_RADIUS)
    rays, img, _ = synth.make_bg_rays(304, N)
    g = torch.Generator().manual_seed(305)
    Nb = (N + 1) // 2
    more = {}
    if fine:
        more = dict(fine_samples=fine, fine_u=torch.rand(N, fine, generator=g), fine_u_bg=torch.rand(Nb, fine // 2, generator=g))
    ctx = scene.forward(dev(rays), dev(img), S, N * S, perturb=1.0, perturb_rand=torch.rand(N, S, generator=g),
                        perturb_rand_bg=torch.rand(Nb, S // 2, generator=g), training=training, **more)
    return [m, b], [ctx]


def mega(cfg=CELL, call=None, fine=0, N=12, S=4):
    subs = [DenseNeRF(cfg, dtype=F32, device="cpu", seed=i) for i in range(3)]
    sh = cfg.get("sh_deg") is not None
    m = MegaNeRF(subs, CEN, 1.15, False, False, joint_training=call is None, sh_training=call is None and sh)
    g = torch.Generator().manual_seed(306)
    if call is not None:
        P = N * S
        x, noise = torch.rand(P, 4 if sh else 7, generator=g), torch.randn(P, generator=g)
        if call == "rgb":
            m.call_rgb(x, torch.rand(N, 3, generator=g), S, noise)
        else:
            m(x[:, :3] if call == "sigma_only" else x, call == "sigma_only", noise)
        return subs, []
    rays, img, rgbs = synth.make_rays(307, N)
    more = {}
    if fine:
        more = dict(fine_samples=fine, fine_u=torch.rand(N, fine, generator=g), sigma_noise_fine=torch.randn(N * fine, generator=g))
    st = m.train_step(dev(rgbs), dev(rays), dev(img), S, perturb=1.0, perturb_rand=torch.rand(N, S, generator=g),
                      sigma_noise=torch.randn(N * S, generator=g), **more)
    return subs, [st["ctx"]] + ([st["ctx_fine"]] if fine else [])


def tail(group, kind="dense", A=1, scaler=False, calls=()):
    """The step's tail alone (apply_step: all-reduce stub, inf check, accumulation window, Adam, refresh of the compute copies) on a
    gradient of ones: the cases of tests/test_optim_tail_cpu.py, which pins the host state this trace cannot see."""
    owner, models = tail_cases._build(group, kind, scaler)
    tail_cases.drive(group, owner, models, A, scaler, calls, lambda view: 0.5, lambda: [m.refresh_compute_copies() for m in models])
    return models, []


def render(**kw):
    return render_cases.run_case(**kw)[2], []


import test_optim_tail_cpu as tail_cases  # noqa: E402

HASH = dict(n_levels=8, log2_table=12, base_res=4, per_level_scale=1.6, aabb_lo=(-1.2, -1.2, -1.2), aabb_hi=(1.2, 1.2, 1.2))


def counter(holder):
    return dict(noise_step=functools.reduce(getattr, COUNTER.split("."), holder))


def noise_step(N=64, S=64, chunk=2048, fine=0, hash_grid=False, mip=False, **kw):
    """grad_step / train_step_mip with device noise on and nothing supplied: jitter, sigma noise, fine u (and gate noise) are drawn"""
    m = SwitchNeRF(dict(synth.BUILDING, hash=HASH) if hash_grid else synth.BUILDING, dtype=BF16, device="cpu", **kw)
    m.set_device_noise(7, step=3, ray_base=5)
    rays, img, rgbs = synth.make_rays(301, N)
    if mip:
        st = m.train_step_mip(dev(rgbs), dev(rays), torch.full((N, 1), 1e-3), dev(img), S + 1, fine + 1, chunk, perturb=1.0, sigma_noise_std=1.0)
    else:
        st = m.grad_step(dev(rgbs), dev(rays), dev(img), S, chunk, perturb=1.0, fine_samples=fine, sigma_noise_std=1.0)
    return m, [st["ctx"]] + ([st["ctx_fine"]] if st.get("ctx_fine") is not None else []) + [counter(m)]


def noise_scene(fine=0, N=16, S=8):
    """BackgroundScene.train_step (compact form) with the scene's device noise on: both models' draws, one advance"""
    m, b = DenseNeRF(synth.DENSE, dtype=F32, device="cpu"), DenseNeRF(synth.DENSE_BG, dtype=F32, device="cpu")
    scene = BackgroundScene(m, b, synth.SPHERE_CENTER, synth.SPHERE_RADIUS)
    scene.set_device_noise(7, step=3, ray_base=5)
    rays, img, rgbs = synth.make_bg_rays(304, N)
    st = scene.train_step(dev(rgbs), dev(rays), dev(img), S, N * S, perturb=1.0, fine_samples=fine, noise_std=1.0)
    return [m, b], [st["ctx"], counter(scene)]


class _OnDevice(torch.Tensor):
    is_cuda = True      # (MoELayer.forward refuses host tensors; every launch behind it is mocked)


def noise_moe_layer(P=64, M=64, E=4):
    """One training forward of moe.MoELayer with gate noise drawn from the layer's seeded generator, and the advance behind it"""
    from switch_nerf_amd.moe import MoELayer
    layer = MoELayer(dict(type="top", k=1, capacity_factor=1.0, gate_noise=1.0), M, dict(type="expertmlp", count_per_node=E, layer_num=2),
                     seeds=(1, 1, 1), dtype=F32).train()
    layer.set_device_noise(7, step=3, row_base=5, device="cpu")
    layer(torch.rand(P, M, generator=torch.Generator().manual_seed(308)).as_subclass(_OnDevice))
    return [], [counter(layer)]

MORE_CASES = {
    **{"render_" + k: (render, v) for k, v in render_cases.CASES.items()},
    **{"tail_" + k: (tail, v) for k, v in tail_cases.CASES.items()},
    "dense_sh_train": (dense_sh_train, dict()),
    "call_dense": (points_call, dict()),
    "call_dense_training_mode": (points_call, dict(training=True)),
    "call_dense_sigma_only": (points_call, dict(sigma_only=True)),
    "call_dense_xyz4": (points_call, dict(xyz_dim=4)),
    "call_dense_xyz4_training_mode": (points_call, dict(xyz_dim=4, training=True)),
    "call_sh": (points_call, dict(cfg=SH2)),
    "call_sh_sigma_only": (points_call, dict(cfg=SH2, sigma_only=True)),
    "call_sh_xyz4": (points_call, dict(cfg=SH2, xyz_dim=4)),
    "call_sh_xyz4_sigma_only": (points_call, dict(cfg=SH2, xyz_dim=4, sigma_only=True)),
    "forward_coef": (points_call, dict(cfg=SH2, coef=True)),
    "bg_scene_train_coarse": (bg_scene, dict()),
    "bg_scene_train_fine": (bg_scene, dict(fine=8)),
    "bg_scene_eval_fine": (bg_scene, dict(fine=8, training=False)),
    "mega_call": (mega, dict(call="all")),
    "mega_call_sigma_only": (mega, dict(call="sigma_only")),
    "mega_sh_call": (mega, dict(cfg=CELL_SH, call="all")),
    "mega_sh_call_rgb": (mega, dict(cfg=CELL_SH, call="rgb")),
    "mega_train_coarse": (mega, dict()),
    "mega_train_fine": (mega, dict(fine=4)),
    "mega_sh_train_coarse": (mega, dict(cfg=CELL_SH)),
    "mega_sh_train_fine": (mega, dict(cfg=CELL_SH, fine=4)),
    "noise_grad_step": (noise_step, dict()),
    "noise_grad_step_fine": (noise_step, dict(fine=64)),
    "noise_grad_step_gate_noise": (noise_step, dict(gate_noise=1.0)),
    "noise_hash_grad_step": (noise_step, dict(hash_grid=True)),
    "noise_hash_grad_step_fine": (noise_step, dict(hash_grid=True, fine=64)),
    "noise_train_step_mip": (noise_step, dict(mip=True, fine=64)),
    "noise_scene_train_step": (noise_scene, dict()),
    "noise_scene_train_step_fine": (noise_scene, dict(fine=8)),
    "noise_moe_layer": (noise_moe_layer, dict()),
}
res = {}
for name, (fn, kw) in list((k, (train, v)) for k, v in CASES.items()) + list(MORE_CASES.items()):
    trace.clear()
    ptr_ids.clear()
    _alive.clear()
    try:
        m, ctxs = fn(**kw)
        res[name] = name_ptrs(list(trace), ranges_of(m, ctxs))
    except Exception as e:  # noqa: BLE001
        res[name] = list(trace) + [["ERROR", repr(e)[:300]]]
    print(name, len(res[name]), res[name][-1][0] if res[name] else None, res[name][-1][1] if res[name] and res[name][-1][0] == "ERROR" else "")
json.dump(res, open(out_path, "w"))
