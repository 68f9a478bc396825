"""CPU launch trace of the step's host-side orchestration: every C-ABI call a step makes (entry point, every scalar argument, every
descriptor field; pointers named after the model buffer / context key they fall into, `tmp` otherwise) with the library mocked, so no
GPU is needed.  For host-side refactors: record the trace on two checkouts and compare - equal traces = the same kernels with the same
arguments in the same order.  Not covered: the side-stream sections and the profile hooks (a CPU model has no side stream).

    python scripts/step_launch_trace.py OUT.json [ROOT]     record (ROOT: the checkout whose switch_nerf_amd is traced, default this one)
    python scripts/step_launch_trace.py --diff A.json B.json

A pointer that is `tmp` on one side and a named buffer on the other is a freed temporary whose address a later buffer took, not a
difference in the launch."""
import ctypes as C
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
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(HERE, "tests"))
import synth  # noqa: E402
from switch_nerf_amd import _lib, ops  # noqa: E402

torch.empty = torch.zeros
torch.empty_like = torch.zeros_like
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


def ranges_of(m, ctxs):
    r = []
    def add(t, n):
        if torch.is_tensor(t) and t.numel():
            r.append((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), n))
    for k, t in m._bufs.items():
        for i, x in enumerate(t if isinstance(t, tuple) else (t,)):
            add(x, "buf%r.%d" % (k, i))
    for k, t in m.wf.items():
        add(t, "wf." + k)
    for k, t in m.wb.items():
        add(t, "wb." + k)
    add(m.flat, "flat"); add(m.grad, "grad"); add(m.m, "adam_m"); add(m.v, "adam_v")
    for ci, c in enumerate(ctxs):
        for k, t in c.items():
            if isinstance(t, (list, tuple)):
                for i, x in enumerate(t):
                    add(x, "c%d.%s.%d" % (ci, k, i))
            elif isinstance(t, dict):
                for kk, x in t.items():
                    add(x, "c%d.%s.%s" % (ci, k, kk))
            else:
                add(t, "c%d.%s" % (ci, k))
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


class FakeLib:
    def __getattr__(self, k):
        return lambda *a: 4096


class _S:
    cuda_stream = 0


ops.call = fake_call
ops._stream = lambda: C.c_void_p(0)
def _ptr(t):
    assert t is None or t.is_contiguous()
    return None if t is None else C.c_void_p(t.data_ptr())


ops._p = _ptr
_lib.load = lambda: FakeLib()
ops._lib.load = _lib.load
_sched = torch.zeros(16, dtype=torch.int32)
ops.chain_sched = lambda dev, key: _sched
torch.cuda.current_stream = lambda *a: _S()

_route = ops.route_top1


def fake_route(idx, gmax, gates, seg_tokens, n_experts, capacity, bpr, want_perm=True, want_drops=False, **kw):
    """a consistent routing for the zero-filled mock: every token of a segment goes to expert 0"""
    r = list(_route(idx, gmax, gates, seg_tokens, n_experts, capacity, bpr, want_perm=want_perm, want_drops=want_drops, **kw))
    P = idx.shape[0]
    n_seg = P // seg_tokens
    loc, counts = r[0], r[1]
    loc.copy_(torch.arange(P, dtype=loc.dtype) % seg_tokens)
    counts.zero_()
    counts.view(n_seg, n_experts)[:, 0] = seg_tokens
    if want_drops:
        nd = max(seg_tokens - capacity, 0)
        r[5].copy_((torch.arange(n_seg * n_experts + 1) > 0).to(torch.int32) * 0 + torch.clamp(torch.arange(n_seg * n_experts + 1) + n_experts - 1, min=0) // n_experts * nd)
        tok = torch.arange(P).view(n_seg, seg_tokens)[:, capacity:].reshape(-1).to(torch.int32)
        r[6][: tok.numel()] = tok
    return tuple(r)


ops.route_top1 = fake_route
from switch_nerf_amd.model import SwitchNeRF  # noqa: E402
from switch_nerf_amd.dense import DenseNeRF  # noqa: E402

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
res = {}
for name, kw in CASES.items():
    trace.clear()
    ptr_ids.clear()
    try:
        m, ctxs = train(**kw)
        res[name] = name_ptrs(list(trace), ranges_of(m, ctxs))
    except Exception as e:  # noqa: BLE001
        res[name] = list(trace) + [["ERROR", repr(e)[:300]]]
    print(name, len(res[name]), res[name][-1][0] if res[name] else None, res[name][-1][1] if res[name] and res[name][-1][0] == "ERROR" else "")
json.dump(res, open(out_path, "w"))
