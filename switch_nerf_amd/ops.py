"""Torch-tensor wrappers over the C ABI (include/swn.h).  torch is used for device memory and streams only.

Every function enqueues HIP kernels from libswn_hip.so on torch's current stream.  There is no fallback path.
"""
from __future__ import annotations

import math
import os

import ctypes as C
from typing import List, Optional, Sequence

import torch

from . import _lib
from ._lib import BF16, F16, F32, ChainDesc, WgradItem, WgradJob, call


def _code(dtype) -> int:
    """torch dtype -> dtype code of the C ABI.  The 16-bit type must be the one the selected build of the library computes in
    (_lib.use_half): bfloat16 -> libswn_hip.so, float16 -> libswn_hip_f16.so."""
    if dtype == torch.float32:
        return F32
    if dtype == torch.bfloat16:
        if _lib.half_kind() != "bf16":
            raise RuntimeError("bfloat16 tensor, but the fp16 build of the library is selected (_lib.use_half('bf16') first)")
        return BF16
    if dtype == torch.float16:
        if _lib.half_kind() != "f16":
            raise RuntimeError("float16 tensor, but the bf16 build of the library is selected (_lib.use_half('f16') first)")
        return F16
    raise TypeError(f"unsupported dtype {dtype}")


def _dt(t: torch.Tensor) -> int:
    return _code(t.dtype)


def _p(t: Optional[torch.Tensor]):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "tensors passed to the HIP library must be contiguous device tensors"
    return C.c_void_p(t.data_ptr())


def _pv(t: torch.Tensor):
    """The address of a strided VIEW (the entry point takes its row stride): the caller has checked the layout."""
    assert t.is_cuda
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def torch_dtype(code: int):
    return {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}[code]


def mfma_probe() -> torch.Tensor:
    out = torch.zeros(2048, dtype=torch.int32, device="cuda")
    call("swn_mfma_probe", _p(out), _stream())
    return out


def sample_pe(rays, t_steps, perturb_rand, perturb: float, n_samples: int, l_xyz: int, l_dir: int, dtype,
              pe_stride: int, dir_stride: int):
    """-> z [N,S] f32, pe_xyz [N*S, pe_stride] dtype, pe_dir [N, dir_stride] dtype"""
    n = rays.shape[0]
    z = torch.empty(n, n_samples, dtype=torch.float32, device=rays.device)
    pe = torch.empty(n * n_samples, pe_stride, dtype=dtype, device=rays.device)
    pd = torch.empty(n, dir_stride, dtype=dtype, device=rays.device)
    call("swn_sample_pe", _p(rays), _p(t_steps), _p(perturb_rand), float(perturb), n, n_samples, l_xyz, l_dir, _dt(pe),
         _p(z), _p(pe), pe_stride, _p(pd), dir_stride, _stream())
    return z, pe, pd


# ---- seeded device-side noise (csrc/philox.hpp, csrc/rng.hip): Philox4x32-10 keyed by (seed, step, stream id, global element index).
# The stream ids are fixed (the same table as philox.hpp); element index e of each:
RNG_JITTER = 0          # coarse stratified jitter     (ray_base + n) * S + s
RNG_SIGMA = 1           # coarse sigma noise           (ray_base + n) * R + r, R rows per ray (S; S - 1 intervals for mip)
RNG_FINE_U = 2          # fine-pass u                  (ray_base + n) * F + f
RNG_SIGMA_FINE = 3      # fine sigma noise             as RNG_SIGMA with the fine row count
RNG_GATE = 4            # gate noise                   (ray_base * R + p) * E + e
RNG_ROUTER_NORMAL = 5   # moe.MoELayer's use_normal_noise draw, addressed like RNG_GATE
RNG_UNIFORM, RNG_NORMAL = 0, 1
# Domains (counter word 3 = stream id | (domain << 8)): the draws above are domain 0.  Domain 1 is the background model of a scene
# (background.BackgroundScene): the stream ids 0-3 again, background row j being global ray g = ray_base + idx_bg[j] (its position in the
# batch), Sb / Fb the background's coarse / fine sample counts:
#   RNG_JITTER g * Sb + a (a: ascending sample)   RNG_SIGMA g * Sb + j (j: evaluated row, descending depth)
#   RNG_FINE_U g * Fb + f                          RNG_SIGMA_FINE g * Fb + f
RNG_DOMAIN_FG, RNG_DOMAIN_BG = 0, 1


def rng_check_step(step: int) -> int:
    """The step is the third counter word of the generator: it must fit 32 bits (checked where the host sets it)."""
    step = int(step)
    if not 0 <= step < 1 << 32:
        raise ValueError(f"device noise: step {step} outside [0, 2^32)")
    return step


def rng_step_tensor(step: int, device) -> torch.Tensor:
    """The device int64[1] the kernels read the step from (a captured launch follows it from replay to replay)."""
    return torch.full((1,), rng_check_step(step), dtype=torch.int64, device=device)


def rng_fill(n: int, base: int, kind: int, seed: int, step_dev, stream_id: int, scale: float = 1.0, out=None):
    """-> out [n] f32: out[i] = the draw of element base + i of (seed, step_dev[0], stream_id); RNG_UNIFORM in [0, 1) or
    RNG_NORMAL * scale."""
    assert step_dev.dtype == torch.int64 and step_dev.numel() == 1
    if out is None:
        out = torch.empty(int(n), dtype=torch.float32, device=step_dev.device)
    assert out.dtype == torch.float32 and out.numel() == int(n)
    call("swn_rng_fill", _p(out), int(n), int(base), int(kind), float(scale), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(step_dev), int(stream_id),
         _stream())
    return out


def _row_index_arg(row_index, n_rows: int, index_limit):
    """row_index (int64 [n_rows] device tensor or None = identity) and the exclusive bound of its entries the library checks the element
    index's overflow with (the entries address the generator only, never memory)."""
    if row_index is None:
        return None, max(int(index_limit or 0), int(n_rows))
    assert row_index.dtype == torch.int64 and row_index.numel() == int(n_rows)
    if index_limit is None:
        raise ValueError("row_index needs index_limit (an exclusive upper bound of its entries, e.g. the rays of the batch)")
    return row_index, int(index_limit)


def rng_fill_rows(n_rows: int, per_row: int, row_base: int, row_index, kind: int, seed: int, step_dev, stream_id: int,
                  domain: int = RNG_DOMAIN_FG, scale: float = 1.0, index_limit=None, out=None):
    """-> out [n_rows, per_row] f32: out[j, s] = the draw of element (row_base + row_index[j]) * per_row + s of (seed, step_dev[0],
    stream_id, domain).  row_index: int64 [n_rows] (unsorted, repeats allowed, entries in [0, index_limit)) or None = the identity."""
    assert step_dev.dtype == torch.int64 and step_dev.numel() == 1
    n_rows, per_row = int(n_rows), int(per_row)
    row_index, limit = _row_index_arg(row_index, n_rows, index_limit)
    if out is None:
        out = torch.empty(max(n_rows, 0), max(per_row, 0), dtype=torch.float32, device=step_dev.device)
    assert out.dtype == torch.float32 and out.numel() == n_rows * per_row
    call("swn_rng_fill_rows", _p(out), n_rows, per_row, int(row_base), _p(row_index), limit, int(kind), float(scale),
         int(seed) & 0xFFFFFFFFFFFFFFFF, _p(step_dev), int(stream_id), int(domain), _stream())
    return out


def rng_advance(step_dev):
    """step_dev[0] += 1 on the device (one launch: the last one of a training step, inside a captured step)."""
    assert step_dev.dtype == torch.int64 and step_dev.numel() == 1
    call("swn_rng_advance", _p(step_dev), _stream())


def sample_pe_rng(rays, t_steps, seed: int, step_dev, ray_base: int, perturb: float, n_samples: int, l_xyz: int, l_dir: int, dtype,
                  pe_stride: int, dir_stride: int):
    """sample_pe with the jitter (stream RNG_JITTER) drawn inside the kernel: no [N,S] noise buffer.
    -> z [N,S] f32, pe_xyz [N*S, pe_stride] dtype, pe_dir [N, dir_stride] dtype"""
    n = rays.shape[0]
    z = torch.empty(n, n_samples, dtype=torch.float32, device=rays.device)
    pe = torch.empty(n * n_samples, pe_stride, dtype=dtype, device=rays.device)
    pd = torch.empty(n, dir_stride, dtype=dtype, device=rays.device)
    call("swn_sample_pe_rng", _p(rays), _p(t_steps), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(step_dev), int(ray_base), float(perturb), n,
         n_samples, l_xyz, l_dir, _dt(pe), _p(z), _p(pe), pe_stride, _p(pd), dir_stride, _stream())
    return z, pe, pd


def pe_from_z(rays, z, l_xyz: int, dtype, pe_stride: int):
    n, S = z.shape
    pe = torch.empty(n * S, pe_stride, dtype=dtype, device=rays.device)
    call("swn_pe_from_z", _p(rays), _p(z), n, S, l_xyz, _dt(pe), _p(pe), pe_stride, _stream())
    return pe


def sample_pdf(z_coarse, weights, u, n_fine: int):
    n, S = z_coarse.shape
    zf = torch.empty(n, n_fine, dtype=torch.float32, device=z_coarse.device)
    call("swn_sample_pdf", _p(z_coarse), _p(weights), _p(u), n, S, n_fine, _p(zf), _stream())
    return zf


def cascade_resample(z_coarse, weights, u, n_fine: int, want_z_fine=False):
    """The cascade's fine depths in one launch (swn_cascade_resample) -> (z_union [N, S+F], z_fine [N, F] or None)."""
    n, S = z_coarse.shape
    dev = z_coarse.device
    zu = torch.empty(n, S + n_fine, dtype=torch.float32, device=dev)
    zf = torch.empty(n, n_fine, dtype=torch.float32, device=dev) if want_z_fine else None
    call("swn_cascade_resample", _p(z_coarse), _p(weights), _p(u), n, S, n_fine, _p(zu), _p(zf), _stream())
    return zu, zf


def merge_samples(z_fine, z_coarse, raw_fine, raw_coarse):
    n, F = z_fine.shape
    S = z_coarse.shape[1]
    dev = z_fine.device
    z = torch.empty(n, F + S, dtype=torch.float32, device=dev)
    order = torch.empty(n, F + S, dtype=torch.int32, device=dev)
    raw = torch.empty(n * (F + S), 4, dtype=torch.float32, device=dev)
    call("swn_merge_samples", _p(z_fine), _p(z_coarse), _p(raw_fine), _p(raw_coarse), n, F, S, _p(z), _p(order), _p(raw), _stream())
    return z, order, raw


def unmerge_grad(d_raw, order, n_fine: int, n_coarse: int):
    n = order.shape[0]
    dev = d_raw.device
    d_fine = torch.empty(n * n_fine, 4, dtype=torch.float32, device=dev)
    d_coarse = torch.empty(n * n_coarse, 4, dtype=torch.float32, device=dev)
    call("swn_unmerge_grad", _p(d_raw), _p(order), n, n_fine, n_coarse, _p(d_fine), _p(d_coarse), _stream())
    return d_fine, d_coarse


def sign_bits_pack(h):
    """[rows, F] 16-bit -> int32 [rows, F / 32]: bit j of word q = (h[:, 32 q + j] > 0) (include/swn.h swn_sign_bits_pack)."""
    assert h.dim() == 2 and h.is_contiguous() and h.element_size() == 2 and h.shape[1] % 32 == 0
    bits = torch.empty(h.shape[0], h.shape[1] // 32, dtype=torch.int32, device=h.device)
    call("swn_sign_bits_pack", _p(h), int(h.shape[0]), int(h.shape[1]), _p(bits), _stream())
    return bits


def sign_bits_unpack(bits, dtype):
    """int32 [rows, W] -> [rows, 32 W] of `dtype` (the library's 16-bit type): 1 where the bit is set, else 0."""
    assert bits.dim() == 2 and bits.is_contiguous() and bits.dtype == torch.int32
    h = torch.empty(bits.shape[0], bits.shape[1] * 32, dtype=dtype, device=bits.device)
    call("swn_sign_bits_unpack", _p(bits), int(bits.shape[0]), int(h.shape[1]), _p(h), _stream())
    return h


def gather_rows(src, index, out=None):
    """out[r] = src[index[r]] (zero rows for index < 0); src [*, C] row-major, index int32 [R]."""
    R, Cc = index.numel(), src.shape[1]
    if out is None:
        out = torch.empty(R, Cc, dtype=src.dtype, device=src.device)
    if R == 0:
        return out
    call("swn_gather_rows", _p(src), _p(index), R, Cc * src.element_size(), _p(out), _stream())
    return out


def scatter_rows(src, index, out):
    """out[index[r]] = src[r] (index < 0: nowhere; no index twice); src [R, C] row-major, index int32 [R], out [*, C] (include/swn.h
    swn_scatter_rows)."""
    R = index.numel()
    assert src.is_contiguous() and out.is_contiguous() and index.dtype == torch.int32 and src.shape[0] >= R and src.dtype == out.dtype
    rb = (src.numel() // max(1, src.shape[0])) * src.element_size()
    assert rb == (out.numel() // max(1, out.shape[0])) * out.element_size()
    if R:
        call("swn_scatter_rows", _p(src), _p(index), R, rb, _p(out), _stream())
    return out


def owner_aux(gate, noise, index, rows_per_ray: int, ray_base: int, out, zero_gate: bool = False):
    """out[r] = (gate[t], bits of (t // rows_per_ray + ray_base), noise[t] or 0, 0), t = index[r] (include/swn.h swn_owner_aux)."""
    n = index.numel()
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape[0] >= n and out.shape[1] == 4 and index.dtype == torch.int32
    if n:
        call("swn_owner_aux", _p(gate), _p(noise), _p(index), n, int(rows_per_ray), int(ray_base), int(bool(zero_gate)), _p(out), _stream())
    return out


def owner_aux_split(aux, gate, ray, noise=None):
    """aux [n, 4] -> gate [n] f32, ray [n] int32, noise [n] f32 (or None) (include/swn.h swn_owner_aux_split)."""
    n = aux.shape[0]
    assert aux.dtype == torch.float32 and aux.is_contiguous() and gate.numel() >= n and ray.numel() >= n and ray.dtype == torch.int32
    if n:
        call("swn_owner_aux_split", _p(aux), n, _p(gate), _p(ray), _p(noise), _stream())


def ray_bias_grad_bits(bits, raw, d_raw, w_color, rows_per_ray: int):
    """-> dc_ray [P / rows_per_ray, 32 W] f32: the per-ray sums of dh2 from the sign bits of h2 (include/swn.h swn_ray_bias_grad_bits)."""
    P, W = bits.shape
    assert bits.dtype == torch.int32 and raw.shape == (P, 4) and d_raw.shape == (P, 4) and P % rows_per_ray == 0 and w_color.shape == (3, 32 * W)
    out = torch.empty(P // rows_per_ray, 32 * W, dtype=torch.float32, device=bits.device)
    call("swn_ray_bias_grad_bits", _p(bits), _p(raw), _p(d_raw), _p(w_color), P // rows_per_ray, int(rows_per_ray), 32 * W, _p(out), _stream())
    return out


def gate_fwd(g, ln_w, ln_b, wg, noise=None, noise_scale: float = 0.0):
    """LayerNorm + fp32 router + softmax + top-1 -> (gates [P, E], idx, gmax, stats).  noise [P, E] fp32: logits += noise_scale * noise
    before the softmax (the gate-noise branch of a training forward, swn_gate_fwd_noise)."""
    P, G = g.shape
    E = wg.shape[0]
    dev = g.device
    gates = torch.empty(P, E, dtype=torch.float32, device=dev)
    idx = torch.empty(P, dtype=torch.int32, device=dev)
    gmax = torch.empty(P, dtype=torch.float32, device=dev)
    stats = torch.empty(P, 2, dtype=torch.float32, device=dev)
    if noise is not None:
        assert noise.shape == (P, E) and noise.dtype == torch.float32
        call("swn_gate_fwd_noise", _p(g), _dt(g), _p(ln_w), _p(ln_b), _p(wg), _p(noise.contiguous()), float(noise_scale), P, G, E, _p(gates),
             _p(idx), _p(gmax), _p(stats), _stream())
    else:
        call("swn_gate_fwd", _p(g), _dt(g), _p(ln_w), _p(ln_b), _p(wg), P, G, E, _p(gates), _p(idx), _p(gmax), _p(stats), _stream())
    return gates, idx, gmax, stats


def gate_bwd(g, ln_w, ln_b, wg, gates, idx, d_gmax, stats, counts, laux_coef, seg_tokens, d_wg, d_ln_w, d_ln_b):
    """Accumulates into d_wg / d_ln_w / d_ln_b (fp32), returns dg."""
    P, G = g.shape
    E = wg.shape[0]
    dg = torch.empty_like(g)
    dlogits = torch.empty(int(_lib.load().swn_gate_bwd_scratch_floats(P, G, E)), dtype=torch.float32, device=g.device)
    call("swn_gate_bwd", _p(g), _dt(g), _p(ln_w), _p(ln_b), _p(wg), _p(gates), _p(idx), _p(d_gmax), _p(stats), _p(counts),
         _p(laux_coef), int(seg_tokens), P, G, E, _p(dg), _p(dlogits), _p(d_wg), _p(d_ln_w), _p(d_ln_b), _stream())
    return dg


def gate_bwd_dense(g, ln_w, ln_b, wg, gates, idx, d_gmax, d_probs, stats, counts, laux_coef, seg_tokens, d_wg, d_ln_w, d_ln_b,
                   d_logits_add=None):
    """gate_bwd with dense operands on top (swn_gate_bwd_dense): d_probs [P, E] w.r.t. the probabilities (top-k layers), d_logits_add
    [P, E] w.r.t. the logits, added behind the softmax backward (load / importance loss)."""
    P, G = g.shape
    E = wg.shape[0]
    for t in (d_probs, d_logits_add):
        assert t is None or (t.shape == (P, E) and t.dtype == torch.float32 and t.is_contiguous())
    dg = torch.empty_like(g)
    dlogits = torch.empty(int(_lib.load().swn_gate_bwd_scratch_floats(P, G, E)), dtype=torch.float32, device=g.device)
    call("swn_gate_bwd_dense", _p(g), _dt(g), _p(ln_w), _p(ln_b), _p(wg), _p(gates), _p(idx), _p(d_gmax), _p(d_probs), _p(d_logits_add),
         _p(stats), _p(counts), _p(laux_coef), int(seg_tokens), P, G, E, _p(dg), _p(dlogits), _p(d_wg), _p(d_ln_w), _p(d_ln_b), _stream())
    return dg


def gate_logits(g, wg, noise=None, noise_scale: float = 0.0, out=None):
    """The fp32 router's logits g @ wg^T (+ noise_scale * noise) [P, E] (swn_gate_logits; no LayerNorm); out: the fp32 [P, E] buffer to fill."""
    P, G = g.shape
    E = wg.shape[0]
    logits = torch.empty(P, E, dtype=torch.float32, device=g.device) if out is None else out
    assert logits.shape == (P, E) and logits.dtype == torch.float32
    call("swn_gate_logits", _p(g), _dt(g), _p(wg), _p(noise), float(noise_scale), P, G, E, _p(logits), _stream())
    return logits


def load_importance_fwd(scores_wo_noise, logits_w_noise, idx_last, sigma: float):
    """load_importance_loss (tutel_fast_dispatch.py:152-174) -> (l_loss [1], coef [2 E] for the backward)."""
    P, E = scores_wo_noise.shape
    dev = scores_wo_noise.device
    l = torch.empty(1, dtype=torch.float32, device=dev)
    coef = torch.empty(2 * E, dtype=torch.float32, device=dev)
    ws = torch.empty(int(_lib.load().swn_load_importance_workspace_floats(P, E)), dtype=torch.float32, device=dev)
    call("swn_load_importance_fwd", _p(scores_wo_noise), _p(logits_w_noise), _p(idx_last), float(sigma), P, E, _p(l), _p(coef), _p(ws), _stream())
    return l, coef


def load_importance_bwd(scores_wo_noise, logits_w_noise, idx_last, coef, d_l, sigma: float):
    """-> d_logits [P, E] of the loss, times the device scalar d_l [1]."""
    P, E = scores_wo_noise.shape
    d_logits = torch.empty(P, E, dtype=torch.float32, device=scores_wo_noise.device)
    call("swn_load_importance_bwd", _p(scores_wo_noise), _p(logits_w_noise), _p(idx_last), _p(coef), _p(d_l), float(sigma), P, E, _p(d_logits),
         _stream())
    return d_logits


def topk_select(gates, k: int):
    """torch.topk(gates, k, dim=1) + the normalised gates of a top-k layer (tutel_fast_dispatch.py:177-182, 204-206)
    -> (idx int32 [k, P], gsel fp32 [k, P], gnorm fp32 [k, P])."""
    P, E = gates.shape
    dev = gates.device
    idx = torch.empty(k, P, dtype=torch.int32, device=dev)
    gsel = torch.empty(k, P, dtype=torch.float32, device=dev)
    gnorm = torch.empty(k, P, dtype=torch.float32, device=dev)
    call("swn_topk_select", _p(gates), P, E, int(k), _p(idx), _p(gsel), _p(gnorm), _stream())
    return idx, gsel, gnorm


def topk_gate_bwd(gates, idx, d_gnorm):
    """Backward of topk_select's normalisation: d_gnorm [k, P] -> d_probs [P, E]."""
    P, E = gates.shape
    k = idx.shape[0]
    d_probs = torch.empty(P, E, dtype=torch.float32, device=gates.device)
    call("swn_topk_gate_bwd", _p(gates), _p(idx), _p(d_gnorm.contiguous()), P, E, int(k), _p(d_probs), _stream())
    return d_probs


def route_topk(idx, gmax, gates, seg_tokens: int, n_experts: int, capacity: int, bpr: bool, want_tok2row=False):
    """Capacity assignment of a top-k routing (swn_route_topk; idx [k, P] from topk_select, gmax [P] the tokens' top-1 gates)
    -> (loc [k, P], counts [k, n_seg, E], perm [n_seg, E * capacity], tok2row [k, P] or None, group_rows [n_seg * E], l_aux [n_seg])."""
    k, P = idx.shape
    n_seg = P // seg_tokens
    dev = idx.device
    loc = torch.empty(k, P, dtype=torch.int32, device=dev)
    counts = torch.empty(k, n_seg, n_experts, dtype=torch.int32, device=dev)
    perm = torch.empty(n_seg, n_experts * capacity, dtype=torch.int32, device=dev)
    tok2row = torch.empty(k, P, dtype=torch.int32, device=dev) if want_tok2row else None
    group_rows = torch.empty(n_seg * n_experts, dtype=torch.int32, device=dev)
    l_aux = torch.empty(n_seg, dtype=torch.float32, device=dev) if gates is not None else None
    nbytes = _lib.load().swn_route_workspace_bytes(P, n_seg, n_experts)
    key = (dev, nbytes)
    ws = _route_ws.get(key)
    if ws is None:
        ws = _route_ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    call("swn_route_topk", _p(idx), _p(gmax), _p(gates), P, int(seg_tokens), int(n_experts), int(capacity), int(bool(bpr)), int(k),
         _p(loc), _p(counts), _p(perm), _p(tok2row), _p(group_rows), _p(l_aux), _p(ws), nbytes, _stream())
    return loc, counts, perm, tok2row, group_rows, l_aux


_route_ws = {}


_route_sync = {}


def route_sync(dev):
    """The synchronisation words of the one-launch routing (swn_route_top1x): zero at creation, left zero by every launch; one per
    (device, stream) - routings on one stream are ordered, routings that may overlap get their own.  Never freed (graphs)."""
    k = (dev, torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0)
    t = _route_sync.get(k)
    if t is None:
        t = _route_sync[k] = torch.zeros(int(_lib.load().swn_route_sync_bytes()) // 4, dtype=torch.int32, device=dev)
    return t


_ROUTE_MODE = int(os.environ.get("SWN_ROUTE_MODE", "0"))            # (experiment build only: see route_top1)
CHAINQ_STATIC = os.environ.get("SWN_CHAINQ_STATIC") is not None       # persistent chains without tile queues (tests assign it)


def route_top1(idx, gmax, gates, seg_tokens: int, n_experts: int, capacity: int, bpr: bool, want_perm=True, want_drops=False, multi=False,
               mode=None):
    """Top-1 capacity assignment of every routing segment (swn_route_top1x) -> (loc, counts, perm, tok2row, l_aux)
    [+ (drop_begin, dropped) with want_drops: the tokens no expert kept, swn_route_dropped's lists, from the same call].
    mode (include/swn.h): 0 = the 20 per-phase kernels (the product library's only mode); 1 / 2 = the fused forms of round 5, in the
    experiment build only (scripts/experiments/build_route_one.sh; SWN_ROUTE_MODE, read once at import, selects them there).
    multi=True: the round 1-4 entry points themselves (swn_route_top1 + swn_route_dropped) - the twin the tests compare with."""
    P = idx.shape[0]
    n_seg = P // seg_tokens
    dev = idx.device
    loc = torch.empty(P, dtype=torch.int32, device=dev)
    counts = torch.empty(n_seg, n_experts, dtype=torch.int32, device=dev)
    perm = torch.empty(n_seg, n_experts * capacity, dtype=torch.int32, device=dev) if want_perm else None
    tok2row = torch.empty(P, dtype=torch.int32, device=dev)
    l_aux = torch.empty(n_seg, dtype=torch.float32, device=dev) if gates is not None else None
    drop_begin = torch.empty(n_seg * n_experts + 1, dtype=torch.int32, device=dev) if want_drops else None
    dropped = torch.empty(P, dtype=torch.int32, device=dev) if want_drops else None
    nbytes = _lib.load().swn_route_workspace_bytes(P, n_seg, n_experts)
    key = (dev, nbytes)
    ws = _route_ws.get(key)
    if ws is None:      # one workspace per size, kept for good: a captured hipGraph may hold its address (coarse / fine passes alternate
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)      # two sizes; a size follows the batch shape: a handful per process)
        _route_ws[key] = ws
    if multi:
        call("swn_route_top1", _p(idx), _p(gmax), _p(gates), P, int(seg_tokens), n_experts, int(capacity), int(bool(bpr)),
             _p(loc), _p(counts), _p(perm), _p(tok2row), _p(l_aux), _p(ws), nbytes, _stream())
        if want_drops:
            call("swn_route_dropped", _p(idx), _p(loc), _p(counts), P, int(seg_tokens), int(n_experts), int(capacity), _p(drop_begin),
                 _p(dropped), _stream())
    else:
        call("swn_route_top1x", _p(idx), _p(gmax), _p(gates), P, int(seg_tokens), n_experts, int(capacity), int(bool(bpr)),
             _p(loc), _p(counts), _p(perm), _p(tok2row), _p(l_aux), _p(drop_begin), _p(dropped),
             _p(route_sync(dev)), int(_ROUTE_MODE if mode is None else mode), _p(ws), nbytes, _stream())
    if want_drops:
        return loc, counts, perm, tok2row, l_aux, drop_begin, dropped
    return loc, counts, perm, tok2row, l_aux


def route_top1_packed(idx, gmax, gates, seg_tokens: int, n_experts: int, bpr: bool):
    """Top-1 routing without dropping, straight into the packed row space (swn_route_top1_packed: capacity_factor = 0 in training)
    -> (loc, counts, begin [n_seg * E], perm [P] row -> token, tok2row [P], l_aux).  loc / counts / l_aux equal route_top1's bit for
    bit; begin / perm / tok2row equal route_pack's of that routing."""
    P = idx.shape[0]
    n_seg = P // seg_tokens
    dev = idx.device
    loc = torch.empty(P, dtype=torch.int32, device=dev)
    counts = torch.empty(n_seg, n_experts, dtype=torch.int32, device=dev)
    begin = torch.empty(n_seg * n_experts, dtype=torch.int32, device=dev)
    perm = torch.empty(P, dtype=torch.int32, device=dev)
    tok2row = torch.empty(P, dtype=torch.int32, device=dev)
    l_aux = torch.empty(n_seg, dtype=torch.float32, device=dev) if gates is not None else None
    nbytes = _lib.load().swn_route_workspace_bytes(P, n_seg, n_experts)
    key = (dev, nbytes)
    ws = _route_ws.get(key)
    if ws is None:      # (kept for good, like route_top1's)
        ws = _route_ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    call("swn_route_top1_packed", _p(idx), _p(gmax), _p(gates), P, int(seg_tokens), int(n_experts), int(bool(bpr)), _p(loc), _p(counts),
         _p(begin), _p(perm), _p(tok2row), _p(l_aux), _p(ws), nbytes, _stream())
    return loc, counts, begin, perm, tok2row, l_aux


def route_dropped(idx, loc, counts, seg_tokens: int, n_experts: int, capacity: int):
    """-> (drop_begin int32 [n_groups + 1], dropped int32 [P]): the tokens no expert kept, per (segment, expert) in location order;
    drop_begin[-1] = their number (a device scalar: nothing is read on the host).  Input of the fused tail (mlp_chain(tail=...))."""
    P = idx.shape[0]
    n_groups = (P // seg_tokens) * n_experts
    drop_begin = torch.empty(n_groups + 1, dtype=torch.int32, device=idx.device)
    dropped = torch.empty(P, dtype=torch.int32, device=idx.device)
    call("swn_route_dropped", _p(idx), _p(loc), _p(counts), P, int(seg_tokens), int(n_experts), int(capacity), _p(drop_begin), _p(dropped),
         _stream())
    return drop_begin, dropped


def dispatch_fwd(gates, indices, locations, x, n_experts: int, capacity: int):
    S, H = x.shape
    d = torch.empty(n_experts * capacity, H, dtype=x.dtype, device=x.device)
    call("swn_dispatch_fwd", _p(gates), _p(indices), _p(locations), _p(x), _p(d), _dt(x), S, H, capacity, n_experts, _stream())
    return d


def dispatch_bwd_data(gates, indices, locations, dispatched, capacity: int):
    S = indices.shape[0]
    H = dispatched.shape[1]
    out = torch.empty(S, H, dtype=dispatched.dtype, device=dispatched.device)
    call("swn_dispatch_bwd_data", _p(gates), _p(indices), _p(locations), _p(out), _p(dispatched), _dt(out), S, H, capacity, _stream())
    return out


def dispatch_fwd_more(gates, indices, locations, x, dispatched, n_experts: int, capacity: int):
    """A further choice's rows into an existing dispatched buffer (top-k: tutel_fast_dispatch.py:26-27, later iterations)."""
    S, H = x.shape
    call("swn_dispatch_fwd_more", _p(gates), _p(indices), _p(locations), _p(x), _p(dispatched), _dt(x), S, H, capacity, n_experts, _stream())
    return dispatched


def dispatch_bwd_data_more(gates, indices, locations, out, dispatched, capacity: int):
    """out[i] += g * dispatched[row] (top-k: `last_result + ...`, tutel_fast_dispatch.py:37, :62)."""
    S = indices.shape[0]
    H = dispatched.shape[1]
    call("swn_dispatch_bwd_data_more", _p(gates), _p(indices), _p(locations), _p(out), _p(dispatched), _dt(out), S, H, capacity, _stream())
    return out


def dispatch_bwd_gate(indices, locations, x, dispatched, capacity: int):
    S, H = x.shape
    gg = torch.empty(S, dtype=torch.float32, device=x.device)
    call("swn_dispatch_bwd_gate", _p(gg), _p(indices), _p(locations), _p(x), _p(dispatched), _dt(x), S, H, capacity, _stream())
    return gg


def dispatch_nobatch_fwd(gates, indices, locations, expert_locations_begin, x, dispatched_rows: int, capacity: int = 0):
    """The no-batch encode kernel (tutel_fast_dispatch_nobatch.py:36): D[begin[idx] + loc] = g * x, rows packed per expert."""
    S, H = x.shape
    E = expert_locations_begin.numel()
    d = torch.empty(int(dispatched_rows), H, dtype=x.dtype, device=x.device)
    call("swn_dispatch_nobatch_fwd", _p(gates), _p(indices), _p(locations), _p(expert_locations_begin), _p(x), _p(d), _dt(x), S, H,
         int(capacity), E, int(dispatched_rows), _stream())
    return d


def dispatch_nobatch_bwd_data(gates, indices, locations, expert_locations_begin, dispatched, capacity: int = 0):
    """... :47 / :73 (also the decode forward): out[i] = g * D[begin[idx] + loc], zero rows for idx < 0."""
    S, H = indices.shape[0], dispatched.shape[1]
    out = torch.empty(S, H, dtype=dispatched.dtype, device=dispatched.device)
    call("swn_dispatch_nobatch_bwd_data", _p(gates), _p(indices), _p(locations), _p(expert_locations_begin), _p(out), _p(dispatched),
         _dt(out), S, H, int(capacity), expert_locations_begin.numel(), _stream())
    return out


def dispatch_nobatch_bwd_gate(indices, locations, expert_locations_begin, x, dispatched, capacity: int = 0):
    """... :53 / :93: dgate[i] = <D[begin[idx] + loc], x[i]>."""
    S, H = x.shape
    gg = torch.empty(S, dtype=torch.float32, device=x.device)
    call("swn_dispatch_nobatch_bwd_gate", _p(gg), _p(indices), _p(locations), _p(expert_locations_begin), _p(x), _p(dispatched), _dt(x),
         S, H, int(capacity), expert_locations_begin.numel(), _stream())
    return gg


def route_pack(idx, loc, counts, seg_tokens: int, n_experts: int):
    """Packed (no-batch) row space of a routing -> begin [n_seg * E] (expert_locations_begin per segment), perm [P] row -> token,
    tok2row [P] token -> row."""
    P = idx.shape[0]
    n_groups = (P // seg_tokens) * n_experts
    begin = torch.empty(n_groups, dtype=torch.int32, device=idx.device)
    perm = torch.empty(P, dtype=torch.int32, device=idx.device)
    tok2row = torch.empty(P, dtype=torch.int32, device=idx.device)
    call("swn_route_pack", _p(idx), _p(loc), _p(counts), P, int(seg_tokens), int(n_experts), _p(begin), _p(perm), _p(tok2row), _stream())
    return begin, perm, tok2row


def combine_fwd(gates, indices, locations, expert_out, capacity: int, seg_tokens: int, n_experts: int, relu: bool):
    S = indices.shape[0]
    H = expert_out.shape[1]
    y = torch.empty(S, H, dtype=expert_out.dtype, device=expert_out.device)
    call("swn_combine_fwd", _p(gates), _p(indices), _p(locations), _p(y), _p(expert_out), _dt(y), S, H, capacity,
         int(seg_tokens), n_experts, int(bool(relu)), _stream())
    return y


def combine_bwd(dy_in, y, dsig, wsig, gate):
    S, H = y.shape
    dout = torch.empty_like(y)
    dgate = torch.empty(S, dtype=torch.float32, device=y.device)
    call("swn_combine_bwd", _p(dy_in), _p(y), _p(dsig), _p(wsig), _p(gate), _dt(y), S, H, _p(dout), _p(dgate), _stream())
    return dout, dgate


def residual_mix_fwd(x, y_moe, y_res, wc, bc):
    """The residual-expert mix (swn_residual_mix_fwd): x / y_moe / y_res [P, M] in one dtype, wc [2, M] / bc [2] f32 ->
    (y [P, M] in that dtype, coef [P, 2] f32 = softmax(x wc^T + bc))."""
    P, M = x.shape
    assert y_moe.shape == x.shape and y_res.shape == x.shape and y_moe.dtype == x.dtype and y_res.dtype == x.dtype
    assert wc.dtype == torch.float32 and bc.dtype == torch.float32 and wc.shape == (2, M) and bc.numel() == 2
    y = torch.empty_like(x)
    coef = torch.empty(P, 2, dtype=torch.float32, device=x.device)
    call("swn_residual_mix_fwd", _p(x), _p(y_moe), _p(y_res), _p(wc), _p(bc), _dt(x), P, M, _p(y), _p(coef), _stream())
    return y, coef


def residual_mix_bwd(dy, x, y_moe, y_res, coef, wc):
    """Backward of residual_mix_fwd (swn_residual_mix_bwd) -> (d_moe, d_res, dx) in x's dtype, d_wc [2, M] and d_bc [2] f32 (ordered
    per-block sums: the same bits on every launch)."""
    P, M = x.shape
    assert all(t.shape == x.shape and t.dtype == x.dtype for t in (dy, y_moe, y_res)) and coef.shape == (P, 2)
    nb = C.c_size_t(0)
    call("swn_residual_mix_workspace_bytes", _dt(x), P, M, C.byref(nb))
    ws = torch.empty(max(int(nb.value), 4) // 4, dtype=torch.float32, device=x.device)
    d_moe, d_res, dx = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    d_wc = torch.empty(2, M, dtype=torch.float32, device=x.device)
    d_bc = torch.empty(2, dtype=torch.float32, device=x.device)
    call("swn_residual_mix_bwd", _p(dy), _p(x), _p(y_moe), _p(y_res), _p(coef), _p(wc), _dt(x), P, M, _p(d_moe), _p(d_res), _p(dx),
         _p(d_wc), _p(d_bc), _p(ws), ws.numel() * 4, _stream())
    return d_moe, d_res, dx, d_wc, d_bc


def heads_fwd(y, h2, w_sigma, b_sigma, w_color, b_color, sigma_noise):
    P, M = y.shape
    H2 = h2.shape[1]
    raw = torch.empty(P, 4, dtype=torch.float32, device=y.device)
    call("swn_heads_fwd", _p(y), _p(h2), _dt(y), _p(w_sigma), _p(b_sigma), _p(w_color), _p(b_color), _p(sigma_noise), P, M, H2,
         _p(raw), _stream())
    return raw


def heads_bwd(y, h2, w_color, raw, d_raw, d_w_sigma, d_b_sigma, d_w_color, d_b_color, rows_per_group: int = 0):
    """-> (dh2, dsig) or, with rows_per_group > 0 (the samples per ray, dividing P), (dh2, dsig, colsum [P / rows_per_group, H2] f32 =
    group_colsum(dh2, rows_per_group) from the same launch)."""
    P, H2 = h2.shape
    M = d_w_sigma.numel()          # (y may be None: the sigma weight gradient comes from the fused backward chain, mlp_chain(combine=(..., dws)))
    dh2 = torch.empty_like(h2)
    dsig = torch.empty(P, dtype=torch.float32, device=h2.device)
    nb = int(_lib.load().swn_heads_bwd_workspace_bytes(int(P), int(M), int(H2)))
    ws = torch.empty(max(nb, 4) // 4, dtype=torch.float32, device=h2.device)     # block partial sums (added in a fixed order)
    cs = torch.empty(P // rows_per_group, H2, dtype=torch.float32, device=h2.device) if rows_per_group else None
    call("swn_heads_bwd", _p(y), _p(h2), _dt(h2), _p(w_color), _p(raw), _p(d_raw), P, M, H2, _p(dh2), _p(dsig), _p(d_w_sigma),
         _p(d_b_sigma), _p(d_w_color), _p(d_b_color), int(rows_per_group), _p(cs), _p(ws), nb, _stream())
    return (dh2, dsig, cs) if rows_per_group else (dh2, dsig)


def group_colsum(x, rows_per_group: int):
    R, Cc = x.shape
    g = R // rows_per_group
    out = torch.empty(g, Cc, dtype=torch.float32, device=x.device)
    call("swn_group_colsum", _p(x), _dt(x), g, rows_per_group, Cc, _p(out), _stream())
    return out


def _idx_arg(image_indices):
    assert image_indices.dtype in (torch.int32, torch.int64) and image_indices.is_contiguous()
    return _p(image_indices), int(image_indices.dtype == torch.int64)


def ray_feat_fwd(pe_dir, in_dir: int, emb, image_indices, w2r, b2):
    """-> feat [N, in_dir + app_dim] f32, c_ray [N, h2] f32 (include/swn.h swn_ray_feat_fwd)."""
    N, h2, app = pe_dir.shape[0], w2r.shape[1], emb.shape[1]
    feat = torch.empty(N, in_dir + app, dtype=torch.float32, device=pe_dir.device)
    c_ray = torch.empty(N, h2, dtype=torch.float32, device=pe_dir.device)
    ip, i64 = _idx_arg(image_indices)
    call("swn_ray_feat_fwd", _p(pe_dir), _dt(pe_dir), pe_dir.shape[1], int(in_dir), _p(emb), app, ip, i64, _p(w2r), _p(b2), N, h2,
         _p(feat), _p(c_ray), _stream())
    return feat, c_ray


def emb_grad(d_feat, image_indices, d_emb):
    """d_emb[image_indices[n]] += d_feat[n], rays in ascending order with a fixed association (deterministic nn.Embedding backward)."""
    assert d_feat.dtype == torch.float32 and d_emb.dtype == torch.float32 and d_feat.stride(1) == 1 and d_emb.is_contiguous()
    ip, i64 = _idx_arg(image_indices)
    call("swn_emb_grad", _p(d_feat), d_feat.stride(0), ip, i64, d_feat.shape[0], d_feat.shape[1], d_emb.shape[0], _p(d_emb), _stream())


def ray_feat_wgrad(feat, dc_ray, d_w2r, d_b2):
    """d_w2r [F, H2] += feat^T dc_ray, d_b2 [H2] += dc_ray.sum(0) (fp32): block partial sums added in a fixed order, one launch + reduce."""
    N, F = feat.shape
    H2 = dc_ray.shape[1]
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (feat, dc_ray, d_w2r, d_b2)) and dc_ray.shape[0] == N
    assert d_w2r.numel() == F * H2 and d_b2.numel() == H2
    nb = int(_lib.load().swn_ray_feat_wgrad_workspace_bytes(int(N), int(F), int(H2)))
    ws = torch.empty(max(nb, 4) // 4, dtype=torch.float32, device=feat.device)
    call("swn_ray_feat_wgrad", _p(feat), _p(dc_ray), N, F, H2, _p(d_w2r), _p(d_b2), _p(ws), nb, _stream())


def ray_feat_dir_fwd(pe_dir, in_dir: int, emb, image_indices, w2r, b2):
    """swn_ray_feat_fwd with NO embedding columns (affine_appearance: layer "2" sees the direction encoding only) ->
    feat [N, in_dir] f32, c_ray [N, h2] f32."""
    N, h2 = pe_dir.shape[0], w2r.shape[1]
    assert w2r.shape[0] == in_dir
    feat = torch.empty(N, in_dir, dtype=torch.float32, device=pe_dir.device)
    c_ray = torch.empty(N, h2, dtype=torch.float32, device=pe_dir.device)
    ip, i64 = _idx_arg(image_indices)
    call("swn_ray_feat_fwd", _p(pe_dir), _dt(pe_dir), pe_dir.shape[1], int(in_dir), _p(emb), 0, ip, i64, _p(w2r), _p(b2), N, h2,
         _p(feat), _p(c_ray), _stream())
    return feat, c_ray


def affine_ray_fwd(emb, image_indices, w_affine, b_affine):
    """-> T [N, 12] f32 = emb[image_indices] @ w_affine^T + b_affine, the per-ray 3 x 4 colour transform (swn_affine_ray_fwd)."""
    N, A = image_indices.shape[0], emb.shape[1]
    assert w_affine.shape == (12, A) and b_affine.numel() == 12 and all(t.dtype == torch.float32 and t.is_contiguous() for t in (emb, w_affine, b_affine))
    T = torch.empty(N, 12, dtype=torch.float32, device=emb.device)
    ip, i64 = _idx_arg(image_indices)
    call("swn_affine_ray_fwd", _p(emb), A, ip, i64, _p(w_affine), _p(b_affine), N, _p(T), _stream())
    return T


def affine_ray_bwd(dT, emb, image_indices, w_affine, d_w_affine, d_b_affine):
    """d_w_affine [12, A] += dT^T emb[image_indices], d_b_affine [12] += dT.sum(0) (ordered block sums) -> d_feat [N, A] = dT @ w_affine,
    the per-ray embedding gradient (for emb_grad)."""
    N, A = dT.shape[0], emb.shape[1]
    assert dT.shape == (N, 12) and image_indices.shape[0] == N and d_w_affine.numel() == 12 * A and d_b_affine.numel() == 12
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (dT, emb, w_affine, d_w_affine, d_b_affine))
    nb = C.c_size_t(0)
    call("swn_affine_ray_bwd_workspace_bytes", N, A, C.byref(nb))
    ws = torch.empty(max(int(nb.value), 4) // 4, dtype=torch.float32, device=dT.device)
    d_feat = torch.empty(N, A, dtype=torch.float32, device=dT.device)
    ip, i64 = _idx_arg(image_indices)
    call("swn_affine_ray_bwd", _p(dT), _p(emb), A, ip, i64, _p(w_affine), N, _p(d_w_affine), _p(d_b_affine), _p(d_feat), _p(ws),
         int(nb.value), _stream())
    return d_feat


def heads_affine_fwd(y, h2, w_sigma, b_sigma, w_color, b_color, sigma_noise, T, rows_per_group: int):
    """heads_fwd with the per-ray colour transform T [P / rows_per_group, 12] (swn_heads_affine_fwd) -> raw [P, 4] f32."""
    P, M = y.shape
    H2 = h2.shape[1]
    assert T.dtype == torch.float32 and T.is_contiguous() and T.shape == (P // rows_per_group, 12) and P % rows_per_group == 0
    raw = torch.empty(P, 4, dtype=torch.float32, device=y.device)
    call("swn_heads_affine_fwd", _p(y), _p(h2), _dt(y), _p(w_sigma), _p(b_sigma), _p(w_color), _p(b_color), _p(sigma_noise), _p(T),
         int(rows_per_group), P, M, H2, _p(raw), _stream())
    return raw


def heads_affine_bwd(y, h2, w_color, b_color, T, raw, d_raw, d_w_sigma, d_b_sigma, d_w_color, d_b_color, rows_per_group: int,
                     want_colsum: bool = True):
    """heads_bwd with the colour transform (swn_heads_affine_bwd) -> (dh2, dsig, colsum [P / rows_per_group, H2] f32 or None,
    dT [P / rows_per_group, 12] f32).  y may be None (d_w_sigma untouched)."""
    P, H2 = h2.shape
    M = d_w_sigma.numel()
    assert T.dtype == torch.float32 and T.is_contiguous() and T.shape == (P // rows_per_group, 12) and P % rows_per_group == 0
    dh2 = torch.empty_like(h2)
    dsig = torch.empty(P, dtype=torch.float32, device=h2.device)
    nb = C.c_size_t(0)
    call("swn_heads_affine_bwd_workspace_bytes", P, M, H2, int(rows_per_group), C.byref(nb))
    ws = torch.empty(max(int(nb.value), 4) // 4, dtype=torch.float32, device=h2.device)
    cs = torch.empty(P // rows_per_group, H2, dtype=torch.float32, device=h2.device) if want_colsum else None
    dT = torch.empty(P // rows_per_group, 12, dtype=torch.float32, device=h2.device)
    call("swn_heads_affine_bwd", _p(y), _p(h2), _dt(h2), _p(w_color), _p(b_color), _p(T), _p(raw), _p(d_raw), P, M, H2, int(rows_per_group),
         _p(dh2), _p(dsig), _p(d_w_sigma), _p(d_b_sigma), _p(d_w_color), _p(d_b_color), _p(cs), _p(dT), _p(ws), int(nb.value), _stream())
    return dh2, dsig, cs, dT


def _sh_check(w_color, b_color, dirs, P: int, H2: int, rows_per_group: int, deg: int):
    B = (int(deg) + 1) ** 2
    assert 0 <= int(deg) <= 4, f"sh_deg {deg} outside 0..4"
    assert rows_per_group > 0 and P % rows_per_group == 0
    assert w_color.shape == (3 * B, H2) and b_color.numel() == 3 * B and dirs.shape == (P // rows_per_group, 3)
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (w_color, b_color, dirs))
    return B


def heads_sh_fwd(y, h2, w_sigma, b_sigma, w_color, b_color, sigma_noise, dirs, rows_per_group: int, deg: int, want_coef: bool = False):
    """heads_fwd with spherical-harmonics colour (swn_heads_sh_fwd): w_color [3 B, H2], b_color [3 B], B = (deg + 1)^2, dirs
    [P / rows_per_group, 3] f32 (not normalised) -> raw [P, 4] f32, or (raw, coef [P, 3 B] f32 = the colour head's linear outputs)."""
    P, M = y.shape
    H2 = h2.shape[1]
    B = _sh_check(w_color, b_color, dirs, P, H2, rows_per_group, deg)
    raw = torch.empty(P, 4, dtype=torch.float32, device=y.device)
    coef = torch.empty(P, 3 * B, dtype=torch.float32, device=y.device) if want_coef else None
    call("swn_heads_sh_fwd", _p(y), _p(h2), _dt(y), _p(w_sigma), _p(b_sigma), _p(w_color), _p(b_color), _p(sigma_noise), _p(dirs),
         int(rows_per_group), int(deg), P, M, H2, _p(raw), _p(coef), _stream())
    return (raw, coef) if want_coef else raw


def heads_sh_bwd(y, h2, w_color, b_color, dirs, raw, d_raw, d_w_sigma, d_b_sigma, d_w_color, d_b_color, rows_per_group: int, deg: int,
                 want_colsum: bool = True):
    """heads_bwd with spherical-harmonics colour (swn_heads_sh_bwd) -> (dh2, dsig, colsum [P / rows_per_group, H2] f32 or None); the four
    parameter gradients are accumulated (d_w_color [3 B, H2], d_b_color [3 B]).  The direction gets no gradient."""
    P, H2 = h2.shape
    M = d_w_sigma.numel()
    B = _sh_check(w_color, b_color, dirs, P, H2, rows_per_group, deg)
    assert d_w_color.numel() == 3 * B * H2 and d_b_color.numel() == 3 * B and y is not None
    dh2 = torch.empty_like(h2)
    dsig = torch.empty(P, dtype=torch.float32, device=h2.device)
    nb = C.c_size_t(0)
    call("swn_heads_sh_bwd_workspace_bytes", P, M, H2, int(rows_per_group), int(deg), C.byref(nb))
    ws = torch.empty(max(int(nb.value), 4) // 4, dtype=torch.float32, device=h2.device)
    cs = torch.empty(P // rows_per_group, H2, dtype=torch.float32, device=h2.device) if want_colsum else None
    call("swn_heads_sh_bwd", _p(y), _p(h2), _dt(h2), _p(w_color), _p(b_color), _p(dirs), _p(raw), _p(d_raw), P, M, H2, int(rows_per_group),
         int(deg), _p(dh2), _p(dsig), _p(d_w_sigma), _p(d_b_sigma), _p(d_w_color), _p(d_b_color), _p(cs), _p(ws), int(nb.value), _stream())
    return dh2, dsig, cs


def step_loss(rgb, target, l_aux_a, l_aux_b, wt: float, loss_scale_dev=None):
    """-> (out4 = [photo, gate_loss, loss, psnr] on the device, d_rgb, d_l_aux_a, d_l_aux_b or None)."""
    dev = rgb.device
    d_rgb = torch.empty_like(rgb)
    d_a = torch.empty_like(l_aux_a)
    d_b = torch.empty_like(l_aux_b) if l_aux_b is not None else None
    out4 = torch.empty(4, dtype=torch.float32, device=dev)
    call("swn_step_loss", _p(rgb), _p(target), rgb.numel(), _p(l_aux_a), l_aux_a.numel(), _p(l_aux_b), 0 if l_aux_b is None else l_aux_b.numel(),
         float(wt), _p(loss_scale_dev), _p(d_rgb), _p(d_a), _p(d_b), _p(out4), _stream())
    return out4, d_rgb, d_a, d_b


def cascade_loss(rgb_fine, rgb_coarse, target, l_aux_fine, l_aux_coarse, wt: float, coarse_photo: bool = True, loss_scale_dev=None):
    """-> (out5 = [photo, coarse_loss, gate_loss, loss, psnr] on the device, d_rgb_fine, d_rgb_coarse, d_l_aux_fine or None,
    d_l_aux_coarse or None): the loss of a cascade step (swn_cascade_loss); either gate-loss vector may be None."""
    d_f, d_c = torch.empty_like(rgb_fine), torch.empty_like(rgb_coarse)
    d_lf = torch.empty_like(l_aux_fine) if l_aux_fine is not None else None
    d_lc = torch.empty_like(l_aux_coarse) if l_aux_coarse is not None else None
    out5 = torch.empty(5, dtype=torch.float32, device=rgb_fine.device)
    call("swn_cascade_loss", _p(rgb_fine), _p(rgb_coarse), _p(target), rgb_fine.numel(), _p(l_aux_fine),
         0 if l_aux_fine is None else l_aux_fine.numel(), _p(l_aux_coarse), 0 if l_aux_coarse is None else l_aux_coarse.numel(), float(wt),
         int(bool(coarse_photo)), _p(loss_scale_dev), _p(d_f), _p(d_c), _p(d_lf), _p(d_lc), _p(out5), _stream())
    return out5, d_f, d_c, d_lf, d_lc


def sample_z(rays, t_steps, perturb_rand, perturb: float, n_samples: int):
    n = rays.shape[0]
    z = torch.empty(n, n_samples, dtype=torch.float32, device=rays.device)
    call("swn_sample_z", _p(rays), _p(t_steps), _p(perturb_rand), float(perturb), n, n_samples, _p(z), _stream())
    return z


def _hash_cfg(hc: dict):
    c = _lib.HashCfg()
    c.n_levels, c.log2_table, c.base_res = int(hc["n_levels"]), int(hc["log2_table"]), int(hc["base_res"])
    c.per_level_scale = float(hc["per_level_scale"])
    for i in range(3):
        c.aabb_lo[i], c.aabb_hi[i] = float(hc["aabb_lo"][i]), float(hc["aabb_hi"][i])
    return c


def hash_encode_fwd(rays, z, table, hc: dict, dtype, out_stride: int):
    """Multiresolution hash-grid encoding of the points o + d z (include/swn.h swn_hash_encode_fwd) -> [N * S, out_stride]."""
    n, S = z.shape
    out = torch.empty(n * S, out_stride, dtype=dtype, device=rays.device)
    call("swn_hash_encode_fwd", _p(rays), _p(z), n, S, C.byref(_hash_cfg(hc)), _p(table), _code(dtype),
         _p(out), int(out_stride), _stream())
    return out


_hash_xcd_tables = {}
HASH_XCD_COPIES = 8          # XCDs of an MI300X / MI355X (the kernel picks its copy by HW_REG_XCC_ID & 7: hashgrid.hip)


HASH_XCD_MB = int(os.environ.get("SWN_HASH_XCD_MB", "1024"))      # (read once; tests assign ops.HASH_XCD_MB)


def hash_xcd_budget_bytes() -> int:
    """Upper bound on the per-XCD gradient-table workspace of hash_encode_bwd (SWN_HASH_XCD_MB, default 1024 MiB; 0 = never)."""
    return HASH_XCD_MB << 20


HASH_BWD_MODE = os.environ.get("SWN_HASH_BWD", "binned")      # "binned" (default) | "atomic": read once; tests assign ops.HASH_BWD_MODE
_hash_bin_ws = {}


def hash_encode_bwd(rays, z, d_out, hc: dict, d_table):
    """d_table [L, T, 2] fp32 += the table gradient for dL/d encoding d_out [N * S, stride].

    Default ("binned", swn_hash_encode_bwd_binned): no global float atomics - the contributions are binned by table tile into a workspace
    (12 bytes per (point, level, corner): 3.2 GB at 2M points x 16 levels, kept per size: a captured hipGraph holds its address) and added
    per tile in fixed point in LDS: bit-deterministic, ~4 x faster than the atomics at the recipe's size (profiles/r06_experiments.md 3).
    Tables of more than 2^22 entries per level, or HASH_BWD_MODE = "atomic": the atomic kernels - one private fp32 copy of the gradient
    table per XCD (HASH_XCD_COPIES x the table: 512 MiB at 16 levels x 2^19, zeroed once, left zero by every launch, never freed) so
    that the atomics of an XCD stay in its own L2; a table whose copies would exceed hash_xcd_budget_bytes() takes the plain path:
    atomics straight into d_table."""
    n, S = z.shape
    if HASH_BWD_MODE == "binned" and int(hc["log2_table"]) <= 22 and n * S * 8 * int(hc["n_levels"]) < (1 << 32):
        cfg = _hash_cfg(hc)
        nbytes = int(_lib.load().swn_hash_bwd_workspace_bytes(n * S, C.byref(cfg)))
        key = (d_table.device, nbytes)
        ws = _hash_bin_ws.get(key)
        if ws is None:
            ws = _hash_bin_ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=d_table.device)
        call("swn_hash_encode_bwd_binned", _p(rays), _p(z), n, S, C.byref(cfg), _p(d_out), _dt(d_out), d_out.shape[1], _p(d_table), _p(ws),
             nbytes, _stream())
        return
    ws_bytes = HASH_XCD_COPIES * d_table.numel() * 4
    if ws_bytes > hash_xcd_budget_bytes():
        call("swn_hash_encode_bwd", _p(rays), _p(z), n, S, C.byref(_hash_cfg(hc)), _p(d_out), _dt(d_out), d_out.shape[1], _p(d_table), _stream())
        return
    key = (d_table.device, d_table.numel())
    ws = _hash_xcd_tables.get(key)
    if ws is None:
        ws = _hash_xcd_tables[key] = torch.zeros(HASH_XCD_COPIES * d_table.numel(), dtype=torch.float32, device=d_table.device)
    call("swn_hash_encode_bwd_xcd", _p(rays), _p(z), n, S, C.byref(_hash_cfg(hc)), _p(d_out), _dt(d_out), d_out.shape[1], _p(d_table), _p(ws),
         _stream())


def mip_encode(rays, radii, z, l_xyz: int, dtype, pe_stride: int):
    """-> integrated positional encoding of the n_edges - 1 frustums per ray: [N * (S - 1), pe_stride] dtype"""
    n, S = z.shape
    pe = torch.empty(n * (S - 1), pe_stride, dtype=dtype, device=rays.device)
    call("swn_mip_encode", _p(rays), _p(radii), _p(z), n, S, l_xyz, _dt(pe), _p(pe), pe_stride, _stream())
    return pe


def mip_resample(z, weights, u_rand, n_fine: int, padding: float = 0.01):
    n, S = z.shape
    zf = torch.empty(n, n_fine, dtype=torch.float32, device=z.device)
    call("swn_mip_resample", _p(z), _p(weights), _p(u_rand), float(padding), n, S, n_fine, _p(zf), _stream())
    return zf


def composite_fwd(raw, z, last_delta=1e10, want_weights=False, rgb_padding=0.0):
    N, S = z.shape
    dev = z.device
    rgb = torch.empty(N, 3, dtype=torch.float32, device=dev)
    depth = torch.empty(N, dtype=torch.float32, device=dev)
    dvar = torch.empty(N, dtype=torch.float32, device=dev)
    w = torch.empty(N, S, dtype=torch.float32, device=dev) if want_weights else None
    call("swn_composite_fwd", _p(raw), _p(z), float(last_delta), float(rgb_padding), N, S, _p(rgb), _p(depth), _p(dvar), _p(w), _stream())
    return rgb, depth, dvar, w


def composite_bwd(raw, z, d_rgb, last_delta=1e10, rgb_padding=0.0):
    N, S = z.shape
    d_raw = torch.empty(N * S, 4, dtype=torch.float32, device=z.device)
    call("swn_composite_bwd", _p(raw), _p(z), float(last_delta), float(rgb_padding), _p(d_rgb), N, S, _p(d_raw), _stream())
    return d_raw


def _host3(v):
    """3 floats in host memory (sphere centre / radii) as a ctypes array; None stays None."""
    if v is None:
        return None
    arr = v.detach().cpu().numpy() if torch.is_tensor(v) else v
    vals = [float(x) for x in arr]
    assert len(vals) == 3
    return (C.c_float * 3)(*vals)


def fg_bounds(rays, center, radius, n_out=None):
    """render_rays' foreground bound (rendering.py:32-44, 497-518) -> rays with the clipped far plane, fg_far [N],
    last_delta [N] (fg_far for rays that continue into the background, 1e10 otherwise), has_bg [N] int32, n_out int32 [1] (the rays
    whose closest approach to the centre is outside the bound: the caller raises like the reference).  n_out: a ZEROED int32 [1] to
    count into (e.g. a slice of a larger counter tensor), or None."""
    N = rays.shape[0]
    dev = rays.device
    rays_fg = torch.empty_like(rays)
    fg_far = torch.empty(N, dtype=torch.float32, device=dev)
    last_delta = torch.empty(N, dtype=torch.float32, device=dev)
    has_bg = torch.empty(N, dtype=torch.int32, device=dev)
    if n_out is None:
        n_out = torch.zeros(1, dtype=torch.int32, device=dev)
    assert n_out.dtype == torch.int32 and n_out.numel() == 1
    call("swn_fg_bounds", _p(rays), _host3(center), _host3(radius), N, _p(rays_fg), _p(fg_far), _p(last_delta), _p(has_bg), _p(n_out),
         _stream())
    return rays_fg, fg_far, last_delta, has_bg, n_out


_bg_t_steps = {}


def _bg_linspace(S: int, dev):
    """linspace(0, 1, S) computed on the host like the reference's, cached per (S, device): no pageable host-to-device copy inside a
    step (such a copy cannot be captured into a hipGraph)."""
    key = (int(S), str(dev))
    t = _bg_t_steps.get(key)
    if t is None:
        t = _bg_t_steps[key] = torch.linspace(0, 1, int(S), dtype=torch.float32).to(dev)
    return t


def bg_sample_pe(rays, center, radius, n_samples, l_xyz, dtype, pe_stride, perturb_rand=None, perturb=0.0, z_in=None, pe_out=None):
    """Background samples of the (gathered) rays: see swn_bg_sample_pe in include/swn.h.  -> z [N,S], depth_real [N,S], pe."""
    N = rays.shape[0]
    dev = rays.device
    S = n_samples if z_in is None else z_in.shape[1]
    z = torch.empty(N, S, dtype=torch.float32, device=dev) if z_in is None else z_in
    dreal = torch.empty(N, S, dtype=torch.float32, device=dev)
    pe = pe_out if pe_out is not None else torch.empty(N * S, pe_stride, dtype=dtype, device=dev)
    t_steps = _bg_linspace(S, dev) if z_in is None else None
    call("swn_bg_sample_pe", _p(rays), _host3(center), _host3(radius), _p(t_steps), _p(perturb_rand), float(perturb), N, S, int(l_xyz),
         _code(dtype), _p(z_in), _p(z) if z_in is None else None, _p(dreal), _p(pe), int(pe_stride), _stream())
    return z, dreal, pe


def bg_sample_pe_rng(rays, center, radius, n_samples, l_xyz, dtype, pe_stride, seed: int, step_dev, ray_base: int, row_index=None,
                     index_limit=None, perturb=1.0, pe_out=None):
    """bg_sample_pe's coarse pass with the jitter (domain RNG_DOMAIN_BG, stream RNG_JITTER) drawn inside the kernel: no [N,S] noise buffer.
    Ray r is global ray ray_base + row_index[r] (None: r).  -> z [N,S], depth_real [N,S], pe."""
    assert step_dev.dtype == torch.int64 and step_dev.numel() == 1
    N, S = rays.shape[0], int(n_samples)
    dev = rays.device
    row_index, limit = _row_index_arg(row_index, N, index_limit)
    z = torch.empty(N, S, dtype=torch.float32, device=dev)
    dreal = torch.empty(N, S, dtype=torch.float32, device=dev)
    pe = pe_out if pe_out is not None else torch.empty(N * S, pe_stride, dtype=dtype, device=dev)
    t_steps = _bg_linspace(S, dev)
    call("swn_bg_sample_pe_rng", _p(rays), _host3(center), _host3(radius), _p(t_steps), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(step_dev),
         int(ray_base), _p(row_index), limit, float(perturb), N, S, int(l_xyz), _code(dtype), _p(z), _p(dreal), _p(pe), int(pe_stride),
         _stream())
    return z, dreal, pe


def bg_pad_ray(center, radius):
    """The ray of a padding row of the fixed-shape background (bg_compact): origin at the bound's centre, direction (0, 0, 1), near 0,
    far twice the way to the bound.  Normalised to the unit sphere it starts at the origin, so its background samples, points and
    metric depths (swn_bg_sample_pe) are finite and every later intermediate of a padding row is."""
    c = [0.0, 0.0, 0.0] if center is None else [float(x) for x in _host3(center)]
    rz = 1.0 if radius is None else float(_host3(radius)[2])
    return (C.c_float * 8)(c[0], c[1], c[2], 0.0, 0.0, 1.0, 0.0, 2.0 * rz)


def bg_compact(has_bg, rays, image_indices, capacity: int, pad_ray, n_bg=None):
    """Stable device-side compaction of the rays with has_bg != 0 into `capacity` rows (swn_bg_compact, include/swn.h) ->
    idx_bg int64 [C], n_bg int32 [1] (the true count, also above C), rays_b [C, 8], img_b [C]; rows from n_bg on are padding
    (idx 0, image 0, pad_ray: bg_pad_ray).  n_bg: an int32 [1] to write the count to, or None."""
    N, Cc = rays.shape[0], int(capacity)
    if not 1 <= Cc <= N:
        raise ValueError(f"bg_compact: capacity {Cc} outside [1, {N} rays]")
    dev = rays.device
    assert has_bg.dtype == torch.int32 and has_bg.numel() == N and rays.dtype == torch.float32 and tuple(rays.shape) == (N, 8)
    assert image_indices.numel() == N
    idx_bg = torch.empty(Cc, dtype=torch.int64, device=dev)
    if n_bg is None:
        n_bg = torch.empty(1, dtype=torch.int32, device=dev)
    assert n_bg.dtype == torch.int32 and n_bg.numel() == 1
    rays_b = torch.empty(Cc, 8, dtype=torch.float32, device=dev)
    img_b = torch.empty(Cc, dtype=image_indices.dtype, device=dev)
    ip, i64 = _idx_arg(image_indices)
    call("swn_bg_compact", _p(has_bg), _p(rays), ip, i64, pad_ray, N, Cc, _p(idx_bg), _p(n_bg), _p(rays_b), _p(img_b), _stream())
    return idx_bg, n_bg, rays_b, img_b


def _blend_check(idx_bg, n_bg, lam):
    assert idx_bg.dtype == torch.int64 and n_bg.dtype == torch.int32 and n_bg.numel() == 1 and lam.dtype == torch.float32
    return lam.numel(), idx_bg.numel()


def bg_blend_fwd(rgb, depth, idx_bg, n_bg, lam, rgb_b, depth_b):
    """IN PLACE: rgb[idx_bg[j]] += rgb_b[j] * lam[idx_bg[j]], depth likewise, for j < min(n_bg, C) (swn_bg_blend_fwd)."""
    N, Cc = _blend_check(idx_bg, n_bg, lam)
    assert rgb.dtype == depth.dtype == rgb_b.dtype == depth_b.dtype == torch.float32
    assert tuple(rgb.shape) == (N, 3) and depth.numel() == N and tuple(rgb_b.shape) == (Cc, 3) and depth_b.numel() == Cc
    call("swn_bg_blend_fwd", _p(idx_bg), _p(n_bg), _p(lam), _p(rgb_b), _p(depth_b), N, Cc, _p(rgb), _p(depth), _stream())
    return rgb, depth


def bg_blend_bwd(d_rgb, idx_bg, n_bg, lam, rgb_b):
    """-> d_lam [N] (0 on rays without background), d_rgb_b [C, 3] (exactly 0 on padding rows): swn_bg_blend_bwd."""
    N, Cc = _blend_check(idx_bg, n_bg, lam)
    assert d_rgb.dtype == rgb_b.dtype == torch.float32 and tuple(d_rgb.shape) == (N, 3) and tuple(rgb_b.shape) == (Cc, 3)
    d_lam = torch.empty(N, dtype=torch.float32, device=lam.device)
    d_rgb_b = torch.empty(Cc, 3, dtype=torch.float32, device=lam.device)
    call("swn_bg_blend_bwd", _p(idx_bg), _p(n_bg), _p(lam), _p(rgb_b), _p(d_rgb), N, Cc, _p(d_lam), _p(d_rgb_b), _stream())
    return d_lam, d_rgb_b


def cells_assign(x, centroids, dim_start: int, margin: float):
    """Spatial-cell membership of the points x [P, stride] (position in columns 0..2) among centroids [K, 3] (swn_cells_assign,
    mega_nerf.py:21-30) -> weights [P, K] fp32 (margin == 1: one-hot of the first nearest cell), counts [K] int32."""
    P, K = x.shape[0], centroids.shape[0]
    assert x.dtype == centroids.dtype == torch.float32 and x.dim() == 2 and centroids.dim() == 2 and centroids.shape[1] == 3
    weights = torch.empty(P, K, dtype=torch.float32, device=x.device)
    counts = torch.empty(K, dtype=torch.int32, device=x.device)
    call("swn_cells_assign", _p(x), x.shape[1], _p(centroids), K, int(dim_start), float(margin), P, _p(weights), _p(counts), _stream())
    return weights, counts


def cells_pack(weights, counts, rows_capacity: Optional[int] = None):
    """The packed row space of a membership (swn_cells_pack) -> begin [K + 1], rows [rows_capacity] (the first begin[K] entries: point
    indices by cell, ascending inside a cell), slot [P, K] (row inside the cell, or -1).  rows_capacity defaults to P * K."""
    P, K = weights.shape
    assert weights.dtype == torch.float32 and counts.dtype == torch.int32 and counts.numel() == K
    dev = weights.device
    cap = P * K if rows_capacity is None else int(rows_capacity)
    begin = torch.empty(K + 1, dtype=torch.int32, device=dev)
    rows = torch.empty(cap, dtype=torch.int32, device=dev)
    slot = torch.empty(P, K, dtype=torch.int32, device=dev)
    need = C.c_size_t(0)
    call("swn_cells_pack_workspace_bytes", P, K, C.byref(need))
    ws = torch.empty(max(1, need.value // 4), dtype=torch.int32, device=dev)
    call("swn_cells_pack", _p(weights), _p(counts), P, K, _p(begin), _p(rows), cap, _p(slot), _p(ws), need.value, _stream())
    return begin, rows, slot


def cells_gather(x, rows, total: int, col0: int = 0, sigma_noise=None):
    """x_out [total, stride - col0] = x[rows[r], col0:], noise_out [total] = sigma_noise[rows[r]] or None (swn_cells_gather)."""
    P, stride = x.shape
    assert x.dtype == torch.float32 and rows.dtype == torch.int32 and rows.numel() >= total
    x_out = torch.empty(total, stride - col0, dtype=torch.float32, device=x.device)
    noise_out = None
    if sigma_noise is not None:
        assert sigma_noise.dtype == torch.float32 and sigma_noise.numel() == P
        noise_out = torch.empty(total, dtype=torch.float32, device=x.device)
    call("swn_cells_gather", _p(x), stride, int(col0), _p(rows), int(total), P, _p(sigma_noise), _p(x_out), _p(noise_out), _stream())
    return x_out, noise_out


def cells_pack_padded(weights, counts, capacity: int):
    """The PADDED row space of a membership (swn_cells_pack_padded): cell i owns the rows [i C, (i + 1) C), C = capacity, whatever the
    batch -> begin [K + 1] (i C), rows [K C] (cell i's member points, ascending, in the first min(counts[i], C) entries of its range; -1
    = a padding row), slot [P, K] (-1 also for a member that did not fit), overflow [1] int32 (the memberships dropped).  begin / rows /
    slot go to cells_blend / cells_blend_bwd with total = K C."""
    P, K = weights.shape
    Cc = int(capacity)
    assert weights.dtype == torch.float32 and counts.dtype == torch.int32 and counts.numel() == K and Cc >= 1
    dev = weights.device
    begin = torch.empty(K + 1, dtype=torch.int32, device=dev)
    rows = torch.empty(K * Cc, dtype=torch.int32, device=dev)
    slot = torch.empty(P, K, dtype=torch.int32, device=dev)
    overflow = torch.empty(1, dtype=torch.int32, device=dev)
    need = C.c_size_t(0)
    call("swn_cells_pack_workspace_bytes", P, K, C.byref(need))
    ws = torch.empty(max(1, need.value // 4), dtype=torch.int32, device=dev)
    call("swn_cells_pack_padded", _p(weights), _p(counts), P, K, Cc, _p(begin), _p(rows), _p(slot), _p(overflow), _p(ws), need.value,
         _stream())
    return begin, rows, slot, overflow


def cells_gather_padded(x, rows, centroids, capacity: int, col0: int = 0, sigma_noise=None):
    """cells_gather over the padded row space (swn_cells_gather_padded), x [P, col0 + 7]: x_out [K C, 7], noise_out [K C] or None.  A
    padding row (rows[r] < 0) is its cell's centroid seen along (0, 0, 1) in image 0 with sigma noise 0; it reads nothing of x."""
    P, stride = x.shape
    K, Cc = centroids.shape[0], int(capacity)
    assert x.dtype == centroids.dtype == torch.float32 and rows.dtype == torch.int32 and rows.numel() == K * Cc
    x_out = torch.empty(K * Cc, stride - col0, dtype=torch.float32, device=x.device)
    noise_out = None
    if sigma_noise is not None:
        assert sigma_noise.dtype == torch.float32 and sigma_noise.numel() == P
        noise_out = torch.empty(K * Cc, dtype=torch.float32, device=x.device)
    call("swn_cells_gather_padded", _p(x), stride, int(col0), _p(rows), _p(centroids), K, Cc, P, _p(sigma_noise), _p(x_out), _p(noise_out),
         _stream())
    return x_out, noise_out


def _sigma_rng_args(seed: int, step_dev, stream_id: int, rows_per_ray: int, ray_base: int, scale: float):
    assert step_dev.dtype == torch.int64 and step_dev.numel() == 1
    return (int(seed) & 0xFFFFFFFFFFFFFFFF, _p(step_dev), int(stream_id), int(rows_per_ray), int(ray_base), float(scale))


def cells_gather_rng(x, rows, total: int, col0: int, seed: int, step_dev, stream_id: int, rows_per_ray: int, ray_base: int, scale: float):
    """cells_gather with the sigma noise drawn at the packed row (swn_cells_gather_rng): noise_out [total] = scale * the normal draw of
    element ray_base * rows_per_ray + rows[r] of (seed, step_dev[0], stream_id) - rng_fill(P, ray_base * rows_per_ray, RNG_NORMAL, ...,
    scale)[rows[r]] bit for bit, with no [P] tensor.  stream_id: RNG_SIGMA or RNG_SIGMA_FINE."""
    P, stride = x.shape
    assert x.dtype == torch.float32 and rows.dtype == torch.int32 and rows.numel() >= total
    x_out = torch.empty(total, stride - col0, dtype=torch.float32, device=x.device)
    noise_out = torch.empty(total, dtype=torch.float32, device=x.device)
    call("swn_cells_gather_rng", _p(x), stride, int(col0), _p(rows), int(total), P,
         *_sigma_rng_args(seed, step_dev, stream_id, rows_per_ray, ray_base, scale), _p(x_out), _p(noise_out), _stream())
    return x_out, noise_out


def cells_gather_padded_rng(x, rows, centroids, capacity: int, col0: int, seed: int, step_dev, stream_id: int, rows_per_ray: int,
                            ray_base: int, scale: float):
    """cells_gather_padded with the sigma noise drawn at the packed row (swn_cells_gather_padded_rng), addressed like cells_gather_rng;
    a padding row gets exactly +0."""
    P, stride = x.shape
    K, Cc = centroids.shape[0], int(capacity)
    assert x.dtype == centroids.dtype == torch.float32 and rows.dtype == torch.int32 and rows.numel() == K * Cc
    x_out = torch.empty(K * Cc, stride - col0, dtype=torch.float32, device=x.device)
    noise_out = torch.empty(K * Cc, dtype=torch.float32, device=x.device)
    call("swn_cells_gather_padded_rng", _p(x), stride, int(col0), _p(rows), _p(centroids), K, Cc, P,
         *_sigma_rng_args(seed, step_dev, stream_id, rows_per_ray, ray_base, scale), _p(x_out), _p(noise_out), _stream())
    return x_out, noise_out


def cells_blend(weights, slot, begin, sub_out, hard: bool):
    """out [P, C] = sum over the member cells (ascending) of weights * sub_out[begin[i] + slot] (swn_cells_blend), C = sub_out.shape[1]
    in {1, 4}; hard: the plain copy of the one member's row."""
    P, K = weights.shape
    total, Cn = sub_out.shape
    assert sub_out.dtype == torch.float32 and slot.dtype == begin.dtype == torch.int32 and tuple(slot.shape) == (P, K)
    out = torch.empty(P, Cn, dtype=torch.float32, device=weights.device)
    call("swn_cells_blend", _p(weights), _p(slot), _p(begin), _p(sub_out), total, P, K, Cn, 1 if hard else 0, _p(out), _stream())
    return out


def cells_blend_bwd(weights, rows, begin, d_out, total: int, hard: bool):
    """d_sub [total, C] = weights[rows[r], cell of r] * d_out[rows[r]] (swn_cells_blend_bwd): the adjoint of cells_blend with respect to
    sub_out, C = d_out.shape[1] in {1, 4}; hard: the plain copy.  rows / begin: cells_pack's."""
    P, K = weights.shape
    Cn, total = d_out.shape[1], int(total)
    assert weights.dtype == d_out.dtype == torch.float32 and rows.dtype == begin.dtype == torch.int32 and d_out.shape[0] == P
    assert 0 <= total <= rows.numel() and begin.numel() == K + 1 and all(t.is_contiguous() for t in (weights, rows, begin, d_out))
    d_sub = torch.empty(total, Cn, dtype=torch.float32, device=weights.device)
    call("swn_cells_blend_bwd", _p(weights), _p(rows), _p(begin), _p(d_out), total, P, K, Cn, 1 if hard else 0, _p(d_sub), _stream())
    return d_sub


def cells_blend_sh(weights, slot, begin, sub_out, dirs, rows_per_group: int, deg: int, hard: bool, want_coef: bool = False):
    """cells_blend for sub-models with spherical-harmonics colour, fused with the evaluation (swn_cells_blend_sh): sub_out [total, 3 B + 1]
    (coefficients row-major [3, B], then sigma), dirs [P / rows_per_group, 3] f32 (not normalised) -> raw [P, 4] = (sigmoid(eval_sh of
    the blended coefficients), blended sigma), or (raw, coef [P, 3 B + 1] = the blended rows).  The library checks deg, rows_per_group
    and the sizes."""
    P, K = weights.shape
    total, width = sub_out.shape
    assert weights.dtype == sub_out.dtype == dirs.dtype == torch.float32 and slot.dtype == begin.dtype == torch.int32
    assert tuple(slot.shape) == (P, K) and begin.numel() == K + 1 and all(t.is_contiguous() for t in (weights, slot, begin, sub_out, dirs))
    rows_per_group, deg = int(rows_per_group), int(deg)
    if 0 <= deg <= 4 and rows_per_group >= 1 and P % rows_per_group == 0:      # (otherwise: the library's error)
        assert width == 3 * (deg + 1) ** 2 + 1 and tuple(dirs.shape) == (P // rows_per_group, 3)
    raw = torch.empty(P, 4, dtype=torch.float32, device=weights.device)
    coef = torch.empty(P, width, dtype=torch.float32, device=weights.device) if want_coef else None
    call("swn_cells_blend_sh", _p(weights), _p(slot), _p(begin), _p(sub_out), total, _p(dirs), rows_per_group, deg, P, K,
         1 if hard else 0, _p(raw), _p(coef), _stream())
    return (raw, coef) if want_coef else raw


def cells_blend_sh_bwd(weights, rows, begin, raw, d_raw, dirs, rows_per_group: int, deg: int, total: int, hard: bool, sub_out=None):
    """The adjoint of cells_blend_sh with respect to sub_out, factored (swn_cells_blend_sh_bwd) -> (q [total, 4], dirs_packed [total, 3]):
    d_lin[r][c B + b] = q[r][c] Y_b(dirs_packed[r]), d_sigma[r] = q[r][3].  raw: cells_blend_sh's output [P, 4]; sub_out [total, 4]: the
    packed rows, needed at degree 0 (the cells' own sigmoid).  The library checks deg, rows_per_group and the sizes."""
    P, K = weights.shape
    total, rows_per_group, deg = int(total), int(rows_per_group), int(deg)
    assert weights.dtype == raw.dtype == d_raw.dtype == dirs.dtype == torch.float32 and rows.dtype == begin.dtype == torch.int32
    assert tuple(raw.shape) == tuple(d_raw.shape) == (P, 4) and 0 <= total <= rows.numel() and begin.numel() == K + 1
    assert all(t.is_contiguous() for t in (weights, rows, begin, raw, d_raw, dirs))
    if rows_per_group >= 1 and P % rows_per_group == 0:      # (otherwise: the library's error)
        assert tuple(dirs.shape) == (P // rows_per_group, 3)
    if sub_out is not None:
        assert sub_out.dtype == torch.float32 and sub_out.is_contiguous() and (deg != 0 or tuple(sub_out.shape) == (total, 4))
    q = torch.empty(total, 4, dtype=torch.float32, device=weights.device)
    dp = torch.empty(total, 3, dtype=torch.float32, device=weights.device)
    call("swn_cells_blend_sh_bwd", _p(weights), _p(rows), _p(begin), _p(raw), _p(d_raw), _p(dirs), _p(sub_out), total, rows_per_group, deg, P, K,
         1 if hard else 0, _p(q), _p(dp), _stream())
    return q, dp


def heads_coef_fwd(y, h2, w_sigma, b_sigma, w_color, b_color, sigma_noise, deg: int, out, inner_sigmoid: bool = False):
    """A cell's heads over packed rows (swn_heads_coef_fwd): out [n, 3 B + 1] f32 - a row-contiguous view, e.g. the cell's slice of the
    packed sub_out - receives (h2 Wc^T + bc, softplus(..)); inner_sigmoid (degree 0): sigmoid on the three colour outputs.  -> out."""
    n, M = y.shape
    H2 = h2.shape[1]
    B = (int(deg) + 1) ** 2
    assert w_color.shape == (3 * B, H2) and b_color.numel() == 3 * B and all(t.dtype == torch.float32 and t.is_contiguous() for t in (w_color, b_color))
    assert out.dtype == torch.float32 and tuple(out.shape) == (n, 3 * B + 1) and out.stride(1) == 1 and (n <= 1 or out.stride(0) >= 3 * B + 1)
    assert sigma_noise is None or (sigma_noise.dtype == torch.float32 and sigma_noise.numel() == n and sigma_noise.is_contiguous())
    call("swn_heads_coef_fwd", _p(y), _p(h2), _dt(y), _p(w_sigma), _p(b_sigma), _p(w_color), _p(b_color), _p(sigma_noise), int(deg),
         1 if inner_sigmoid else 0, n, M, H2, _pv(out), out.stride(0) if n > 1 else 3 * B + 1, _stream())
    return out


def heads_coef_bwd_workspace_bytes(n: int, M: int, H2: int, deg: int) -> int:
    nb = C.c_size_t(0)
    call("swn_heads_coef_bwd_workspace_bytes", int(n), int(M), int(H2), int(deg), C.byref(nb))
    return int(nb.value)


def heads_coef_bwd(y, h2, w_color, q, dirs, rows_out, d_w_sigma, d_b_sigma, d_w_color, d_b_color, deg: int, want_colsum: bool = True):
    """The backward of heads_coef_fwd (swn_heads_coef_bwd) from q [n, 4], dirs [n, 3] (cells_blend_sh_bwd's, a cell's slice) and rows_out
    [n, 3 B + 1] = what heads_coef_fwd wrote (its sigma column is read) -> (dh2, dsig, colsum [n, H2] f32 or None); the four parameter
    gradients are accumulated."""
    n, H2 = h2.shape
    M = d_w_sigma.numel()
    B = (int(deg) + 1) ** 2
    assert w_color.shape == (3 * B, H2) and w_color.dtype == torch.float32 and w_color.is_contiguous()
    assert d_w_color.numel() == 3 * B * H2 and d_b_color.numel() == 3 * B and y is not None
    assert q.dtype == dirs.dtype == rows_out.dtype == torch.float32 and tuple(q.shape) == (n, 4) and tuple(dirs.shape) == (n, 3)
    assert q.is_contiguous() and dirs.is_contiguous() and tuple(rows_out.shape) == (n, 3 * B + 1) and rows_out.stride(1) == 1
    dh2 = torch.empty_like(h2)
    dsig = torch.empty(n, dtype=torch.float32, device=h2.device)
    nb = heads_coef_bwd_workspace_bytes(n, M, H2, deg)
    ws = torch.empty(max(nb, 4) // 4, dtype=torch.float32, device=h2.device)
    cs = torch.empty(n, H2, dtype=torch.float32, device=h2.device) if want_colsum else None
    sig = rows_out[:, 3 * B]
    call("swn_heads_coef_bwd", _p(y), _p(h2), _dt(h2), _p(w_color), _p(q), _p(dirs), _pv(sig), rows_out.stride(0) if n > 1 else 3 * B + 1, n, M, H2,
         int(deg), _p(dh2), _p(dsig), _p(d_w_sigma), _p(d_b_sigma), _p(d_w_color), _p(d_b_color), _p(cs), _p(ws), nb, _stream())
    return dh2, dsig, cs


def composite_bounded_fwd(raw, z, last_delta=None, flip=False, depth_real=None, want_weights=False, want_bg_lambda=False):
    """Compositing with a per-ray last delta / descending depths / metric depth source / leftover transmittance
    (rendering.py:435-494 with last_delta, flip, depth_real, get_bg_lambda) -> rgb, depth, depth_variance, weights, bg_lambda."""
    N, S = z.shape
    dev = z.device
    rgb = torch.empty(N, 3, dtype=torch.float32, device=dev)
    depth = torch.empty(N, dtype=torch.float32, device=dev)
    dvar = torch.empty(N, dtype=torch.float32, device=dev)
    w = torch.empty(N, S, dtype=torch.float32, device=dev) if want_weights else None
    lam = torch.empty(N, dtype=torch.float32, device=dev) if want_bg_lambda else None
    call("swn_composite_bounded_fwd", _p(raw), _p(z), _p(last_delta), int(bool(flip)), _p(depth_real), N, S, _p(rgb), _p(depth),
         _p(dvar), _p(w), _p(lam), _stream())
    return rgb, depth, dvar, w, lam


PLY_RGBA, PLY_SEG_ALPHA, PLY_SEG_RGB = 0, 1, 2        # swn_points_pack modes (include/swn.h)
PLY_RECORD_BYTES = {PLY_RGBA: 16, PLY_SEG_ALPHA: 16, PLY_SEG_RGB: 15}


def point_fields(rays, z, raw, last_delta=1e10, z_pts=None, order=None, want_pts=True, want_alpha=True, want_pts_alpha=True):
    """Per-sample point outputs of one pass (rendering.py:299, :443-452): z [N,T] / raw [N*T,4] the depths and outputs it
    composites (merged order when `order` [N,T] is given), last_delta a float or a per-ray [N] tensor, z_pts [N,n] the pass's own
    unmerged depths (None = z).  -> pts [N,n,3], alpha [N,T], pts_alpha [N,n] (None where not wanted)."""
    N, T = z.shape
    zp = z if z_pts is None else z_pts
    n = zp.shape[1]
    dev = z.device
    pts = torch.empty(N, n, 3, dtype=torch.float32, device=dev) if want_pts else None
    alpha = torch.empty(N, T, dtype=torch.float32, device=dev) if want_alpha else None
    pa = torch.empty(N, n, dtype=torch.float32, device=dev) if want_pts_alpha else None
    ld_ray = last_delta.contiguous() if torch.is_tensor(last_delta) else None
    ld = 1e10 if ld_ray is not None else float(last_delta)
    call("swn_point_fields", _p(rays), _p(zp), n, _p(z), _p(raw), N, T, ld, _p(ld_ray), _p(order), _p(pts), _p(alpha), _p(pa),
         _stream())
    return pts, alpha, pa


def _rgb_arg(rgb, R, S):
    """pts_rgb [R,S,3]: contiguous (stride 3) or the raw[:, :3] view of a contiguous raw [R*S,4] (stride 4); anything else is
    copied.  -> (tensor to keep alive until the launch, pointer, sample stride)."""
    assert rgb.is_cuda and rgb.dtype == torch.float32 and tuple(rgb.shape) == (R, S, 3)
    for cs in (3, 4):
        if rgb.stride() == (S * cs, cs, 1):
            return rgb, C.c_void_p(rgb.data_ptr()), cs
    rgb = rgb.contiguous()
    return rgb, C.c_void_p(rgb.data_ptr()), 3


def points_pack(pts, pts_alpha, mode, skip=1, idx=None, n_experts=1, pts_rgb=None, pixel_rgb=None, palette=None, want_all=True,
                want_experts=True):
    """PLY vertex bodies of the kept samples [:, :, ::skip] on the device (swn_points_pack): -> (all [K * rec] uint8 or None,
    experts [K * rec] uint8 - expert 0's records, then expert 1's, ... - or None, counts [E] int32 or None), K = R * ceil(S / skip)."""
    R, S = pts.shape[0], pts.shape[1]
    dev = pts.device
    rec = PLY_RECORD_BYTES[mode]
    K = R * ((S + skip - 1) // skip)
    part = want_experts and idx is not None
    out_all = torch.empty(K * rec, dtype=torch.uint8, device=dev) if want_all else None
    out_exp = torch.empty(K * rec, dtype=torch.uint8, device=dev) if part else None
    counts = torch.zeros(n_experts, dtype=torch.int32, device=dev) if part else None
    ws_bytes = 4 * n_experts * ((K + 2047) // 2048) if part else 0        # the block counts (include/swn.h)
    ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device=dev) if part else None
    _rgb, rgb_p, rgb_stride = _rgb_arg(pts_rgb, R, S) if pts_rgb is not None else (None, None, 3)
    if idx is not None:
        idx = idx.reshape(-1)
        idx = idx if idx.dtype == torch.int32 else idx.to(torch.int32)
        assert idx.numel() == R * S
    call("swn_points_pack", _p(pts.contiguous()), rgb_p, rgb_stride, _p(None if pts_alpha is None else pts_alpha.contiguous()),
         _p(None if idx is None else idx.contiguous()), _p(None if pixel_rgb is None else pixel_rgb.contiguous()), _p(palette), R, S,
         int(skip), int(n_experts), int(mode), _p(out_all), _p(out_exp), _p(counts), _p(ws), ws_bytes, _stream())
    return out_all, out_exp, counts


def composite_bounded_bwd(raw, z, d_rgb, last_delta=None, flip=False, d_bg_lambda=None):
    N, S = z.shape
    d_raw = torch.empty(N * S, 4, dtype=torch.float32, device=z.device)
    call("swn_composite_bounded_bwd", _p(raw), _p(z), _p(last_delta), int(bool(flip)), _p(d_rgb), _p(d_bg_lambda), N, S, _p(d_raw),
         _stream())
    return d_raw


def pack_weights(master, dtype, transpose: bool):
    """master [n_wsets, in, out] fp32 -> packed compute copy for mlp_chain, tagged with its logical (n, k)."""
    assert master.dim() == 3 and master.dtype == torch.float32
    ws, i, o_ = master.shape
    out = torch.empty(ws * i * o_, dtype=dtype, device=master.device)
    call("swn_pack_weights", _p(master), _p(out), _dt(out), ws, i, o_, int(bool(transpose)), _stream())
    out.swn_nk = (o_, i) if transpose else (i, o_)
    return out


def repack_weights(master, packed, transpose: bool):
    ws, i, o_ = master.shape
    call("swn_pack_weights", _p(master), _p(packed), _dt(packed), ws, i, o_, int(bool(transpose)), _stream())
    return packed


def repack_weights_batched(pairs):
    """pairs: (master [ws, in, out] f32, packed, transpose[, in_padded[, out_padded]]) of one compute dtype -> one launch per 32 weights.
    in_padded / out_padded: the packed copy's in / out dimension when larger than the master's (zero-padded: pack_weights_padded)."""
    from ._lib import PackItem
    for i0 in range(0, len(pairs), 32):
        chunk = pairs[i0:i0 + 32]
        arr = (PackItem * len(chunk))()
        for it, pr in zip(arr, chunk):
            master, packed, transpose = pr[:3]
            ws, i, o_ = master.shape
            ipad = int(pr[3]) if len(pr) > 3 and pr[3] else i
            opad = int(pr[4]) if len(pr) > 4 and pr[4] else o_
            it.master, it.out, it.n_wsets, it.in_dim, it.out_dim, it.transpose = _p(master), _p(packed), ws, ipad, opad, int(bool(transpose))
            it.in_rows, it.out_cols = (i if ipad != i else 0), (o_ if opad != o_ else 0)
        call("swn_pack_weights_batched", arr, len(chunk), _dt(chunk[0][1]), _stream())


def pack_weights_padded(master, dtype, transpose: bool, in_padded: int = 0, out_padded: int = 0):
    """pack_weights with the master's in / out dimension zero-padded: a 128-feature first layer for the K = 256 kernels of chain
    geometries 6 / 7 (mlp_chain(..., x_features=128)) - forward (transpose): in 128 -> 256; backward-data of a 128-output layer: out 128 ->
    256.  Refresh with repack_weights_batched([(master, packed, transpose, in_padded, out_padded)])."""
    assert master.dim() == 3 and master.dtype == torch.float32
    ws, i, o_ = master.shape
    ipad, opad = in_padded or i, out_padded or o_
    assert ipad >= i and opad >= o_
    out = torch.empty(ws * ipad * opad, dtype=dtype, device=master.device)
    out.swn_nk = (opad, ipad) if transpose else (ipad, opad)
    repack_weights_batched([(master, out, transpose, ipad, opad)])
    return out


class Layer:
    """One Linear of a chain: w = pack_weights(...) output (carries .swn_nk = (N, K)), b [n_wsets, N] f32 or None."""

    def __init__(self, w, b=None, relu=0, skip=False, save=None, mask=None, rowbias=None, rows_per_bias=0):
        self.w, self.b, self.relu, self.skip, self.save, self.mask = w, b, int(relu), int(skip), save, mask      # skip: 0 / 1 residual / 2 concat half
        self.rowbias, self.rows_per_bias = rowbias, int(rows_per_bias)

    def without_saves(self):
        """The layer as an inference launch runs it: no activation save, no ReLU mask."""
        return Layer(self.w, self.b, self.relu, self.skip, None, None, self.rowbias, self.rows_per_bias)

    def with_mask_words(self, w0, w1):
        """The layer with words [w0, w1) of its ReLU mask (one routing segment of a mask buffer that holds every segment's)."""
        return Layer(self.w, self.b, self.relu, self.skip, self.save, None if self.mask is None else self.mask[w0:w1], self.rowbias,
                     self.rows_per_bias)


# ---- the expert chain's rules, each written once (SwitchNeRF, ep_owner.py and the autograd functions of moe.py build their launches from
# these; pure Python over Layer and tensors)
def expert_fwd_layers(w, b, skips, saves, masks):
    """Forward layers of an expert MLP from packed weights w[l] and biases b[l]: ReLU on all but the last layer, the residual skip on the
    layers in `skips`; layer l < L - 1 saves its output in saves[l] and its ReLU mask in masks[l] (length L - 1, None = nothing saved)."""
    L = len(w)
    return [Layer(w[l], b[l], relu=1 if l < L - 1 else 0, skip=(l in skips), save=saves[l] if l < L - 1 else None,
                  mask=masks[l] if l < L - 1 else None) for l in range(L)]


def expert_bwd_layers(wb, masks, dz):
    """Backward-data layers in launch order (layer L - 1 first) from the backward copies wb[l]: above layer 0 the layer's input gradient
    goes through the ReLU mask of the layer below (relu = 2, masks[l - 1]) and is saved as dz[l - 1], the next weight-gradient operand."""
    return [Layer(wb[l], None, relu=2 if l > 0 else 0, mask=masks[l - 1] if l > 0 else None, save=dz[l - 1] if l > 0 else None)
            for l in range(len(wb) - 1, -1, -1)]


def expert_wgrad_items(x_first, saves, dz, dz_last, dw, db, a_gather=None, b_gather=None):
    """(a, dz, dw, db, a_gather, b_gather) per layer for wgrad_multi / wgrad_batched: layer 0 reads the chain's input rows x_first (through
    a_gather), layer l > 0 the saved output of layer l - 1; layer L - 1 reads dz_last (through b_gather), layer l < L - 1 the saved dz[l]."""
    L = len(dw)
    return [(x_first if l == 0 else saves[l - 1], dz_last if l == L - 1 else dz[l], dw[l], db[l], a_gather if l == 0 else None,
             b_gather if l == L - 1 else None) for l in range(L)]


def expert_geometry(M, dt, rows, preferred=7):
    """Geometry of an expert chain, forward and backward alike (the pair shares its ReLU mask layout): `preferred` for 256-feature experts
    in a 16-bit compute dtype once a group holds at least one full 256-row tile, else the 64-row kernels (1)."""
    return preferred if (M == 256 and dt != torch.float32 and rows >= 256) else 1


def chain_tile_rows(dtype) -> int:
    return _lib.load().swn_chain_tile_rows(_code(dtype))


def chain_mask_words(dtype, n_groups: int, group_stride: int, max_width: int = 256) -> int:
    """uint32 words per layer mask buffer for a chain launch with this geometry (1 bit per row x feature of the kernel's tile;
    max_width = the widest layer of the chain: > 256 selects the 512-feature kernels)."""
    return int(_lib.load().swn_chain_mask_words(_code(dtype), int(n_groups), int(group_stride), int(max_width)))


def chain_mask_words_packed(dtype, rows: int, n_groups: int, max_width: int = 256) -> int:
    """uint32 words per layer mask buffer of a chain with packed mask slots (mlp_chain(packed_rows=rows)): at most `rows` packed rows
    in n_groups groups - ceil(rows / tile rows) + n_groups tiles instead of n_groups * ceil(group_stride / tile rows)."""
    w = C.c_int64(0)
    call("swn_chain_mask_words_packed", _code(dtype), int(rows), int(n_groups), int(max_width), C.byref(w))
    return int(w.value)


def mlp_chain(x, layers: Sequence[Layer], y, n_groups=1, n_wsets=1, group_stride=None, group_rows=None,
              group_rows_clamp=None, x_gather=None, x_save=None, y_add=None, y_add_gather=None, tag=0, x_scale=None,
              x_relu=False, geometry=0, group_begin=None, combine=None, heads=None, sched=None, x_features=0, tail=None, head=None,
              packed_rows=0, x_k=0):
    """geometry: 0 / 1 the 64-row tile kernels, 2 - 5 the chain_big.hip geometries (include/swn.h).  group_begin: first row of every
    group (packed / no-batch layout) instead of g * group_stride.  combine = (y_fwd, dsig, wsig, gate, dgate_out): the combine backward
    (ops.combine_bwd) fused into the write-out of the last layer.  heads = (w_sigma, b_sigma, w_color, b_color, sigma_noise or None, raw):
    the sigma / colour heads (ops.heads_fwd) fused into the tail forward chain (tag 4) - y may then be None (nothing but raw is written).
    sched: int32 [16] zero-initialised tile-queue counters of the persistent geometries 6 / 7 (chain_sched(); left zero by the kernel).
    tail = (tail_first, gate [P] f32, drop_begin, dropped, y_features[, bias_row int32 [P]]): the dense tail folded into the expert forward chain (include/swn.h,
    tail_first: geometry 7, tag 7) - layers[tail_first:] are shared layers, the saves from layer tail_first - 1 on, y and the heads'
    raw are in token order (P rows), x_gather maps rows to tokens.
    head = (head_layers, drop_begin, dropped): the mirror image for the backward pass (include/swn.h, head_layers: geometry 7, tag 8) -
    x = dh2 in token order, layers[:head_layers] shared, `combine` (token order) applied behind them, the expert backward layers after.
    packed_rows > 0: packed ReLU-mask slots (include/swn.h swn_chain_desc.packed_rows; group_begin required, geometry 0 / 1 / 7): the
    masks of a row space of at most packed_rows rows, sized by chain_mask_words_packed - the forward and backward chains set it alike.
    x_k > 0 (with x_features = 128): the first layer's real K - the zero half of its padded weights is not multiplied (include/swn.h
    swn_chain_desc.x_k; same bits as x_k = 0 for finite x)."""
    d = ChainDesc()
    d.packed_rows = int(packed_rows)
    d.dtype = _dt(x)
    d.tag = int(tag)
    d.geometry = int(geometry)
    d.n_layers = len(layers)
    d.n_groups, d.n_wsets = int(n_groups), int(n_wsets)
    d.group_stride = int(group_stride if group_stride is not None else (y if y is not None else heads[5]).shape[0])
    if tail is not None:
        t_first, t_gate, t_begin, t_dropped, t_yf = tail[:5]
        if len(tail) > 5 and tail[5] is not None:      # token -> row of the last layer's rowbias (a token space that is not in ray order)
            assert tail[5].dtype == torch.int32 and tail[5].is_contiguous() and tail[5].numel() >= t_gate.numel()
            d.tail_bias_row = _p(tail[5])
        assert t_gate.dtype == torch.float32 and t_begin.dtype == torch.int32 and t_dropped.dtype == torch.int32 and x_gather is not None
        d.tail_first, d.y_features, d.tail_gate, d.tail_dropped = int(t_first), int(t_yf), _p(t_gate), _p(t_dropped)
        d.tail_n_dropped = t_begin.data_ptr() + 4 * (t_begin.numel() - 1)
        d.tail_dropped_max, d.tail_tokens = int(t_dropped.numel()), int(t_gate.numel())
    if head is not None:
        h_layers, h_begin, h_dropped = head
        assert h_begin.dtype == torch.int32 and h_dropped.dtype == torch.int32 and x_gather is not None and combine is not None
        d.head_layers, d.tail_dropped = int(h_layers), _p(h_dropped)
        d.tail_n_dropped = h_begin.data_ptr() + 4 * (h_begin.numel() - 1)
        d.tail_dropped_max, d.tail_tokens = int(h_dropped.numel()), int(x.shape[0])
    d.group_rows = _p(group_rows)
    d.group_rows_clamp = int(group_rows_clamp if group_rows_clamp is not None else d.group_stride)
    d.group_begin = _p(group_begin)
    d.x, d.x_gather, d.x_save, d.y = _p(x), _p(x_gather), _p(x_save), _p(y)
    d.x_scale, d.x_relu = _p(x_scale), int(bool(x_relu))
    d.y_add, d.y_add_gather = _p(y_add), _p(y_add_gather)
    d.x_features = int(x_features)                 # (geometry 6 / 7: 128-feature rows under a zero-padded K = 256 first layer)
    d.x_k = int(x_k)                               # (... whose K loop stops at the real K)
    if sched is None and d.geometry >= 6 and not CHAINQ_STATIC:
        sched = chain_sched(x.device, d.tag)       # (launches of one role on one stream are ordered: they can share the counters)
    if sched is not None:
        assert sched.dtype == torch.int32 and sched.numel() >= 16
        d.sched = _p(sched)
    if combine is not None:
        cy, cds, cws, cg, cdg = combine[:5]
        assert cy.dtype == x.dtype and (cy.shape == y.shape or head is not None) and cg.dtype == torch.float32 and cdg.dtype == torch.float32
        d.comb_y, d.comb_dsig, d.comb_wsig, d.comb_gate, d.comb_dgate = _p(cy), _p(cds), _p(cws), _p(cg), _p(cdg)
        if len(combine) > 5 and combine[5] is not None:      # the sigma head's weight gradient += from the same pass (fused backward only)
            dws = combine[5]
            assert head is not None and dws.dtype == torch.float32 and dws.numel() == 256 and dws.is_contiguous()
            if packed_rows > 0:      # (packed slots: ceil(packed_rows / 256) + n_groups tiles = one group of packed_rows + 256 n_groups rows)
                nb = int(_lib.load().swn_chain_dwsig_workspace_bytes(1, int(packed_rows) + 256 * int(n_groups)))
            else:
                nb = int(_lib.load().swn_chain_dwsig_workspace_bytes(int(n_groups), int(d.group_rows_clamp)))
            ws = _dwsig_ws.get((x.device, nb))
            if ws is None:           # per-wave partial sums (zeroed and added up in a fixed order by the launch); never freed (graphs)
                ws = _dwsig_ws[(x.device, nb)] = torch.empty(nb // 4, dtype=torch.float32, device=x.device)
            d.comb_dwsig, d.comb_dwsig_ws = _p(dws), _p(ws)
    if heads is not None:
        hws, hbs, hwc, hbc, hnoise, hraw = heads
        assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (hws, hbs, hwc, hbc, hraw)) and hraw.shape[1] == 4
        assert hnoise is None or (hnoise.dtype == torch.float32 and hnoise.is_contiguous())
        d.heads_ws, d.heads_bs, d.heads_wc, d.heads_bc, d.heads_noise, d.heads_raw = _p(hws), _p(hbs), _p(hwc), _p(hbc), _p(hnoise), _p(hraw)
    for i, ly in enumerate(layers):
        L = d.layers[i]
        assert ly.w.dtype == x.dtype and hasattr(ly.w, "swn_nk"), "weights must come from ops.pack_weights (compute dtype)"
        L.w, L.b, L.save, L.mask = _p(ly.w), _p(ly.b), _p(ly.save), _p(ly.mask)
        L.rowbias, L.rows_per_bias = _p(ly.rowbias), ly.rows_per_bias
        L.n, L.k = ly.w.swn_nk
        L.relu, L.skip = ly.relu, int(ly.skip)
    call("swn_mlp_chain", C.byref(d), _stream())
    return y


_chain_sched = {}
_dwsig_ws = {}


def chain_sched(dev, key):
    """The tile-queue counters of a persistent chain launch (geometry 6 / 7): int32 [16], zero at creation and left zero by every launch.
    One tensor per (device, stream, key): launches that share one are ordered on their stream; give launches that may overlap on
    different streams different keys.  Never freed (a captured hipGraph holds the address)."""
    k = (dev, torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0, key)
    t = _chain_sched.get(k)
    if t is None:
        t = _chain_sched[k] = torch.zeros(16, dtype=torch.int32, device=dev)
    return t


_wgrad_ws = {}


def _wgrad_workspace(dev, nbytes: int):
    """One workspace per (device, stream) - launches on different streams may overlap -, grown to the largest request."""
    key = (dev, torch.cuda.current_stream().cuda_stream)
    held = _wgrad_ws.setdefault(key, [])
    for ws in held:
        if ws.numel() >= nbytes:
            return ws
    # a larger request: a NEW buffer next to the old ones, which are NEVER freed (a captured hipGraph may hold an old one's address
    # for as long as the process lives; a handful of growth steps at most - the sizes depend on the job count and the weight sets only)
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    held.insert(0, ws)
    return ws


def _multi_ws_bytes(n_jobs: int, n_wsets: int) -> int:
    return int(_lib.load().swn_wgrad_multi_workspace_bytes(int(n_jobs), int(n_wsets)))


def wgrad(a, b, dw, db=None, n_groups=1, n_wsets=1, group_stride=None, group_rows=None, group_rows_clamp=None, n_splits=8,
          tag=0, use_workspace=True, a_gather=None, b_gather=None):
    """dw [n_wsets, m_dim, n_dim] f32 += a^T b per group; db [n_wsets, n_dim] += colsum(b).
    a_gather / b_gather: read the rows of a / b through an index (the routing permutation) instead of a dispatched copy.
    With a workspace (default) the launch is the balanced stream kernel (swn_wgrad_multi: n_splits is ignored) whenever
    n_groups % n_wsets == 0; use_workspace=False adds the partial tiles with fp32 atomics (the row-split kernel)."""
    m_dim, n_dim = a.shape[1], b.shape[1]
    assert group_stride is not None or (a_gather is None and b_gather is None)
    if m_dim > 256 or n_dim > 256:      # wider than one 256 x 256 tile: column blocks of the operands, one launch
        return wgrad_batched([(a, b, dw, db, a_gather, b_gather)], n_groups, n_wsets, group_stride, group_rows, group_rows_clamp,
                             n_splits, tag)
    gs = int(group_stride if group_stride is not None else a.shape[0])
    ws, ws_bytes = None, 0
    if use_workspace:
        ws = _wgrad_workspace(a.device, max(int(n_groups) * int(n_splits) * (m_dim * n_dim + n_dim) * 4, _multi_ws_bytes(1, n_wsets)))
        ws_bytes = ws.numel()
    call("swn_wgrad", _p(a), _p(b), _p(a_gather), _p(b_gather), _dt(a), m_dim, n_dim, int(n_groups), int(n_wsets), gs, _p(group_rows),
         int(group_rows_clamp if group_rows_clamp is not None else gs), _p(dw), _p(db), int(n_splits), int(tag), _p(ws), ws_bytes, _stream())


def wgrad_multi(jobs, n_groups=1, n_wsets=1, group_stride=None, group_rows=None, group_rows_clamp=None, tag=0, group_begin=None):
    """jobs: tuples (a, b, dw, db, a_gather, b_gather) over ONE row grouping, each with its own widths (multiples of 32):
    the balanced stream launch (swn_wgrad_multi, include/swn.h) - up to 8 GEMMs per launch, the work cut into equal shares of the
    valid rows, deterministic reduction.  dw [n_wsets, m, n] f32 (accumulated into), db [n_wsets, n] or None.  Operands wider than
    256 features (the Mission Bay widths) are cut into 256-column blocks - one GEMM per (row block of dw, column block of dw) through
    the per-job leading dimensions - so packed row spaces (group_begin: the rows an expert-parallel rank received) work at any width."""
    a0 = jobs[0][0]
    gs = int(group_stride if group_stride is not None else a0.shape[0])
    esz = a0.element_size()
    gemms = []              # (a ptr, b ptr, a_gather, b_gather, dw ptr, db ptr, m, n, lda, ldb, ldw, dw_set_stride, db_set_stride)
    for (a, b, dw, db, ag, bg) in jobs:
        m, n = a.shape[1], b.shape[1]
        assert a.dtype == a0.dtype and b.dtype == a0.dtype and dw.shape[-2:] == (m, n) and dw.dtype == torch.float32
        bm, bn = min(m, 256), min(n, 256)
        assert m % bm == 0 and n % bn == 0, "operand widths above 256 must be multiples of 256"
        for i in range(0, m, bm):
            for j in range(0, n, bn):
                gemms.append((a.data_ptr() + i * esz, b.data_ptr() + j * esz, _p(ag), _p(bg), dw.data_ptr() + (i * n + j) * 4,
                              (db.data_ptr() + j * 4) if (db is not None and i == 0) else None, bm, bn, m, n, n, m * n, n))
    for i0 in range(0, len(gemms), 8):
        chunk = gemms[i0:i0 + 8]
        arr = (WgradJob * len(chunk))()
        for jb, (pa, pb, ag, bg, pdw, pdb, m, n, lda, ldb, ldw, dws, dbs) in zip(arr, chunk):
            jb.a, jb.b, jb.a_gather, jb.b_gather, jb.dw, jb.db = pa, pb, ag, bg, pdw, pdb
            jb.m_dim, jb.n_dim, jb.lda, jb.ldb, jb.ldw = m, n, lda, ldb, ldw
            jb.dw_set_stride, jb.db_set_stride = dws, dbs
        ws = _wgrad_workspace(a0.device, _multi_ws_bytes(len(chunk), n_wsets))
        call("swn_wgrad_multi", arr, len(chunk), _dt(a0), int(n_groups), int(n_wsets), gs, _p(group_rows),
             int(group_rows_clamp if group_rows_clamp is not None else gs), _p(group_begin), int(tag), _p(ws), ws.numel(), _stream())


def wgrad_batched(items, n_groups=1, n_wsets=1, group_stride=None, group_rows=None, group_rows_clamp=None, n_splits=8, tag=0):
    """items: tuples (a, b, dw, db, a_gather, b_gather) of identical shapes / grouping -> launches of up to 8 GEMM blocks
    (see wgrad).  Operands wider than 256 features are cut into 256-column blocks (swn_wgrad_blocks)."""
    a0, b0 = items[0][0], items[0][1]
    M, N = a0.shape[1], b0.shape[1]
    bm, bn = min(M, 256), min(N, 256)
    esz = a0.element_size()
    gs = int(group_stride if group_stride is not None else a0.shape[0])
    blocks = []
    for (a, b, dw, db, ag, bg) in items:
        assert a.shape[1] == M and b.shape[1] == N and a.dtype == a0.dtype and dw.shape[-2:] == (M, N)
        for i in range(0, M, bm):
            for j in range(0, N, bn):
                blocks.append((a.data_ptr() + i * esz, b.data_ptr() + j * esz, _p(ag), _p(bg), dw.data_ptr() + (i * N + j) * 4,
                               (db.data_ptr() + j * 4) if (db is not None and i == 0) else None))
    per = int(n_groups) * int(n_splits) * (bm * bn + bn) * 4
    ws = _wgrad_workspace(a0.device, max(8 * per, _multi_ws_bytes(8, n_wsets)))
    for i0 in range(0, len(blocks), 8):
        chunk = blocks[i0:i0 + 8]
        arr = (WgradItem * len(chunk))()
        for i, (pa, pb, ag, bg, pdw, pdb) in enumerate(chunk):
            arr[i].a, arr[i].b, arr[i].a_gather, arr[i].b_gather, arr[i].dw, arr[i].db = pa, pb, ag, bg, pdw, pdb
        call("swn_wgrad_blocks", arr, len(chunk), _dt(a0), bm, bn, M, N, N, M * N, N, int(n_groups), int(n_wsets), gs, _p(group_rows),
             int(group_rows_clamp if group_rows_clamp is not None else gs), int(n_splits), int(tag), _p(ws), ws.numel(), _stream())


def adam_step(param, grad, m, v, shadow, step: int, lr: float, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    n = param.numel()
    call("swn_adam_step", _p(param), _p(grad), _p(m), _p(v), _p(shadow), _dt(shadow) if shadow is not None else F32, n,
         float(lr), float(beta1), float(beta2), float(eps), int(step), float(grad_scale), _stream())


def grad_accum(acc, grad, scale: float):
    """acc += grad * scale (fp32; product and sum rounded separately): one micro-step's gradient into the accumulation window."""
    n = acc.numel()
    assert grad.numel() == n and acc.dtype == grad.dtype == torch.float32 and acc.is_contiguous() and grad.is_contiguous()
    call("swn_grad_accum", _p(acc), _p(grad), n, float(scale), _stream())
    return acc


def adam_accum_step(param, acc, grad, m, v, shadow, step: int, lr: float, beta1=0.9, beta2=0.999, eps=1e-8, accum_scale=1.0,
                    grad_scale=1.0):
    """The last micro-step of an accumulation window: Adam on (acc + grad * accum_scale) * grad_scale - grad None: on acc * grad_scale -
    and acc cleared, in one pass (the bits of grad_accum followed by adam_step)."""
    n = param.numel()
    assert acc.numel() == n and (grad is None or grad.numel() == n)
    call("swn_adam_accum_step", _p(param), _p(acc), _p(grad), _p(m), _p(v), _p(shadow), _dt(shadow) if shadow is not None else F32, n,
         float(lr), float(beta1), float(beta2), float(eps), int(step), float(accum_scale), float(grad_scale), _stream())


# ---- the finite guard (csrc/finite_guard.hip; the guarded accumulation launches: csrc/accum.hip)
def finite_guard(metrics, psnr_slot: int, ok, skipped=None):
    """ok[0] = 1 iff every metric is finite (+inf passes in slot psnr_slot; -1: no such slot); skipped[0] += 1 - ok.  One launch."""
    assert metrics.dtype == torch.float32 and ok.dtype == torch.int32 and ok.numel() == 1
    assert skipped is None or (skipped.dtype == torch.int64 and skipped.numel() == 1)
    call("swn_finite_guard", _p(metrics), metrics.numel(), int(psnr_slot), _p(ok), _p(skipped), _stream())
    return ok


_bias_tables = {}


def adam_bias_table(device, beta1=0.9, beta2=0.999):
    """The device table [rows, 2] of Adam's bias corrections per step count that the guarded launches index (swn_adam_bias_table:
    computed on the host by the expressions of swn_adam_step).  One per device and pair of betas, made on first use - a host-to-device
    copy, so before a capture: set_check_finite makes the table of the default betas, a caller with other betas calls this first."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())      # "cuda" and "cuda:0" are one table
    key = (device, float(beta1), float(beta2))
    if key not in _bias_tables:
        # the corrections are exactly 1 once beta^t < 2^-25 (half an ulp of 1): t > 25 ln 2 / -ln(beta), + 1 % and a few rows of slack
        beta = float(torch.tensor(max(float(beta1), float(beta2)), dtype=torch.float32))      # (the fp32 value the launch is handed)
        if not 0.0 <= beta < 1.0:
            raise ValueError(f"adam_bias_table: betas must lie in [0, 1), got {beta1}, {beta2}")
        cap = 64 if beta == 0.0 else int(1.01 * 25 * math.log(2.0) / -math.log(beta)) + 64
        host = torch.empty(cap, 2, dtype=torch.float32)
        rows = C.c_long(0)
        call("swn_adam_bias_table", float(beta1), float(beta2), C.c_void_p(host.data_ptr()), cap, C.byref(rows))
        _bias_tables[key] = host[: rows.value].to(device).contiguous()
    return _bias_tables[key]


def adam_step_guarded(param, grad, m, v, shadow, step_state, ok, lr: float, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    """adam_step under the guard's flag: ok[0] = 1 takes optimizer step step_state[0] + 1 (the bits of adam_step) and advances
    step_state[0]; ok[0] = 0 changes nothing.  step_state: int32[2] (see include/swn.h)."""
    n = param.numel()
    assert grad.numel() == m.numel() == v.numel() == n and step_state.dtype == torch.int32 and step_state.numel() == 2
    assert ok.dtype == torch.int32 and ok.numel() == 1 and (shadow is None or shadow.numel() == n)
    tab = adam_bias_table(param.device, beta1, beta2)
    call("swn_adam_step_guarded", _p(param), _p(grad), _p(m), _p(v), _p(shadow), _dt(shadow) if shadow is not None else F32, n,
         float(lr), float(beta1), float(beta2), float(eps), _p(tab), tab.shape[0], _p(step_state), float(grad_scale), _p(ok), _stream())


def grad_accum_guarded(acc, grad, scale: float, ok):
    """grad_accum under the guard's flag; ok[0] = 0 clears acc instead (a flagged micro-step discards the window's partial sums)."""
    n = acc.numel()
    assert grad.numel() == n and acc.dtype == grad.dtype == torch.float32 and ok.dtype == torch.int32 and ok.numel() == 1
    call("swn_grad_accum_guarded", _p(acc), _p(grad), n, float(scale), _p(ok), _stream())
    return acc


def adam_accum_step_guarded(param, acc, grad, m, v, shadow, step_state, ok, lr: float, beta1=0.9, beta2=0.999, eps=1e-8,
                            accum_scale=1.0, grad_scale=1.0):
    """adam_accum_step under the guard's flag (step count as in adam_step_guarded); ok[0] = 0 clears acc and changes nothing else."""
    n = param.numel()
    assert acc.numel() == m.numel() == v.numel() == n and (grad is None or grad.numel() == n)
    assert step_state.dtype == torch.int32 and step_state.numel() == 2 and ok.dtype == torch.int32 and ok.numel() == 1
    assert shadow is None or shadow.numel() == n
    tab = adam_bias_table(param.device, beta1, beta2)
    call("swn_adam_accum_step_guarded", _p(param), _p(acc), _p(grad), _p(m), _p(v), _p(shadow),
         _dt(shadow) if shadow is not None else F32, n, float(lr), float(beta1), float(beta2), float(eps), _p(tab), tab.shape[0],
         _p(step_state), float(accum_scale), float(grad_scale), _p(ok), _stream())


# ---- image metrics (csrc/ssim.hip; the user-facing layer: metrics.py)
_ssim_ws = {}


def ssim_fwd(pred, target, taps, c1: float, c2: float, mask=None, map_out=None, out=None):
    """SSIM and squared error of image pairs in one pass (swn_ssim_fwd): pred, target fp32 [n, A, B, C] channels last, C <= 4; taps: the
    window, a host fp32 tensor of odd length <= 15; mask uint8 [n, A, B] or None -> out [n, 4] = (ssim, mse, ssim over the masked
    pixels, mse over them; nan without a mask or with an empty one).  map_out [n, A, B, C]: the SSIM map.  Two launches, no host read.
    The workspace is one per (device, stream, shape), never freed (a captured hipGraph holds its address)."""
    assert pred.dim() == 4 and pred.shape == target.shape and pred.dtype == target.dtype == torch.float32
    n, A, B, Cc = pred.shape
    assert taps.device.type == "cpu" and taps.dtype == torch.float32 and taps.is_contiguous() and taps.dim() == 1
    assert mask is None or (mask.dtype == torch.uint8 and mask.shape == (n, A, B))
    assert map_out is None or (map_out.dtype == torch.float32 and map_out.shape == pred.shape)
    if out is None:
        out = torch.empty(n, 4, dtype=torch.float32, device=pred.device)
    assert out.dtype == torch.float32 and out.shape == (n, 4)
    key = (pred.device, torch.cuda.current_stream().cuda_stream, n, A, B)
    ws = _ssim_ws.get(key)
    if ws is None:
        need = C.c_size_t(0)
        call("swn_ssim_workspace_bytes", n, A, B, C.byref(need))
        ws = _ssim_ws[key] = torch.empty(need.value, dtype=torch.uint8, device=pred.device)
    call("swn_ssim_fwd", _p(pred), _p(target), _p(mask), n, A, B, Cc, C.c_void_p(taps.data_ptr()), taps.numel(), float(c1), float(c2),
         _p(map_out), _p(ws), ws.numel(), _p(out), _stream())
    return out


# ---- rays from cameras (csrc/raygen.hip; the user-facing layer: rays.py)
def _alt_arg(ray_altitude_range):
    """-> a host float[2] for the altitude planes, or None."""
    if ray_altitude_range is None:
        return None
    a = [float(v) for v in ray_altitude_range]
    if len(a) != 2:
        raise ValueError(f"ray_altitude_range must be a pair, got {len(a)} values")
    return (C.c_float * 2)(*a)


def _rays_out(out, n: int, dev, lead=()):
    shape = tuple(lead) + (n, 8)
    if out is None:
        return torch.empty(*shape, dtype=torch.float32, device=dev)
    if out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous() or not out.is_cuda:
        raise ValueError(f"out must be a contiguous fp32 device tensor {shape}, got {out.dtype} {tuple(out.shape)}")
    return out


def rays_from_camera(camera: "_lib.Camera", near: float, far: float, ray_altitude_range, pixel_begin: int, n: int, out=None,
                     image_indices_out=None, device=None):
    """swn_rays_from_camera: the rays [n, 8] of the row-major pixels [pixel_begin, pixel_begin + n) of one camera (a _lib.Camera, passed
    by value), written into `out` when given; image_indices_out: an int64 [n] filled with the camera's image index.  One launch."""
    dev = out.device if out is not None else torch.device("cuda" if device is None else device)
    out = _rays_out(out, n, dev)
    ii = image_indices_out
    if ii is not None and (ii.dtype != torch.int64 or tuple(ii.shape) != (n,) or not ii.is_contiguous() or ii.device != out.device):
        raise ValueError(f"image_indices_out must be a contiguous int64 [{n}] tensor on {out.device}")
    with torch.cuda.device(out.device):
        call("swn_rays_from_camera", C.byref(camera), float(near), float(far), _alt_arg(ray_altitude_range), int(pixel_begin), int(n),
             _p(out), _p(ii), _stream())
    return out


def ray_directions(W: int, H: int, fx: float, fy: float, cx: float, cy: float, center_pixels: bool, device):
    """swn_ray_directions -> the camera-space unit directions [H, W, 3]."""
    out = torch.empty(int(H), int(W), 3, dtype=torch.float32, device=device)
    with torch.cuda.device(out.device):
        call("swn_ray_directions", int(W), int(H), float(fx), float(fy), float(cx), float(cy), int(bool(center_pixels)), _p(out), _stream())
    return out


def rays_from_directions(directions, c2w, near: float, far: float, ray_altitude_range, out=None):
    """swn_rays_from_directions: directions [n, 3] and poses c2w [K, 3, 4], both fp32 on the device -> rays [K, n, 8]."""
    assert directions.dtype == c2w.dtype == torch.float32 and directions.dim() == 2 and directions.shape[1] == 3
    assert c2w.dim() == 3 and tuple(c2w.shape[1:]) == (3, 4) and c2w.device == directions.device
    if c2w.data_ptr() % 16:
        c2w = c2w.clone()
    n, K = directions.shape[0], c2w.shape[0]
    out = _rays_out(out, n, directions.device, (K,))
    with torch.cuda.device(out.device):
        call("swn_rays_from_directions", _p(directions), _p(c2w), K, n, float(near), float(far), _alt_arg(ray_altitude_range), _p(out),
             _stream())
    return out


def rays_from_pixels(table, cam_idx, pix_idx, W: int, H: int, center_pixels: bool, near: float, far: float, ray_altitude_range, out=None):
    """swn_rays_from_pixels: table [M, 16] fp32 (c2w, fx, fy, cx, cy per camera), cam_idx / pix_idx [n] both int32 or both int64 ->
    rays [n, 8].  Index values are not checked (rays.pixel_rays(check=True) does)."""
    assert table.dtype == torch.float32 and table.dim() == 2 and table.shape[1] == 16
    assert cam_idx.dtype == pix_idx.dtype and cam_idx.shape == pix_idx.shape and cam_idx.dim() == 1
    assert cam_idx.device == pix_idx.device == table.device
    n = cam_idx.shape[0]
    out = _rays_out(out, n, table.device)
    cp, i64 = _idx_arg(cam_idx)
    pp, _ = _idx_arg(pix_idx)
    with torch.cuda.device(out.device):
        call("swn_rays_from_pixels", _p(table), table.shape[0], cp, pp, i64, n, int(W), int(H), int(bool(center_pixels)), float(near),
             float(far), _alt_arg(ray_altitude_range), _p(out), _stream())
    return out


# ---- rays the NeRF-dataset way (csrc/raygen_nerf.hip; the user-facing layer: nerf_rays.py)
def _radii_out(out, n: int, dev):
    if out is None:
        return torch.empty(n, 1, dtype=torch.float32, device=dev)
    if out.dtype != torch.float32 or tuple(out.shape) != (n, 1) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"radii_out must be a contiguous fp32 tensor ({n}, 1) on {dev}, got {out.dtype} {tuple(out.shape)}")
    return out


def _origin_arg(scene_origin):
    """-> a host double[3] for the globe's centre, or None."""
    if scene_origin is None:
        return None
    o = [float(v) for v in scene_origin]
    if len(o) != 3:
        raise ValueError(f"scene_origin must have three values, got {len(o)}")
    return (C.c_double * 3)(*o)


def nerf_rays_from_camera(camera: "_lib.NerfCamera", mode: int, near: float, far: float, focal: float, near_ndc: float, pixel_begin: int,
                          n: int, out=None, device=None):
    """swn_nerf_rays_from_camera: the rays [n, 8] of the row-major pixels [pixel_begin, pixel_begin + n) of one camera (a
    _lib.NerfCamera, passed by value) in mode _lib.NERF_RAW / NERF_NORMALIZED / NERF_NDC, written into `out` when given.  One launch."""
    dev = out.device if out is not None else torch.device("cuda" if device is None else device)
    out = _rays_out(out, n, dev)
    with torch.cuda.device(out.device):
        call("swn_nerf_rays_from_camera", C.byref(camera), int(mode), float(near), float(far), float(focal), float(near_ndc),
             int(pixel_begin), int(n), _p(out), _stream())
    return out


def nerf_rays_bungee(camera: "_lib.NerfCamera", scene_scaling_factor: float, scene_origin, ray_nearfar: int, pixel_begin: int, n: int,
                     out=None, radii_out=None, device=None):
    """swn_nerf_rays_bungee: rays [n, 8] with per-ray near / far (_lib.NERF_SPHERE / NERF_FLAT) and the mip radii [n, 1].  One launch."""
    given = out if out is not None else radii_out
    dev = given.device if given is not None else torch.device("cuda" if device is None else device)
    out = _rays_out(out, n, dev)
    radii = _radii_out(radii_out, n, out.device)
    with torch.cuda.device(out.device):
        call("swn_nerf_rays_bungee", C.byref(camera), float(scene_scaling_factor), _origin_arg(scene_origin), int(ray_nearfar),
             int(pixel_begin), int(n), _p(out), _p(radii), _stream())
    return out, radii


def nerf_rays_from_pixels(table, cam_idx, pix_idx, W: int, H: int, mode: int, near: float, far: float, focal: float, near_ndc: float,
                          scene_scaling_factor: float, scene_origin, out=None, radii_out=None):
    """swn_nerf_rays_from_pixels: table [M, 16] fp32 (c2w, fx, fy, cx, cy per camera), cam_idx / pix_idx [n] both int32 or both int64,
    any _lib.NERF_* mode -> rays [n, 8], and radii [n, 1] in the bungee modes (None otherwise).  Index values are not checked."""
    assert table.dtype == torch.float32 and table.dim() == 2 and table.shape[1] == 16
    assert cam_idx.dtype == pix_idx.dtype and cam_idx.shape == pix_idx.shape and cam_idx.dim() == 1
    assert cam_idx.device == pix_idx.device == table.device
    n = cam_idx.shape[0]
    out = _rays_out(out, n, table.device)
    radii = _radii_out(radii_out, n, table.device) if mode in (_lib.NERF_BUNGEE_SPHERE, _lib.NERF_BUNGEE_FLAT) else None
    cp, i64 = _idx_arg(cam_idx)
    pp, _ = _idx_arg(pix_idx)
    with torch.cuda.device(out.device):
        call("swn_nerf_rays_from_pixels", _p(table), table.shape[0], cp, pp, i64, n, int(W), int(H), int(mode), float(near), float(far),
             float(focal), float(near_ndc), float(scene_scaling_factor), _origin_arg(scene_origin), _p(out), _p(radii), _stream())
    return out, radii


def nerf_rays_dirs(camera_row, W: int, H: int):
    """swn_nerf_rays_dirs: camera_row [16] fp32 on the device (c2w, fx, fy, cx, cy) -> raw rays_o, rays_d, each [H, W, 3]."""
    assert camera_row.dtype == torch.float32 and camera_row.numel() == 16 and camera_row.is_contiguous() and camera_row.is_cuda
    if camera_row.data_ptr() % 16:
        camera_row = camera_row.clone()
    o = torch.empty(int(H), int(W), 3, dtype=torch.float32, device=camera_row.device)
    d = torch.empty_like(o)
    with torch.cuda.device(o.device):
        call("swn_nerf_rays_dirs", _p(camera_row), int(W), int(H), _p(o), _p(d), _stream())
    return o, d


def nerf_ndc(rays_o, rays_d, W: int, H: int, focal: float, near: float):
    """swn_nerf_ndc: ndc_rays over contiguous fp32 device tensors rays_o, rays_d [n, 3] -> (o, d), each [n, 3]."""
    assert rays_o.dtype == rays_d.dtype == torch.float32 and rays_o.shape == rays_d.shape and rays_o.dim() == 2 and rays_o.shape[1] == 3
    assert rays_o.is_contiguous() and rays_d.is_contiguous() and rays_o.device == rays_d.device and rays_o.is_cuda
    o, d = torch.empty_like(rays_o), torch.empty_like(rays_d)
    with torch.cuda.device(o.device):
        call("swn_nerf_ndc", _p(rays_o), _p(rays_d), rays_o.shape[0], int(W), int(H), float(focal), float(near), _p(o), _p(d), _stream())
    return o, d


def cast(src, dst):
    call("swn_cast", _p(src), _p(dst), _dt(dst), src.numel(), _stream())
    return dst


def cast_transpose(src, dst):
    """src [B, R, C] f32 -> dst [B, C, R] (dst dtype)"""
    B, R, Cc = src.shape
    call("swn_cast_transpose", _p(src), _p(dst), _dt(dst), B, R, Cc, _stream())
    return dst
