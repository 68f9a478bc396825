"""Plain torch restatement, in float64, of what a top-k gate and use_load_importance_loss add to the router (switch_nerf_amd/csrc/route.hip:
gate_logits / load_importance_* / topk_gate_bwd, elementwise.hip: gate_bwd_kernel's dense operands), and the seeded inputs both test files
build them on.  Every reference takes the exact values the kernel sees (a 16-bit input is rounded to 16 bits first, then widened) and computes in
`dtype` - float64 for the reference itself, float32 for the reference's own rounding error, which the tolerances of the GPU tests are derived
from (tolerance()).  Shared by tests/test_topk_gate_refs_cpu.py and tests/test_topk_gate_kernels_gpu.py; imports neither the library nor a GPU."""
import math

import torch

EPS = torch.finfo(torch.float32).eps            # the clamp of the top-k normalisation (tutel_fast_dispatch.py:204-206)
ULP = 2.0 ** -23                                # one fp32 ulp of 1


def gate_logits_ref(g, wg, noise, scale, dtype=torch.float64):
    """g @ wg.T + scale * noise (noise may be None)."""
    out = g.to(dtype) @ wg.to(dtype).t()
    return out if noise is None else out + float(scale) * noise.to(dtype)


def load_importance_ref(logits, add, idx_last, sigma, d_l=1.0, scores=None, dtype=torch.float64):
    """scores = softmax(logits), logits_w = logits + add, thr = logits_w.gather(idx_last), then the reference formula
    (tutel_fast_dispatch.py:152-174): l = (cv2(Imp) + cv2(Load)) / 2, Imp_e = sum_t scores, Load_e = sum_t Normal(0, sigma).cdf(scores - thr),
    cv2(v) = v.var() / (v.mean()^2 + 1e-10).  scores (optional): the rounded probabilities the kernel is handed - they replace the softmax's
    values, the gradient still runs through the softmax.
    -> dict(l, d_logits = d_l * dl/dlogits, d_imp = dl/dImp, d_load = dl/dLoad, imp, load, z = (scores - thr) / sigma)."""
    x = logits.detach().to(dtype).requires_grad_(True)
    sc = torch.softmax(x, 1)
    if scores is not None:
        sc = sc + (scores.to(dtype) - sc).detach()
    thr = (x + add.to(dtype)).gather(1, idx_last.long().view(-1, 1))
    z = (sc - thr) / sigma
    imp = sc.sum(0)
    load = (0.5 * (1 + torch.erf(z / math.sqrt(2.0)))).sum(0)
    cv2 = lambda v: v.var() / (v.mean() ** 2 + 1e-10)
    l = (cv2(imp) + cv2(load)) / 2.0
    d_logits, = torch.autograd.grad(l, x, retain_graph=True)
    imp_l, load_l = imp.detach().requires_grad_(True), load.detach().requires_grad_(True)
    d_imp, d_load = torch.autograd.grad((cv2(imp_l) + cv2(load_l)) / 2.0, (imp_l, load_l))
    return dict(l=l.detach(), d_logits=float(d_l) * d_logits, d_imp=d_imp, d_load=d_load, imp=imp.detach(), load=load.detach(), z=z.detach())


def topk_norm_fwd_ref(gates, idx, dtype=torch.float64):
    """The normalised gates [K, P] of the choices idx [K, P]: g_j / clamp(sum_j g_j, min=eps) for K > 1, g_j itself for K = 1."""
    gs = gates.to(dtype).gather(1, idx.long().t())
    if idx.shape[0] > 1:
        gs = gs / torch.clamp(gs.sum(1, keepdim=True), min=EPS)
    return gs.t()


def topk_norm_bwd_ref(gates, idx, d_gnorm, dtype=torch.float64):
    """d_gnorm [K, P] -> the gradient [P, E] w.r.t. the gates, by autograd through topk_norm_fwd_ref (zero outside a token's K experts)."""
    g = gates.detach().to(dtype).requires_grad_(True)
    (topk_norm_fwd_ref(g, idx, dtype) * d_gnorm.to(dtype)).sum().backward()
    return g.grad


def gate_bwd_dense_ref(g, ln_w, ln_b, wg, idx, d_gmax, d_probs, d_logits_add, counts, coef, seg_tokens, dtype=torch.float64):
    """Autograd through the optional LayerNorm (eps 1e-5), pr = softmax(xn @ wg.T) and
    sum(pr * (coef[seg] * counts[seg] + onehot(idx) * d_gmax + d_probs)) + sum(logits * d_logits_add); d_gmax / d_probs / d_logits_add may be None.
    -> dict(dg, d_wg, d_ln_w, d_ln_b, pr)."""
    P, G = g.shape
    E = wg.shape[0]
    x = g.detach().to(dtype).requires_grad_(True)
    W = wg.detach().to(dtype).requires_grad_(True)
    lw = ln_w.detach().to(dtype).requires_grad_(True) if ln_w is not None else None
    lb = ln_b.detach().to(dtype).requires_grad_(True) if ln_w is not None else None
    xn = torch.nn.functional.layer_norm(x, (G,), lw, lb, 1e-5) if ln_w is not None else x
    logits = xn @ W.t()
    pr = torch.softmax(logits, 1)
    dp = coef.to(dtype).repeat_interleave(seg_tokens)[:, None] * counts.to(dtype).repeat_interleave(seg_tokens, 0)
    if d_gmax is not None:
        dp = dp + torch.nn.functional.one_hot(idx.long(), E).to(dtype) * d_gmax.to(dtype)[:, None]
    if d_probs is not None:
        dp = dp + d_probs.to(dtype)
    loss = (pr * dp).sum()
    if d_logits_add is not None:
        loss = loss + (logits * d_logits_add.to(dtype)).sum()
    loss.backward()
    return dict(dg=x.grad, d_wg=W.grad, d_ln_w=lw.grad if lw is not None else None, d_ln_b=lb.grad if lb is not None else None, pr=pr.detach())


def tolerance(ref32, ref64):
    """The tolerance of a float comparison that is not one of the project's own: 8 x the error of the plain fp32 torch evaluation of the
    reference (ref32) against float64 (ref64), at least 4 fp32 ulps of max|ref|.  8 = the kernel's other summation order (256-way strided
    partials, then blocks, against torch's pairwise sum) and erff / __expf being a few ulps off libm.  -> (tolerance, the fp32 error)."""
    ref64 = ref64.double()
    err32 = (ref32.double() - ref64).abs().max().item()
    return max(8.0 * err32, 4.0 * ULP * ref64.abs().max().item()), err32


# ---- gate_logits: (dtype, E, gate_dim, P, noise) - every E of {1, 2, 8, 13, 16}, gate_dim of {1, 63, 64, 65, 256, 512, 1000} (the 64-lane
# feature loop: under one pass, one short, exact, one over, several), P of {1, 5, 2 * 16384 + 3} (past one grid stride) at least once
P_STRIDE = 2 * 16384 + 3
GATE_LOGITS_CASES = [
    ("f32", 1, 1, 1, False), ("f32", 2, 63, 5, True), ("bf16", 8, 64, 5, False), ("f32", 13, 65, 5, True), ("bf16", 16, 256, 1, True),
    ("f32", 8, 512, P_STRIDE, True), ("bf16", 13, 1000, 5, False), ("f32", 16, 1000, 5, True), ("bf16", 2, 65, P_STRIDE, False),
    ("bf16", 1, 63, 1, True), ("f32", 13, 256, P_STRIDE, False), ("f32", 16, 64, 5, False),
]
NOISE_SCALE = 0.125


def gate_logits_inputs(case):
    """-> (g, wg, noise or None): g already rounded to the case's dtype, everything on the CPU."""
    kind, E, G, P, with_noise = case
    gen = torch.Generator().manual_seed(1000 + 31 * E + 7 * G + P % 997)
    g = torch.randn(P, G, generator=gen) * 1.3 + 0.4
    g = g.to(torch.bfloat16) if kind == "bf16" else g
    wg = torch.randn(E, G, generator=gen) * 0.3
    noise = torch.randn(P, E, generator=gen) if with_noise else None
    return g, wg, noise


# ---- load / importance loss: (P, E, k, sigma * E) - P of {1, 255, 257, 4099, 131072 + 300} (one thread, one block short / over, several
# blocks, past the 512-block stride), E of {2, 3, 8, 13, 16}, the threshold the k-th largest noisy logit for k of {1, 2, E}, sigma of
# {1, 0.5, 2} / E, each at least once
P_LI_STRIDE = 131072 + 300
LOAD_IMPORTANCE_CASES = [
    (1, 2, 1, 1.0), (255, 3, 2, 0.5), (257, 8, 8, 2.0), (4099, 13, 2, 1.0), (P_LI_STRIDE, 16, 1, 0.5), (P_LI_STRIDE, 8, 2, 1.0),
    (4099, 16, 16, 2.0), (257, 2, 2, 0.5),
]
SATURATED_CASE = (4099, 8, 2, 0.05)          # sigma = 0.05 / E and no threshold shift: the cdf is 0 or 1 almost everywhere
D_L = -2.5


def load_importance_inputs(case, shift=True):
    """The well-conditioned inputs of a load / importance case -> dict(logits, scores, logits_w (all fp32: what the kernel is handed),
    add (float64: logits_w - logits, exact), idx_last int32, sigma).  logits = 0.3 randn + a per-expert slope over +-0.3; add = sigma randn
    (gate_noise / E = sigma) + a per-token constant that puts the k-th largest noisy logit within +-2 sigma of 1 / E (shift=False: no
    constant - the saturated case)."""
    P, E, k, sE = case
    sigma = sE / E
    gen = torch.Generator().manual_seed(2000 + 17 * E + k + P % 991)
    logits = (0.3 * torch.randn(P, E, generator=gen, dtype=torch.float64) + torch.linspace(-0.3, 0.3, E, dtype=torch.float64)).float()
    noisy = logits.double() + sigma * torch.randn(P, E, generator=gen, dtype=torch.float64)
    if shift:
        target = 1.0 / E + (torch.rand(P, generator=gen, dtype=torch.float64) * 4 - 2) * sigma
        noisy = noisy + (target - noisy.topk(k, dim=1).values[:, -1])[:, None]
    logits_w = noisy.float()
    idx_last = logits_w.topk(k, dim=1).indices[:, -1].to(torch.int32)
    scores = torch.softmax(logits.double(), 1).float()
    return dict(logits=logits, scores=scores, logits_w=logits_w, add=logits_w.double() - logits.double(), idx_last=idx_last, sigma=sigma)


def load_importance_refs(inp):
    """-> (float64 reference, its plain fp32 evaluation) on the inputs of load_importance_inputs."""
    a = (inp["logits"], inp["add"], inp["idx_last"], inp["sigma"], D_L, inp["scores"])
    return load_importance_ref(*a, dtype=torch.float64), load_importance_ref(*a, dtype=torch.float32)


# ---- top-k normalisation backward: (E, K) x P
TOPK_CASES = [(1, 1), (2, 2), (8, 1), (8, 2), (13, 3), (16, 16), (64, 5), (64, 64)]
TOPK_TOKENS = [1, 257, 1000]


def topk_inputs(E, K, P):
    """-> (gates fp32 [P, E] softmax rows, the last of them with exact ties when P > 1; d_gnorm fp32 [K, P])."""
    gen = torch.Generator().manual_seed(3000 + 101 * E + 11 * K + P)
    gates = torch.softmax(1.5 * torch.randn(P, E, generator=gen, dtype=torch.float64), 1).float()
    if P > 1 and E > 1:
        gates[-1] = gates[-1, 0]                 # every gate of the row equal: ties all the way down
        if E > 2:
            gates[-2, 1] = gates[-2, 0]          # one exact tie among random gates
    return gates, torch.randn(K, P, generator=gen)


def topk_special_rows(E):
    """Hand-built rows [3, E] (E >= 2): all gates 1e-9 (any K <= 64 of them sum below eps: clamped); two gates of exactly 2^-24 and zeros
    (the K largest sum to exactly eps: not clamped); the same with 2^-25 (sum eps / 2: clamped)."""
    r = torch.zeros(3, E)
    r[0] = 1e-9
    r[1, :2] = 2.0 ** -24
    r[2, :2] = 2.0 ** -25
    return r
