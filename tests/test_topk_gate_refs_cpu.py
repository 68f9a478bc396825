"""The float64 references of tests/topk_gate_ref.py against what the suite already trusts (the CPU oracle), the conditioning of the inputs
the GPU tests of the load / importance loss run on, and the references' own fp32 rounding error - the figure the GPU tolerances are 8 x of
(topk_gate_ref.tolerance; the table is in profiles/r11_topk_gate_kernel_parity.md).  No GPU, no library."""
import numpy as np
import pytest
import torch

import topk_gate_ref as R
from oracle import switchnerf_oracle as O

LI_CASES = R.LOAD_IMPORTANCE_CASES
_cache = {}


def li(case, shift=True):
    """Inputs and (fp64, fp32) references of a case, computed once."""
    key = (case, shift)
    if key not in _cache:
        inp = R.load_importance_inputs(case, shift)
        _cache[key] = (inp,) + R.load_importance_refs(inp)
    return _cache[key]


@pytest.mark.parametrize("case", LI_CASES + [R.SATURATED_CASE])
def test_load_importance_ref_equals_the_oracle(case):
    """load_importance_ref's loss = oracle.load_importance_loss on the same inputs: to 1e-5 relative (the oracle casts its inputs to fp32), and to
    1e-12 against the same formula with torch.distributions' own Normal.cdf (the reference's form, tutel_fast_dispatch.py:156-162) in float64."""
    P, E, k, sE = case
    inp, r64, _ = li(case, shift=case != R.SATURATED_CASE)
    thr = inp["logits_w"].gather(1, inp["idx_last"].long()[:, None])
    l32 = O.load_importance_loss(inp["scores"], thr, E, sE).double().item()
    sc = inp["scores"].double()
    load = torch.distributions.Normal(torch.zeros(1, dtype=torch.float64), torch.tensor([sE / E], dtype=torch.float64)).cdf(sc - thr.double()).sum(0)
    cv2 = lambda v: v.var() / (v.mean() ** 2 + 1e-10)
    l_dist = ((cv2(sc.sum(0)) + cv2(load)) / 2).item()
    l = r64["l"].item()
    assert abs(l_dist - l) <= 1e-12 * max(1.0, abs(l))
    if case != R.SATURATED_CASE:          # (saturated: the fp32 loss is ill-conditioned - no relative claim)
        assert abs(l32 - l) <= 1e-5 * abs(l)
        assert 0.005 <= l <= 2.0          # the loss is O(0.01 ... 1) on these inputs


@pytest.mark.parametrize("case", LI_CASES)
def test_load_importance_inputs_are_well_conditioned(case):
    """A condition on the inputs, not on the kernel: the cdf is unsaturated for at least a quarter of the (token, expert) pairs and no expert's
    load vanishes.  (Where the cdf saturates everywhere a plain fp32 evaluation is already 2e-3 off float64.)"""
    P, E, k, sE = case
    inp, r64, _ = li(case)
    assert (r64["z"].abs() < 3).double().mean().item() >= 0.25
    assert (r64["load"] >= 0.01 * P).all()
    # the threshold is the k-th largest noisy logit and lies within 2 sigma of 1 / E
    thr = inp["logits_w"].gather(1, inp["idx_last"].long()[:, None])[:, 0]
    assert torch.equal(thr, inp["logits_w"].topk(k, dim=1).values[:, -1])
    assert ((thr.double() - 1.0 / E).abs() <= 2 * inp["sigma"] + 1e-6).all()
    assert torch.equal((inp["logits"].double() + inp["add"]).float(), inp["logits_w"])


def test_load_importance_gradients_by_central_differences():
    """d_logits (through the softmax AND the threshold entry) and dl/dImp, dl/dLoad of the reference against central differences in float64."""
    case = (255, 3, 2, 0.5)
    inp = R.load_importance_inputs(case)
    r = R.load_importance_ref(inp["logits"], inp["add"], inp["idx_last"], inp["sigma"], R.D_L)
    h = 1e-6
    for t, e in ((0, 0), (7, int(inp["idx_last"][7])), (100, 2), (254, int(inp["idx_last"][254]))):
        lp = []
        for s in (+h, -h):
            x = inp["logits"].double().clone()
            x[t, e] += s
            lp.append(R.load_importance_ref(x, inp["add"], inp["idx_last"], inp["sigma"])["l"].item())
        fd = R.D_L * (lp[0] - lp[1]) / (2 * h)
        assert abs(fd - r["d_logits"][t, e].item()) <= 1e-6 * max(1e-3, abs(fd))
    cv2 = lambda v: v.var() / (v.mean() ** 2 + 1e-10)
    for name, grad, other in (("imp", r["d_imp"], r["load"]), ("load", r["d_load"], r["imp"])):
        v = r[name]
        for e in range(3):
            vp, vm = v.clone(), v.clone()
            vp[e] += h * v[e]
            vm[e] -= h * v[e]
            fd = 0.5 * (cv2(vp) - cv2(vm)).item() / (2 * h * v[e].item())
            assert abs(fd - grad[e].item()) <= 1e-6 * grad.abs().max().item()


@pytest.mark.parametrize("E,K", [(2, 2), (8, 1), (8, 2), (13, 3), (16, 16)])
def test_topk_normalisation_equals_the_oracle_layer(E, K):
    """topk_norm_fwd_ref / topk_norm_bwd_ref against oracle.moe_layer_topk: with expert e an identity on feature e alone and rows of ones,
    the layer's output IS its normalised gates gs (y[t, idx_j] = gs_j), and the gradient it hands its `gates` is the normalisation's."""
    P = 257
    gen = torch.Generator().manual_seed(5)
    gate_in, wg = torch.randn(P, 24, generator=gen), torch.randn(E, 24, generator=gen) * 0.3
    W = [torch.diag_embed(torch.eye(E))]                       # [E, E, E]: expert e keeps feature e
    B = [torch.zeros(E, 1, E)]
    gi = gate_in.clone().requires_grad_(True)
    y, _, r, gates = O.moe_layer_topk(torch.ones(P, E), gi, wg, W, B, (), K, float(E), False)
    idx = torch.from_numpy(r["idx"])
    assert (torch.from_numpy(r["loc"]) < r["capacity"]).all()
    gn = R.topk_norm_fwd_ref(gates.detach(), idx)
    want = torch.zeros(P, E, dtype=torch.float64).scatter_(1, idx.long().t(), gn.t())
    assert (y.detach().double() - want).abs().max().item() <= 4 * R.ULP
    d_gn = torch.randn(K, P, generator=gen)
    gates.retain_grad()
    (y * torch.zeros(P, E).scatter_(1, idx.long().t(), d_gn.t())).sum().backward()
    ref = R.topk_norm_bwd_ref(gates.detach(), idx, d_gn)
    assert (gates.grad.double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
    assert (ref.scatter(1, idx.long().t(), 0.0) == 0).all()          # zero outside the token's K experts


def test_topk_normalisation_clamp_rows():
    """The hand-built rows: under the clamp the gradient is d_gn / eps (torch.clamp passes none to the sum), a sum of exactly eps is not
    clamped (gn = 1/2 each), K = 1 is the identity."""
    E, K = 8, 2
    rows = R.topk_special_rows(E)
    idx = torch.tensor([[0, 0, 0], [1, 1, 1]], dtype=torch.int32)
    d_gn = torch.tensor([[0.75, -1.25, 0.5], [2.0, 0.5, -3.0]])
    g = R.topk_norm_bwd_ref(rows, idx, d_gn)
    assert (rows[:, :2].sum(1) == torch.tensor([2 * np.float32(1e-9), R.EPS, R.EPS / 2])).all()
    for t in (0, 2):
        assert torch.equal(g[t, :2], d_gn[:, t].double() / R.EPS) and not g[t, 2:].any()
    assert torch.equal(R.topk_norm_fwd_ref(rows, idx)[:, 1], torch.tensor([0.5, 0.5], dtype=torch.float64))
    s = (d_gn[:, 1].double() * 0.5).sum()
    assert torch.allclose(g[1, :2], (d_gn[:, 1].double() - s) / R.EPS, rtol=1e-12, atol=0)
    one = R.topk_norm_bwd_ref(rows, idx[:1], d_gn[:1])
    assert torch.equal(one[:, 0], d_gn[0].double()) and not one[:, 1:].any()


def test_gate_bwd_dense_ref_terms():
    """gate_bwd_dense_ref without its dense operands is the construction of test_router_16bit_matrix_pipe_kernels_vs_fp64; the dense operands
    add linearly: d_logits_add alone gives dg = d_logits_add @ wg (no LayerNorm), and d_probs = onehot(idx) * d_gmax equals passing d_gmax."""
    gen = torch.Generator().manual_seed(9)
    P, G, E, seg = 2 * 37, 32, 4, 37
    g, wg = torch.randn(P, G, generator=gen), torch.randn(E, G, generator=gen) * 0.3
    lw, lb = 1 + 0.2 * torch.randn(G, generator=gen), 0.1 * torch.randn(G, generator=gen)
    idx = torch.randint(0, E, (P,), generator=gen)
    counts, coef = torch.randint(0, seg, (2, E), generator=gen), torch.rand(2, generator=gen)
    dgm, dla = torch.randn(P, generator=gen), torch.randn(P, E, generator=gen)
    zc = torch.zeros(2)
    a = R.gate_bwd_dense_ref(g, None, None, wg, idx, None, None, dla, counts, zc, seg)
    assert torch.allclose(a["dg"], dla.double() @ wg.double(), rtol=1e-12, atol=1e-14)
    assert torch.allclose(a["d_wg"], dla.double().t() @ g.double(), rtol=1e-12, atol=1e-13)
    b = R.gate_bwd_dense_ref(g, lw, lb, wg, idx, dgm, None, None, counts, coef, seg)
    c = R.gate_bwd_dense_ref(g, lw, lb, wg, idx, None, torch.nn.functional.one_hot(idx, E) * dgm[:, None], None, counts, coef, seg)
    for k in ("dg", "d_wg", "d_ln_w", "d_ln_b"):
        assert torch.allclose(b[k], c[k], rtol=1e-12, atol=1e-14)
    d = R.gate_bwd_dense_ref(g, lw, lb, wg, idx, dgm, None, dla, counts, coef, seg)
    e = R.gate_bwd_dense_ref(g, lw, lb, wg, idx, None, None, dla, counts, zc, seg)
    for k in ("dg", "d_wg", "d_ln_w", "d_ln_b"):
        assert torch.allclose(d[k], b[k] + e[k], rtol=1e-10, atol=1e-13)


def test_fp32_error_of_the_references():
    """The reference measured against itself: a plain fp32 torch evaluation against float64, per GPU case.  The GPU tolerances are 8 x these
    (at least 4 fp32 ulps of max|ref|), so the figures must be rounding noise: below 1e-5 of max|ref|, the agreement the oracle's own fp32
    evaluation shows on well-conditioned inputs.  Printed (pytest -s) for profiles/r11_topk_gate_kernel_parity.md."""
    lines = []
    for case in LI_CASES:
        _, r64, r32 = li(case)
        for k in ("l", "d_logits", "d_imp", "d_load"):
            tol, e32 = R.tolerance(r32[k], r64[k])
            m = r64[k].abs().max().item()
            lines.append(f"load_importance P={case[0]} E={case[1]} k={case[2]} sigma={case[3]}/E {k}: max|ref| {m:.3e} fp32 err {e32:.2e} tol {tol:.2e}")
            assert e32 <= 1e-5 * m, lines[-1]
    _, r64, r32 = li(R.SATURATED_CASE, shift=False)
    tol, e32 = R.tolerance(r32["d_logits"], r64["d_logits"])
    assert all(torch.isfinite(r32[k]).all() and torch.isfinite(r64[k]).all() for k in ("l", "d_logits", "d_imp", "d_load"))
    lines.append(f"load_importance saturated {R.SATURATED_CASE} d_logits: max|ref| {r64['d_logits'].abs().max().item():.3e} fp32 err {e32:.2e} tol {tol:.2e}")
    for case in R.GATE_LOGITS_CASES:
        g, wg, noise = R.gate_logits_inputs(case)
        r64 = R.gate_logits_ref(g, wg, noise, R.NOISE_SCALE)
        tol, e32 = R.tolerance(R.gate_logits_ref(g, wg, noise, R.NOISE_SCALE, torch.float32), r64)
        m = r64.abs().max().item()
        lines.append(f"gate_logits {case}: max|ref| {m:.3e} fp32 err {e32:.2e} tol {tol:.2e}")
        assert e32 <= 1e-5 * m, lines[-1]
    for E, K in R.TOPK_CASES:
        for P in R.TOPK_TOKENS:
            gates, d_gn = R.topk_inputs(E, K, P)
            idx = gates.topk(K, dim=1).indices.t().to(torch.int32)
            r64 = R.topk_norm_bwd_ref(gates, idx, d_gn)
            tol, e32 = R.tolerance(R.topk_norm_bwd_ref(gates, idx, d_gn, torch.float32), r64)
            m = r64.abs().max().item()
            lines.append(f"topk_gate_bwd E={E} K={K} P={P}: max|ref| {m:.3e} fp32 err {e32:.2e} tol {tol:.2e}")
            assert e32 <= 1e-5 * m, lines[-1]
    print("\n" + "\n".join(lines))
