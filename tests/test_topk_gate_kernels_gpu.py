"""Kernel-level parity of what a top-k gate and use_load_importance_loss add to the router, and of swn_gather_rows: every entry point called
directly (the layer goldens of test_moe_gpu.py reach them at 256 features x 8 experts only), bitwise where the operation is exact, against
the float64 references of tests/topk_gate_ref.py otherwise.  Tolerances that are not the project's own are 8 x the reference's own fp32
rounding error (topk_gate_ref.tolerance); measured figures: profiles/r11_topk_gate_kernel_parity.md."""
import pytest
import torch

import synth
import topk_gate_ref as R
from oracle import switchnerf_oracle as O
from tests.test_kernels_gpu import dev, ops, report

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def bits(t):
    return t.contiguous().view(torch.uint8)


# ---------------------------------------------------------------------------------------------------------------- gate_logits
@pytest.mark.parametrize("case", R.GATE_LOGITS_CASES, ids=lambda c: "-".join(map(str, c)))
def test_gate_logits(case):
    """swn_gate_logits = g @ wg.T + 0.125 * noise in float64 on the exact (16-bit) rows; gate_dim around the 64-lane feature loop, token
    counts past one grid stride (16384 waves), E of 1 ... 16.  Exactly P * E floats are written: a guard row behind them keeps its bits.
    Observed on the MI355X: kernel errors of 4.9e-09 ... 4.8e-06, at most 0.09 of their tolerances (1.0e-07 ... 1.3e-04); per case in
    profiles/r11_topk_gate_kernel_parity.md."""
    kind, E, G, P, with_noise = case
    o = ops()
    g, wg, noise = R.gate_logits_inputs(case)
    ref = R.gate_logits_ref(g, wg, noise, R.NOISE_SCALE)
    tol, e32 = R.tolerance(R.gate_logits_ref(g, wg, noise, R.NOISE_SCALE, torch.float32), ref)
    gd, wd, nd = g.to(dev()), wg.to(dev()), noise.to(dev()) if with_noise else None
    out = o.gate_logits(gd, wd, nd, R.NOISE_SCALE if with_noise else 0.0)
    assert out.shape == (P, E) and out.dtype == torch.float32
    report("gate_logits_" + "_".join(map(str, case)), out, ref.float())
    err = (out.double().cpu() - ref).abs().max().item()
    print(f"gate_logits {case}: max|ref| {ref.abs().max().item():.3e} fp32-ref err {e32:.2e} tol {tol:.2e} kernel err {err:.2e}")
    assert err <= tol
    # the same call into a buffer with a guard row behind the P * E floats
    buf = torch.full((P + 1, E), float("nan"), device=dev())
    guard = buf[P].clone()
    assert o.gate_logits(gd, wd, nd, R.NOISE_SCALE if with_noise else 0.0, out=buf[:P]).data_ptr() == buf.data_ptr()
    assert torch.equal(bits(buf[:P]), bits(out)) and torch.equal(bits(buf[P]), bits(guard))


# ---------------------------------------------------------------------------------------------------------------- load / importance
def _li_run(inp):
    o = ops()
    sc, lw, il = inp["scores"].to(dev()), inp["logits_w"].to(dev()), inp["idx_last"].to(dev())
    l, coef = o.load_importance_fwd(sc, lw, il, inp["sigma"])
    d_logits = o.load_importance_bwd(sc, lw, il, coef, torch.tensor([R.D_L], device=dev()), inp["sigma"])
    return l, coef, d_logits


@pytest.mark.parametrize("case", R.LOAD_IMPORTANCE_CASES, ids=lambda c: "-".join(map(str, c)))
def test_load_importance_fwd_bwd(case):
    """swn_load_importance_fwd / _bwd against the float64 reference on well-conditioned inputs (test_topk_gate_refs_cpu.py): the loss, the
    coefficients dl/dImp (coef[:E]) and dl/dLoad (coef[E:]) and d_logits = d_l * dl/dlogits with the device scalar d_l = -2.5; token counts
    around one block and past the 512-block grid stride, E of 2 ... 16, the threshold at the 1st / 2nd / E-th noisy logit.  Every tolerance is
    8 x the fp32 error of the reference itself.  Twice on the same inputs: the same bits (fixed summation order).
    Observed on the MI355X: at most 0.41 of the tolerance (l at P = 1: 9.1e-08 of 2.2e-07); at P = 131372, E = 8, k = 2 the loss is 2.1e-10 off
    (tolerance 1.7e-08) - 4.1e-08 before the block sums were kept in double.  Per case: profiles/r11_topk_gate_kernel_parity.md."""
    P, E, k, sE = case
    inp = R.load_importance_inputs(case)
    r64, r32 = R.load_importance_refs(inp)
    l, coef, d_logits = _li_run(inp)
    tag = f"P{P}_E{E}_k{k}_s{sE}"
    got = dict(l=l.reshape(()), d_imp=coef[:E], d_load=coef[E:], d_logits=d_logits)
    fails = []
    for key in ("l", "d_imp", "d_load", "d_logits"):
        tol, e32 = R.tolerance(r32[key], r64[key])
        report(f"load_importance_{key}_{tag}", got[key], r64[key].float())
        err = (got[key].double().cpu() - r64[key]).abs().max().item()
        print(f"load_importance {tag} {key}: max|ref| {r64[key].abs().max().item():.3e} fp32-ref err {e32:.2e} tol {tol:.2e} kernel err {err:.2e}")
        if not err <= tol:
            fails.append((key, err, tol))
    assert not fails, fails          # (observed: every err <= 0.41 tol)
    l2, coef2, d2 = _li_run(inp)
    assert torch.equal(bits(l), bits(l2)) and torch.equal(bits(coef), bits(coef2)) and torch.equal(bits(d_logits), bits(d2))


def test_load_importance_saturated():
    """sigma = 0.05 / E and no threshold shift: the cdf is 0 or 1 almost everywhere and the loss is ill-conditioned (no relative claim on it):
    everything finite, d_logits to 8 x the reference's own fp32 error, an absolute tolerance of 3e-6 of max|ref|.
    Observed on the MI355X: 6.7e-09 against a tolerance of 9.9e-08 (max|ref| 3.0e-02)."""
    inp = R.load_importance_inputs(R.SATURATED_CASE, shift=False)
    r64, r32 = R.load_importance_refs(inp)
    l, coef, d_logits = _li_run(inp)
    assert torch.isfinite(l).all() and torch.isfinite(coef).all() and torch.isfinite(d_logits).all()
    tol, e32 = R.tolerance(r32["d_logits"], r64["d_logits"])
    err = (d_logits.double().cpu() - r64["d_logits"]).abs().max().item()
    report("load_importance_d_logits_saturated", d_logits, r64["d_logits"].float())
    print(f"load_importance saturated d_logits: max|ref| {r64['d_logits'].abs().max().item():.3e} fp32-ref err {e32:.2e} tol {tol:.2e} kernel err {err:.2e}")
    assert err <= tol


# ---------------------------------------------------------------------------------------------------------------- top-k normalisation
@pytest.mark.parametrize("E,K", R.TOPK_CASES)
def test_topk_gate_bwd(E, K):
    """swn_topk_gate_bwd against autograd in float64 through g_j / clamp(sum_j g_j, eps), gathered with the kernel's own indices
    (swn_topk_select; its tie order is tested in test_kernels_gpu.py): softmax rows and rows with exact ties at 1 / 257 / 1000 tokens, and the
    hand-built rows - selected gates summing below eps (the gradient is d_gn / eps, exact: eps is a power of two), to exactly eps (not
    clamped).  K = 1 is the identity.  Outside a token's K experts the gradient is exactly 0.
    Observed on the MI355X: 0 at K = 1, otherwise 4.5e-08 ... 1.2e-05, at most 0.42 of the tolerance (8 x the reference's fp32 error); per
    case in profiles/r11_topk_gate_kernel_parity.md."""
    o = ops()
    for P in R.TOPK_TOKENS:
        gates, d_gn = R.topk_inputs(E, K, P)
        gd = gates.to(dev())
        idx = o.topk_select(gd, K)[0]
        assert torch.equal(gates.gather(1, idx.cpu().long().t()), gates.topk(K, dim=1).values)      # (ties: the kernel's own order)
        got = o.topk_gate_bwd(gd, idx, d_gn.to(dev()))
        ref = R.topk_norm_bwd_ref(gates, idx.cpu(), d_gn)
        tol, e32 = R.tolerance(R.topk_norm_bwd_ref(gates, idx.cpu(), d_gn, torch.float32), ref)
        report(f"topk_gate_bwd_E{E}_K{K}_P{P}", got, ref.float())
        err = (got.double().cpu() - ref).abs().max().item()
        print(f"topk_gate_bwd E={E} K={K} P={P}: max|ref| {ref.abs().max().item():.3e} fp32-ref err {e32:.2e} tol {tol:.2e} kernel err {err:.2e}")
        assert err <= tol          # (observed: err <= 0.42 tol)
        assert (got.cpu().scatter(1, idx.cpu().long().t(), 0.0) == 0).all() and (got.cpu() != 0).sum(1).max().item() <= K
        if K == 1:
            assert torch.equal(got.cpu().gather(1, idx.cpu().long().t())[:, 0], d_gn[0])
    if E < 2:
        return
    rows = R.topk_special_rows(E)
    d_gn = torch.randn(K, 3, generator=torch.Generator().manual_seed(E + K))
    idx = o.topk_select(rows.to(dev()), K)[0]
    got = o.topk_gate_bwd(rows.to(dev()), idx, d_gn.to(dev())).cpu()
    ref = R.topk_norm_bwd_ref(rows, idx.cpu(), d_gn)
    sel = got.gather(1, idx.cpu().long().t())                                       # [3, K]
    assert (got.scatter(1, idx.cpu().long().t(), 0.0) == 0).all()
    if K == 1:
        assert torch.equal(sel, d_gn.t())
        return
    for t in (0, 2):             # under the clamp: d_gn / eps, bit for bit
        assert torch.equal(sel[t], d_gn[:, t] * 2.0 ** 23) and torch.equal(sel[t].double(), ref.gather(1, idx.cpu().long().t())[t])
    # a sum of exactly eps is not clamped: (d_gn_j - sum_m d_gn_m gn_m) / eps
    assert (got[1].double() - ref[1]).abs().max().item() <= 4 * R.ULP * ref[1].abs().max().item()
    assert (ref[1].gather(0, idx.cpu().long()[:, 1]) - d_gn[:, 1].double() / R.EPS).abs().max().item() > 1e3      # (the clamped form differs)


# ---------------------------------------------------------------------------------------------------------------- gate backward, dense operands
GATE_PAIRS = [(128, 4), (128, 8), (256, 4), (256, 8), (256, 16), (512, 8), (512, 16)]
_OPERANDS = ("d_probs", "d_logits_add", "all")


def _gate_bwd_cases():
    for Gd, E in GATE_PAIRS:
        for kind in ("f32", "bf16"):
            if (Gd, E) in ((256, 8), (512, 16)):
                for ln in (True, False):
                    for operands in _OPERANDS:
                        yield Gd, E, kind, ln, operands
            else:
                yield Gd, E, kind, True, "all"


@pytest.mark.parametrize("Gd,E,kind,ln,operands", list(_gate_bwd_cases()))
def test_gate_bwd_dense(Gd, E, kind, ln, operands):
    """swn_gate_bwd_dense against autograd in float64 (LayerNorm, softmax, sum(pr * (coef counts + onehot(idx) d_gmax + d_probs)) +
    sum(logits * d_logits_add)) at all seven (gate_dim, experts) pairs of the dispatch macros, fp32 and 16-bit rows, two ragged segments of
    1031 tokens with their own counts and coefficient; the parameter gradients accumulate into a non-zero prefill.  Tolerances: the
    project's own for this kernel (dg 1e-5 of max in fp32, 6e-3 in 16-bit: the output rows; parameter gradients 2e-4 of max)."""
    o = ops()
    gen = torch.Generator().manual_seed(100 * Gd + E)
    seg, n_seg = 1031, 2
    P = seg * n_seg
    g = (torch.randn(P, Gd, generator=gen) * 1.3 + 0.4).to(DT[kind]).to(dev())
    ln_w = (1.0 + 0.2 * torch.randn(Gd, generator=gen)).to(dev()) if ln else None
    ln_b = (0.1 * torch.randn(Gd, generator=gen)).to(dev()) if ln else None
    wg = (torch.randn(E, Gd, generator=gen) / 16).to(dev())
    counts = torch.randint(0, seg, (n_seg, E), generator=gen, dtype=torch.int32).to(dev())
    coef = (torch.rand(n_seg, generator=gen) * 1e-3).to(dev())
    d_gmax = torch.randn(P, generator=gen).to(dev()) if operands == "all" else None
    d_probs = torch.randn(P, E, generator=gen).to(dev()) if operands != "d_logits_add" else None
    d_la = (0.5 * torch.randn(P, E, generator=gen)).to(dev()) if operands != "d_probs" else None
    gates, idx, gmax, stats = o.gate_fwd(g, ln_w, ln_b, wg)
    fill = 0.375
    d_wg, d_lw, d_lb = (torch.full(s, fill, device=dev()) for s in ((E, Gd), (Gd,), (Gd,)))
    dg = o.gate_bwd_dense(g, ln_w, ln_b, wg, gates, idx, d_gmax, d_probs, stats, counts, coef, seg, d_wg, d_lw if ln else None,
                          d_lb if ln else None, d_logits_add=d_la)
    r = R.gate_bwd_dense_ref(*(None if t is None else t.cpu() for t in (g, ln_w, ln_b, wg, idx, d_gmax, d_probs, d_la, counts, coef)), seg)
    assert (gates.double().cpu() - r["pr"]).abs().max().item() <= 1e-5
    rel = lambda a, b: ((a.double().cpu() - b).abs().max() / b.abs().max()).item()
    tag = f"{Gd}x{E}_{kind}_ln{int(ln)}_{operands}"
    report("gate_bwd_dense_dg_" + tag, dg, r["dg"].float())
    report("gate_bwd_dense_dwg_" + tag, d_wg - fill, r["d_wg"].float())
    assert dg.dtype == g.dtype and rel(dg, r["dg"]) <= (1e-5 if kind == "f32" else 6e-3)
    assert rel(d_wg - fill, r["d_wg"]) <= 2e-4
    if ln:
        assert rel(d_lw - fill, r["d_ln_w"]) <= 2e-4 and rel(d_lb - fill, r["d_ln_b"]) <= 2e-4
    else:
        assert torch.equal(d_lw, torch.full_like(d_lw, fill)) and torch.equal(d_lb, torch.full_like(d_lb, fill))


@pytest.mark.parametrize("Gd,E", GATE_PAIRS)
@pytest.mark.parametrize("ln", [True, False])
def test_gate_bwd_dense_with_zero_operands_is_gate_bwd(Gd, E, ln):
    """In fp32 swn_gate_bwd_dense with all-zero d_probs (and with all-zero d_logits_add) equals swn_gate_bwd bit for bit: the same VALU
    kernel, and x + 0.f is exact."""
    o = ops()
    gen = torch.Generator().manual_seed(7 * Gd + E)
    seg, n_seg = 1031, 2
    P = seg * n_seg
    g = (torch.randn(P, Gd, generator=gen) * 1.3 + 0.4).to(dev())
    ln_w = (1.0 + 0.2 * torch.randn(Gd, generator=gen)).to(dev()) if ln else None
    ln_b = (0.1 * torch.randn(Gd, generator=gen)).to(dev()) if ln else None
    wg = (torch.randn(E, Gd, generator=gen) / 16).to(dev())
    counts = torch.randint(0, seg, (n_seg, E), generator=gen, dtype=torch.int32).to(dev())
    coef = (torch.rand(n_seg, generator=gen) * 1e-3).to(dev())
    d_gmax = torch.randn(P, generator=gen).to(dev())
    gates, idx, gmax, stats = o.gate_fwd(g, ln_w, ln_b, wg)
    zeros = torch.zeros(P, E, device=dev())
    outs = []
    for dp, dla in ((None, None), (zeros, None), (None, zeros), (zeros, zeros)):
        d_wg, d_lw, d_lb = (torch.full(s, 0.375, device=dev()) for s in ((E, Gd), (Gd,), (Gd,)))
        a = (g, ln_w, ln_b, wg, gates, idx, d_gmax)
        b = (stats, counts, coef, seg, d_wg, d_lw if ln else None, d_lb if ln else None)
        dg = o.gate_bwd(*a, *b) if dp is None and dla is None else o.gate_bwd_dense(*a, dp, *b, d_logits_add=dla)
        outs.append((dg, d_wg, d_lw, d_lb))
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            assert torch.equal(bits(x), bits(y))


# ---------------------------------------------------------------------------------------------------------------- dispatch, further choices
@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("cf", [0.25, 4.0])
@pytest.mark.parametrize("K,P,E,H", [(K, P, E, H) for K in (2, 3) for P, E, H in ((1, 2, 8), (65, 8, 72), (1000, 8, 256), (300, 64, 64)) if K <= E])
def test_dispatch_more(K, P, E, H, cf, kind):
    """swn_dispatch_fwd_more / swn_dispatch_bwd_data_more (the later iterations of tutel_fast_dispatch.py:26-27 and :34-37) on
    oracle.route_topk's routing, most pairs dropped (capacity factor 0.25) or none (4.0).
    Forward: after swn_dispatch_fwd for choice 0 and _more for the rest every owned row is the single correctly rounded product g * x
    (x itself without gates), every other row exactly zero - bitwise.  Backward data: out += g * D[row] against the float64 sum over the
    choices (1e-6 relative in fp32, 2e-2 in 16-bit: test_tutel_sparse_abi's); a token whose choice j was dropped keeps its row's bits."""
    o = ops()
    dt = DT[kind]
    r = O.route_topk(synth.make_gates(500 + P + K, P, E, 2.0), K, cf, True)
    cap = int(r["capacity"])
    gen = torch.Generator().manual_seed(P + 13 * K)
    x = torch.randn(P, H, generator=gen).to(dt)
    gate = torch.rand(K, P, generator=gen) + 0.05
    idx, loc = torch.from_numpy(r["idx"]), torch.from_numpy(r["loc"])
    xd, gd, id_, ld = x.to(dev()), gate.to(dev()), idx.to(dev()), loc.to(dev())
    if cap < 1:          # int(0.25 * ceil(1 / 2)) = 0 rows per expert: there is no buffer to dispatch into - the entry points refuse
        with pytest.raises(RuntimeError):
            o.dispatch_fwd_more(gd[1], id_[1], ld[1], xd, torch.empty(0, H, dtype=dt, device=dev()), E, cap)
        with pytest.raises(RuntimeError):
            o.dispatch_bwd_data_more(gd[1], id_[1], ld[1], torch.zeros(P, H, dtype=dt, device=dev()), torch.empty(0, H, dtype=dt, device=dev()), cap)
        return
    keep = loc < cap
    rows = idx.long() * cap + loc.long()
    assert cf < 1 or keep.all()
    for with_gates in (True, False):
        want = torch.zeros(E * cap, H, dtype=dt)
        for j in range(K):
            want[rows[j][keep[j]]] = ((gate[j][:, None] * x.float()).to(dt) if with_gates else x)[keep[j]]
        d = o.dispatch_fwd(gd[0] if with_gates else None, id_[0], ld[0], xd, E, cap)
        for j in range(1, K):
            assert o.dispatch_fwd_more(gd[j] if with_gates else None, id_[j], ld[j], xd, d, E, cap) is d
        assert torch.equal(bits(d.cpu()), bits(want)), f"dispatched rows, gates={with_gates}"
    # backward data
    D = torch.randn(E * cap, H, generator=gen).to(dt)
    Dd = D.to(dev())
    ref = torch.zeros(P, H, dtype=torch.float64)
    for j in range(K):
        ref += torch.where(keep[j][:, None], gate[j].double()[:, None] * D.double()[rows[j].clamp(max=E * cap - 1)], torch.zeros((), dtype=torch.float64))
    out = o.dispatch_bwd_data(gd[0], id_[0], ld[0], Dd, cap)
    for j in range(1, K):
        assert o.dispatch_bwd_data_more(gd[j], id_[j], ld[j], out, Dd, cap) is out
    report(f"dispatch_bwd_data_more_K{K}_P{P}_E{E}_H{H}_cf{cf}_{kind}", out, ref.float())
    assert (out.double().cpu() - ref).abs().max().item() <= (1e-6 if kind == "f32" else 2e-2) * ref.abs().max().item()
    # `+=` of one choice alone onto a filled buffer: dropped tokens keep their bits, kept tokens gain g * D[row]
    for j in range(1, K):
        prev = torch.randn(P, H, generator=gen).to(dt)
        out = o.dispatch_bwd_data_more(gd[j], id_[j], ld[j], prev.to(dev()), Dd, cap).cpu()
        assert torch.equal(bits(out[~keep[j]]), bits(prev[~keep[j]]))
        want = prev.double()[keep[j]] + gate[j].double()[keep[j]][:, None] * D.double()[rows[j][keep[j]]]
        if keep[j].any():
            assert (out.double()[keep[j]] - want).abs().max().item() <= (1e-6 if kind == "f32" else 2e-2) * want.abs().max().item()


# ---------------------------------------------------------------------------------------------------------------- the chain of a top-k gate
def test_topk_gate_chain_bf16_512x16():
    """swn_gate_fwd -> swn_topk_select -> swn_topk_gate_bwd -> swn_gate_bwd_dense at bf16, 512 features, 16 experts, k = 2, 2050 tokens
    against autograd in float64 of sum(d_gn * gnorm) + coef * sum(counts * pr), gnorm gathered with the kernel's own indices.  Tolerances
    as for swn_gate_bwd_dense: dg 6e-3 of max (16-bit rows), d_wg 2e-4 of max."""
    o = ops()
    gen = torch.Generator().manual_seed(77)
    P, Gd, E, K = 2050, 512, 16, 2
    g = (torch.randn(P, Gd, generator=gen) * 1.3 + 0.4).to(torch.bfloat16).to(dev())
    wg = (torch.randn(E, Gd, generator=gen) * 0.05).to(dev())
    d_gn = torch.randn(K, P, generator=gen).to(dev())
    counts = torch.randint(0, P, (1, E), generator=gen, dtype=torch.int32).to(dev())
    coef = torch.tensor([3e-4], device=dev())
    gates, idx0, gmax, stats = o.gate_fwd(g, None, None, wg)
    idx, gsel, gn = o.topk_select(gates, K)
    assert torch.equal(idx[0], idx0)
    d_probs = o.topk_gate_bwd(gates, idx, d_gn)
    d_wg = torch.full((E, Gd), 0.375, device=dev())
    dg = o.gate_bwd_dense(g, None, None, wg, gates, idx0, None, d_probs, stats, counts, coef, P, d_wg, None, None)
    x = g.double().cpu().requires_grad_(True)
    W = wg.double().cpu().requires_grad_(True)
    pr = torch.softmax(x @ W.t(), 1)
    gnorm = R.topk_norm_fwd_ref(pr, idx.cpu())
    assert (gn.double().cpu() - gnorm.detach()).abs().max().item() <= 1e-5
    ((d_gn.double().cpu() * gnorm).sum() + coef.double().cpu()[0] * (counts.double().cpu() * pr).sum()).backward()
    rel = lambda a, b: ((a.double().cpu() - b).abs().max() / b.abs().max()).item()
    report("topk_chain_dg", dg, x.grad.float())
    report("topk_chain_dwg", d_wg - 0.375, W.grad.float())
    assert rel(dg, x.grad) <= 6e-3
    assert rel(d_wg - 0.375, W.grad) <= 2e-4


# ---------------------------------------------------------------------------------------------------------------- gather_rows
@pytest.mark.parametrize("R_", [1, 3001])
def test_gather_rows(R_):
    """swn_gather_rows (every expert-parallel send buffer) byte for byte: out[r] = src[index[r]], zero rows for index -1, repeated indices,
    rows of 4, 16 and 512 bytes (the widths of the swn_scatter_rows test), the `out=` form and the allocating form; gather_rows after
    scatter_rows through a permutation gives the source back."""
    o = ops()
    gen = torch.Generator().manual_seed(11 + R_)
    S = 5000
    index = torch.randint(0, S, (R_,), generator=gen).to(torch.int32)
    if R_ > 1:
        index[1::7] = index[0]                   # repeats
        index[::9] = -1
    for neg_only in ((False, True) if R_ == 1 else (False,)):
        if neg_only:
            index = torch.tensor([-1], dtype=torch.int32)
        for cols, dtype in ((1, torch.float32), (4, torch.float32), (256, torch.bfloat16), (4, torch.int32)):
            src = torch.randn(S, cols, generator=gen).to(dtype) if dtype != torch.int32 else torch.randint(-2**31, 2**31 - 1, (S, cols), generator=gen, dtype=torch.int32)
            want = torch.where((index >= 0)[:, None], src[index.long().clamp(min=0)], torch.zeros((), dtype=dtype))
            got = o.gather_rows(src.to(dev()), index.to(dev()))
            assert got.shape == (R_, cols) and got.dtype == dtype and torch.equal(bits(got.cpu()), bits(want))
            buf = torch.full((R_ + 1, cols), 7, dtype=dtype).to(dev())                  # (a guard row behind the R rows)
            assert o.gather_rows(src.to(dev()), index.to(dev()), out=buf[:R_]).data_ptr() == buf.data_ptr()
            assert torch.equal(bits(buf[:R_].cpu()), bits(want)) and (buf[R_] == 7).all()
            if cols * src.element_size() % 16 == 0:
                # 16-byte rows in buffers that start 4 bytes off a 16-byte boundary: the 4-byte pieces, the same bytes
                w = cols * src.element_size() // 4
                s_off = torch.zeros(S * w + 1, dtype=torch.int32, device=dev())
                s_off[1:] = src.contiguous().view(torch.int32).reshape(-1).to(dev())
                d_off = torch.full((R_ * w + 2,), 7, dtype=torch.int32, device=dev())
                assert s_off[1:].data_ptr() % 16 == 4 and d_off[1:].data_ptr() % 16 == 4
                o.gather_rows(s_off[1:].view(S, w), index.to(dev()), out=d_off[1:1 + R_ * w].view(R_, w))
                assert torch.equal(bits(d_off[1:1 + R_ * w].cpu()), bits(want).reshape(-1)) and d_off[0] == 7 and d_off[-1] == 7
            if R_ > 1:
                perm = torch.randperm(S, generator=gen)[:R_].to(torch.int32).to(dev())
                rows = src[:R_].to(dev())
                scattered = o.scatter_rows(rows, perm, torch.zeros(S, cols, dtype=dtype, device=dev()))
                assert torch.equal(bits(o.gather_rows(scattered, perm)), bits(rows))
