"""The residual MoE branch of the layer mirror (moe_layer(use_residual=True); tutel_moe_layer_nobatch.py:504-505, 666-671, 777-788):
against the reference layer's own run (scripts/gen_golden_residual.py), the bf16 layer and the mix kernels (swn_residual_mix_fwd /
_bwd) against fp64 restatements of their stated arithmetic, moe_no_batch / eval, and run-to-run bit equality."""
import os

import numpy as np
import pytest
import torch

import residual_weights
import synth

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


def _layer(cfg, k=1, cf=1.0, dtype=torch.float32, **kw):
    from switch_nerf_amd.moe import moe_layer
    return moe_layer(gate_type=dict(type="top", k=k, fp32_gate=True, capacity_factor=cf, batch_prioritized_routing=True, gate_noise=-1.0,
                                    compute_balance_loss=False, dispatcher_no_score=False, is_postscore=True, gate_dim=cfg["gate_hidden"]),
                     model_dim=cfg["model_dim"],
                     experts=dict(type="expertmlp", count_per_node=cfg["num_experts"], hidden_size_per_expert=cfg["model_dim"],
                                  layer_num=cfg["expert_layers"], skips=list(cfg["skips"])),
                     seeds=(1, 1, 1), return_gates=True, dtype=dtype, **kw).cuda()


def _load(moe, seed, cfg):
    sd = residual_weights.layer_state_dict(seed, cfg)
    if not moe.use_residual:
        sd = {k: v for k, v in sd.items() if not k.startswith(("coefficient.", "residual_expert."))}
    moe.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)


def _chain64(x, moe):
    """The residual expert in fp64 (ExpertMLP.forward, tutel_moe_layer_nobatch.py:901-924) with the layer's weights in its dtype."""
    rex, dt = moe.residual_expert, moe.dtype
    h = x0 = x.double()
    L = moe.layer_num
    for l in range(L):
        h = h @ rex.weights[l].detach()[0].to(dt).double() + rex.bias[l].detach()[0, 0].double()
        if l in moe.skips:
            h = h + x0
            if l < L - 1:
                h = torch.relu(h)
            x0 = h
        elif l < L - 1:
            h = torch.relu(h)
    return h


def _coef64(x, moe):
    return torch.softmax(x.double() @ moe.coefficient.weight.detach().double().t() + moe.coefficient.bias.detach().double(), dim=-1)


@pytest.mark.parametrize("tag", ["top1_cf100", "top1_cf000", "top2_cf100", "m64e4_p1000"])
def test_residual_layer_vs_reference_golden_fp32(tag):
    """Output, l_aux, the indices (bit-exact), the mixing weights, dx, dgate_input and every parameter gradient (coefficient and
    residual expert included) against the reference layer's run; the tolerances of test_dyncap_gpu's moe-layer fixtures."""
    g = np.load(os.path.join(G, f"moe_layer_residual_{tag}.npz"))
    seed, P, k, cf, M = int(g["seed"]), int(g["P"]), int(g["k"]), float(g["cf"]), int(g["model_dim"])
    cfg = synth.BUILDING if M == 256 else dict(synth.small_cfg(M, int(g["n_experts"])), gate_hidden=int(g["gate_dim"]))
    moe = _layer(cfg, k, cf, use_residual=True)
    _load(moe, seed, cfg)
    rng = np.random.default_rng(seed + 1000)
    x = rng.standard_normal((P, M)).astype(np.float32)
    gi = rng.standard_normal((P, cfg["gate_hidden"])).astype(np.float32)
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    gt = torch.from_numpy(gi).cuda().requires_grad_(True)
    y = moe(xt, gate_input=gt)
    np.testing.assert_array_equal(y.gate_extras["gates"].cpu().numpy().reshape(-1), g["topk"].reshape(-1))
    np.testing.assert_allclose(y.l_aux.item(), float(g["l_aux"]), rtol=1e-5)
    np.testing.assert_allclose(moe.residual_coef.cpu().numpy(), g["coef"], rtol=0, atol=1e-5)
    dy = rng.standard_normal(tuple(y.shape)).astype(np.float32)
    ((y * torch.from_numpy(dy).cuda()).sum() + y.l_aux).backward()
    for n, t, rtol in (("y", y.detach(), 1e-4), ("dx", xt.grad, 1e-3), ("dgate_input", gt.grad, 1e-3)):
        got = t.cpu().numpy()
        ref, ref_sum = g["slice__" + n], g["sum__" + n]
        atol = 5e-5 if n == "y" else 2e-4 * np.abs(ref).max()
        np.testing.assert_allclose(got.reshape(-1)[:: max(1, got.size // 2048)][:2048], ref, rtol=rtol, atol=atol, err_msg=n)
        np.testing.assert_allclose(synth.checksum(got)[1:], ref_sum[1:], rtol=1e-3, err_msg=n)
        assert abs(synth.checksum(got)[0] - ref_sum[0]) <= 1e-3 * ref_sum[1], n
    names = {str(n) for n in g["names"]}
    assert {n for n, _ in moe.named_parameters()} == names
    for n, p in moe.named_parameters():
        got = p.grad.cpu().numpy()
        ref_sum = g["gsum__" + n]
        scale = max(1e-12, float(ref_sum[1]))
        assert abs(synth.checksum(got)[0] - ref_sum[0]) <= 1e-3 * scale + 1e-9, n
        sl = got.reshape(-1)[:: max(1, got.size // 997)][:997]
        ref = g["gslice__" + n]
        np.testing.assert_allclose(sl, ref, rtol=2e-3, atol=1e-7 + 5e-4 * np.abs(ref).max(), err_msg=n)


def _mix_operands(P, M, dtype, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x, ym, yr, dy = (torch.randn(P, M, device="cuda", generator=gen).to(dtype) for _ in range(4))
    wc = (torch.rand(2, M, device="cuda", generator=gen) * 2 - 1) * (2.0 / M ** 0.5)
    bc = (torch.rand(2, device="cuda", generator=gen) * 2 - 1) * 0.1
    return x, ym, yr, dy, wc.contiguous(), bc.contiguous()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M", [64, 256, 512])
@pytest.mark.parametrize("P", [1, 63, 1000, 65536 + 17])
def test_mix_kernels_vs_fp64(P, M, dtype):
    """swn_residual_mix_fwd / _bwd against fp64 from the stored operands.  Tolerances: coef within 1e-5 (fp32 logits and softmax); each
    dtype output within one rounding (2^-8 relative for bf16, 1e-5 for fp32) of the fp64 value plus the fp32 error of the per-token dot
    products (1e-5 of their absolute sums, times what multiplies them); dWc / dbc within 2e-5 of the absolute sums of their terms plus the
    same per-token error.  dWc / dbc bit-identical across two launches."""
    from switch_nerf_amd import ops
    x, ym, yr, dy, wc, bc = _mix_operands(P, M, dtype, 1000 * M + P)
    y, coef = ops.residual_mix_fwd(x, ym, yr, wc, bc)
    d_moe, d_res, dx, d_wc, d_bc = ops.residual_mix_bwd(dy, x, ym, yr, coef, wc)
    d_moe2, d_res2, dx2, d_wc2, d_bc2 = ops.residual_mix_bwd(dy, x, ym, yr, coef, wc)
    torch.cuda.synchronize()
    assert torch.equal(d_wc, d_wc2) and torch.equal(d_bc, d_bc2)
    assert torch.equal(dx, dx2) and torch.equal(d_moe, d_moe2) and torch.equal(d_res, d_res2)
    X, YM, YR, DY, W = x.double(), ym.double(), yr.double(), dy.double(), wc.double()
    c = torch.softmax(X @ W.t() + bc.double(), dim=-1)
    assert (coef.double() - c).abs().max().item() <= 1e-5
    rel = 2.0 ** -8 if dtype == torch.bfloat16 else 1e-5
    y_ref = YM * c[:, :1] + YR * c[:, 1:]
    tol = rel * y_ref.abs() + 1e-5 * (YM.abs() + YR.abs())
    assert bool(((y.double() - y_ref).abs() <= tol).all())
    # backward
    g0, g1 = (DY * YM).sum(1), (DY * YR).sum(1)
    e_g = 1e-5 * ((DY * YM).abs().sum(1) + (DY * YR).abs().sum(1))          # fp32 error of the token's dot products
    sg = c[:, 0] * g0 + c[:, 1] * g1
    dl = torch.stack([c[:, 0] * (g0 - sg), c[:, 1] * (g1 - sg)], 1)
    for got, ref in ((d_moe, c[:, :1] * DY), (d_res, c[:, 1:] * DY)):
        assert bool(((got.double() - ref).abs() <= rel * ref.abs() + 1e-5 * DY.abs()).all())
    dx_ref = dl @ W
    tol = rel * dx_ref.abs() + (rel * dl.abs() + e_g[:, None]) @ W.abs() + 1e-7
    assert bool(((dx.double() - dx_ref).abs() <= tol).all())
    dw_ref, db_ref = dl.t() @ X, dl.sum(0)
    assert bool(((d_wc.double() - dw_ref).abs() <= 2e-5 * (dl.abs().t() @ X.abs()) + e_g[None, :] @ X.abs() + 1e-6).all())
    assert bool(((d_bc.double() - db_ref).abs() <= 2e-5 * dl.abs().sum(0) + e_g.sum() + 1e-6).all())


def test_mix_refuses_unsupported_width():
    from switch_nerf_amd import ops
    x = torch.zeros(8, 96, device="cuda")
    with pytest.raises(RuntimeError, match="model_dim 96"):
        ops.residual_mix_fwd(x, x, x, torch.zeros(2, 96, device="cuda"), torch.zeros(2, device="cuda"))


def test_residual_layer_bf16_vs_fp64_restatement():
    """The bf16 layer (persistent 256-row chain for the residual expert at P = 4096) with the reference fixture's weights: the residual
    expert within bf16 intermediate rounding (2e-2 of its largest value) of the fp64 chain on the bf16 weights; the mixing weights within
    1e-5 of fp64 softmax on the bf16 input; the output within one bf16 rounding of y_moe c0 + y_res c1 in fp64 on the stored operands
    (y_moe: the same layer without the branch, y_res: the residual expert's launch); coefficient gradients within 1e-3 of their largest
    value of fp64 on the bf16 operands; the residual expert's gradients point where the fp32 layer's do (cosine > 0.99)."""
    from switch_nerf_amd.moe import _ResidualExpertFunction
    cfg, seed, P = synth.BUILDING, 51, 4096
    m16 = _layer(cfg, dtype=torch.bfloat16, use_residual=True)
    _load(m16, seed, cfg)
    plain = _layer(cfg, dtype=torch.bfloat16)
    _load(plain, seed, cfg)
    m32 = _layer(cfg, use_residual=True)
    _load(m32, seed, cfg)
    gen = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(P, 256, device="cuda", generator=gen).requires_grad_(True)
    gi = torch.randn(P, 256, device="cuda", generator=gen)
    y = m16(x, gate_input=gi)
    assert y.dtype == torch.float32 and y.shape == (P, 256)
    coef = m16.residual_coef.double()
    with torch.no_grad():
        ym = plain(x, gate_input=gi).double()
        xs = x.detach().to(torch.bfloat16)
        rex = m16.residual_expert
        yr = _ResidualExpertFunction.apply(m16, xs, *rex.weights, *rex.bias).double()
    assert torch.equal(plain(x, gate_input=gi).l_aux, y.l_aux)
    yr64 = _chain64(xs, m16)
    assert (yr - yr64).abs().max().item() <= 2e-2 * yr64.abs().max().item()
    c = _coef64(xs, m16)
    assert (coef - c).abs().max().item() <= 1e-5
    y_ref = ym * c[:, :1] + yr * c[:, 1:]
    assert bool(((y.detach().double() - y_ref).abs() <= 2.0 ** -8 * y_ref.abs() + 1e-5 * (ym.abs() + yr.abs())).all())
    dy = torch.randn(P, 256, device="cuda", generator=gen)
    (y * dy).sum().backward()
    DY = dy.to(torch.bfloat16).double()
    g0, g1 = (DY * ym).sum(1), (DY * yr).sum(1)
    sg = coef[:, 0] * g0 + coef[:, 1] * g1
    dl = torch.stack([coef[:, 0] * (g0 - sg), coef[:, 1] * (g1 - sg)], 1)
    dw_ref, db_ref = dl.t() @ xs.double(), dl.sum(0)
    assert (m16.coefficient.weight.grad.double() - dw_ref).abs().max().item() <= 1e-3 * dw_ref.abs().max().item()
    assert (m16.coefficient.bias.grad.double() - db_ref).abs().max().item() <= 1e-3 * db_ref.abs().max().item() + 1e-3
    assert torch.isfinite(x.grad).all() and x.grad.abs().max().item() > 0
    y32 = m32(x.detach(), gate_input=gi)
    (y32 * dy).sum().backward()
    for (n, p16), p32 in zip(m16.named_parameters(), m32.parameters()):
        if n.startswith("residual_expert."):
            cos = torch.nn.functional.cosine_similarity(p16.grad.flatten(), p32.grad.flatten(), dim=0).item()
            assert cos > 0.99, (n, cos)


@pytest.mark.parametrize("M,E,k,P", [(256, 8, 1, 2048), (64, 4, 2, 1000)])
def test_residual_no_batch_and_eval_vs_fp64(M, E, k, P):
    """moe_no_batch (capacity = P, nothing dropped) in eval under no_grad: the output against fp64 of y_moe c0 + chain(x) c1 with y_moe the
    no-batch layer without the branch (the reference's no-batch branch asserts on the test stubs, so there is no reference fixture);
    l_aux and the indices are those of the layer without the branch."""
    cfg = synth.BUILDING if M == 256 else dict(synth.small_cfg(M, E), gate_hidden=128)      # (the router takes 128, 256 or 512 features)
    nb = _layer(cfg, k, use_residual=True, moe_no_batch=True)
    _load(nb, 54, cfg)
    plain = _layer(cfg, k, moe_no_batch=True)
    _load(plain, 54, cfg)
    nb.eval(), plain.eval()
    gen = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(P, M, device="cuda", generator=gen)
    gi = torch.randn(P, cfg["gate_hidden"], device="cuda", generator=gen)
    with torch.no_grad():
        y, ym = nb(x, gate_input=gi), plain(x, gate_input=gi)
    assert torch.equal(y.l_aux, ym.l_aux) and torch.equal(y.gate_extras["gates"], ym.gate_extras["gates"])
    assert bool((ym.abs().sum(-1) > 0).all())
    c = _coef64(x, nb)
    y_ref = ym.double() * c[:, :1] + _chain64(x, nb) * c[:, 1:]
    assert (y.double() - y_ref).abs().max().item() <= 1e-4 * y_ref.abs().max().item()


@pytest.mark.parametrize("k,cf", [(1, 0.0), (2, 1.0)])
def test_residual_layer_is_bit_reproducible(k, cf):
    """bf16, ragged P = 1000 (persistent chain geometry, a partial last tile): two forward / backward runs give the same output, input
    gradients and parameter gradients bit for bit (the mixing weights' gradients are ordered block sums, no atomics)."""
    cfg = synth.BUILDING
    moe = _layer(cfg, k, cf, dtype=torch.bfloat16, use_residual=True)
    _load(moe, 52, cfg)
    gen = torch.Generator(device="cuda").manual_seed(17)
    x = torch.randn(1000, 256, device="cuda", generator=gen)
    gi = torch.randn(1000, 256, device="cuda", generator=gen)
    dy = torch.randn(1000, 256, device="cuda", generator=gen)
    runs = []
    for _ in range(2):
        moe.zero_grad(set_to_none=True)
        xt, gt = x.clone().requires_grad_(True), gi.clone().requires_grad_(True)
        y = moe(xt, gate_input=gt)
        ((y * dy).sum() + y.l_aux).backward()
        runs.append((y.detach(), xt.grad, gt.grad, [p.grad.clone() for p in moe.parameters()]))
    (ya, dxa, dga, pa), (yb, dxb, dgb, pb) = runs
    assert torch.equal(ya, yb) and torch.equal(dxa, dxb) and torch.equal(dga, dgb)
    for (n, _), a, b in zip(moe.named_parameters(), pa, pb):
        assert torch.equal(a, b), n
    assert moe.coefficient.weight.grad.abs().max().item() > 0 and moe.residual_expert.weights[0].grad.abs().max().item() > 0
