"""affine_appearance on the GPU (models/nerf_moe.py:153-161, 426-438): the four entry points of csrc/affine.hip against an fp32 torch
restatement written here, the training step / mip step / model call against the reference model's own run (tests/golden/*affine*.npz,
scripts/gen_golden_affine.py), and the step's other drivers (bf16, graph replay, autograd bridge, split step, no-batch and ragged
evaluation) against the plain step."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import affine_weights as aw
import synth

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _model(dtype, seed, gate_scale=0.02, **kw):
    from switch_nerf_amd.model import SwitchNeRF
    m = SwitchNeRF(aw.affine_cfg(), dtype=dtype, **kw)
    m.load_state_dict(aw.make_affine_weights(seed, gate_scale=gate_scale))
    return m


def _err(name, got, ref):
    e = (got.detach().float().cpu() - ref.detach().float().cpu()).abs().max().item()
    print(f"{name}: max |err| {e:.3e} of {ref.detach().abs().max().item():.3e}")
    return e


def _restate_heads(y, h2, ws, bs, wc, bc, noise, T, S):
    """fp32: raw = [sigmoid(A (h2 Wc^T + bc) + t), softplus(y ws + bs + noise - 1)], [A | t] = T[ray] (nerf_moe.py:392-441, nerf.py:68-69)."""
    lin = h2 @ wc.t() + bc
    Tp = T.view(-1, 3, 4).repeat_interleave(S, 0)
    rgb = torch.sigmoid((Tp[:, :, :3] @ lin[:, :, None]).squeeze(-1) + Tp[:, :, 3])
    sig = torch.nn.functional.softplus(y @ ws + bs + noise - 1.0)
    return torch.cat([rgb, sig[:, None]], 1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N,S", [(5, 13), (64, 64)])
def test_affine_entry_points_vs_fp32_restatement(dtype, N, S):
    """swn_affine_ray_fwd / swn_heads_affine_fwd / swn_heads_affine_bwd / swn_affine_ray_bwd (+ the ordered embedding reduction) at 65
    points (no multiple of a block or a wave) and at 4096, M = 256, H2 = 128.  Tolerances: those of test_kernels_gpu.py's
    test_heads_and_combine_bwd for swn_heads_fwd / swn_heads_bwd (3e-6 forward; dh2 1e-5 fp32 / 1e-2 for 16-bit rows; 1e-3 reductions)."""
    from switch_nerf_amd import ops as o
    rng = np.random.default_rng(1000 + N)
    P, M, H2, A, NI = N * S, 256, 128, 48, 10
    f = lambda *s, scale=1.0: torch.from_numpy((rng.standard_normal(s) * scale).astype(np.float32))
    y, h2 = torch.relu(f(P, M)), torch.relu(f(P, H2))
    y[::7] = 0
    ws, bs, wc, bc, noise = f(M, scale=1 / 16), torch.tensor([0.3]), f(3, H2, scale=1 / 11), f(3, scale=0.1), f(P)
    emb, idx = f(NI, A), torch.from_numpy(aw.affine_image_indices(N, N, NI))
    sd = aw.make_affine_weights(N)
    wa, ba = torch.from_numpy(sd["affine.weight"]), torch.from_numpy(sd["affine.bias"])
    yr, h2r = y.to(dtype).float().requires_grad_(True), h2.to(dtype).float().requires_grad_(True)
    wsr, bsr, wcr, bcr, war, bar, embr = [t.clone().requires_grad_(True) for t in (ws, bs, wc, bc, wa, ba, emb)]
    T_ref = embr[idx] @ war.t() + bar
    T_ref.retain_grad()
    raw_ref = _restate_heads(yr, h2r, wsr, bsr, wcr, bcr, noise, T_ref, S)
    d_raw = f(P, 4)
    (raw_ref * d_raw).sum().backward()
    D = lambda t: t.to(DEV)
    yd, h2d, idxd = D(y).to(dtype), D(h2).to(dtype), D(idx)
    T = o.affine_ray_fwd(D(emb), idxd, D(wa), D(ba))
    assert _err("T", T, T_ref) <= 3e-6
    raw = o.heads_affine_fwd(yd, h2d, D(ws), D(bs), D(wc), D(bc), D(noise), T, S)
    assert _err("raw", raw, raw_ref) <= 3e-6
    # per-row matrices (rows_per_group = 1: the ragged evaluation's form) give the same bits
    raw1 = o.heads_affine_fwd(yd, h2d, D(ws), D(bs), D(wc), D(bc), D(noise), T.repeat_interleave(S, 0).contiguous(), 1)
    assert torch.equal(raw1, raw)
    zeros = lambda: [torch.zeros(M, device=DEV), torch.zeros(1, device=DEV), torch.zeros(3, H2, device=DEV), torch.zeros(3, device=DEV)]
    acc = zeros()
    dh2, dsig, cs, dT = o.heads_affine_bwd(yd, h2d, D(wc), D(bc), T, raw, D(d_raw), *acc, rows_per_group=S)
    assert _err("dh2", dh2, h2r.grad * (h2r > 0)) <= (1e-5 if dtype == torch.float32 else 1e-2)
    for name, got, ref in (("dws", acc[0], wsr.grad), ("dbs", acc[1], bsr.grad), ("dwc", acc[2], wcr.grad), ("dbc", acc[3], bcr.grad),
                           ("dT", dT, T_ref.grad)):
        assert _err(name, got, ref) <= 1e-3, name
    ref_cs = o.group_colsum(dh2, S)
    assert cs.shape == ref_cs.shape and (cs - ref_cs).abs().max().item() <= 2e-5 * max(1.0, ref_cs.abs().max().item())
    dwa, dba, demb = torch.zeros(12, A, device=DEV), torch.zeros(12, device=DEV), torch.zeros(NI, A, device=DEV)
    d_feat = o.affine_ray_bwd(dT, D(emb), idxd, D(wa), dwa, dba)
    o.emb_grad(d_feat, idxd, demb)
    for name, got, ref in (("d_affine_w", dwa, war.grad), ("d_affine_b", dba, bar.grad), ("d_emb", demb, embr.grad)):
        assert _err(name, got, ref) <= 1e-3, name
    assert not demb[aw.UNHIT_IMAGE].any() and demb.abs().sum() > 0
    # a second run: the same bits everywhere (fixed-order sums, no atomics), and the parameter gradients ACCUMULATE
    acc2 = zeros()
    dh2b, dsigb, csb, dTb = o.heads_affine_bwd(yd, h2d, D(wc), D(bc), T, raw, D(d_raw), *acc2, rows_per_group=S)
    dwa2, dba2, demb2 = torch.zeros_like(dwa), torch.zeros_like(dba), torch.zeros_like(demb)
    o.emb_grad(o.affine_ray_bwd(dTb, D(emb), idxd, D(wa), dwa2, dba2), idxd, demb2)
    assert torch.equal(dTb, dT) and torch.equal(demb2, demb) and torch.equal(dwa2, dwa) and torch.equal(dba2, dba)
    assert torch.equal(dh2b, dh2) and torch.equal(dsigb, dsig) and torch.equal(csb, cs) and all(torch.equal(a, b) for a, b in zip(acc, acc2))
    o.heads_affine_bwd(yd, h2d, D(wc), D(bc), T, raw, D(d_raw), *acc2, rows_per_group=S)
    assert all(torch.allclose(t, 2 * f_, rtol=1e-6, atol=0) for t, f_ in zip(acc2, acc))
    o.affine_ray_bwd(dT, D(emb), idxd, D(wa), dwa2, dba2)
    assert torch.allclose(dwa2, 2 * dwa, rtol=1e-6, atol=0) and torch.allclose(dba2, 2 * dba, rtol=1e-6, atol=0)
    # y == NULL: d_w_sigma untouched, everything else the same bits; no column sums asked: the same again
    acc3 = zeros()
    acc3[0].fill_(3.0)
    dh2n, dsign, csn, dTn = o.heads_affine_bwd(None, h2d, D(wc), D(bc), T, raw, D(d_raw), *acc3, rows_per_group=S)
    assert torch.equal(acc3[0], torch.full_like(acc3[0], 3.0)) and all(torch.equal(a, b) for a, b in zip(acc3[1:], acc[1:]))
    assert torch.equal(dh2n, dh2) and torch.equal(dsign, dsig) and torch.equal(csn, cs) and torch.equal(dTn, dT)
    out = o.heads_affine_bwd(yd, h2d, D(wc), D(bc), T, raw, D(d_raw), *zeros(), rows_per_group=S, want_colsum=False)
    assert out[2] is None and torch.equal(out[0], dh2) and torch.equal(out[3], dT)
    # the sigma pre-activation gradient against the restatement (through y's gradient: dy = dsig ws)
    assert _err("dsig", dsig[:, None] * D(ws)[None, :], yr.grad) <= 1e-5


def _check_grads(m, g, tag):
    """tests/test_model_gpu.py's gradient criterion for render_train_*: checksums within 1e-3 of the reference's absolute sum, slices
    rtol 2e-3 / atol 1e-7 + 2e-4 max|ref|."""
    gd = m.grad_dict()
    assert list(gd.keys()) == [str(n) for n in g["names"]]
    worst = 0.0
    for k, t in gd.items():
        got = t.cpu().numpy()
        ref_sum = g["gsum__" + k]
        scale = max(1e-12, float(ref_sum[1]))
        assert abs(synth.checksum(got)[0] - ref_sum[0]) <= 1e-3 * scale + 1e-9, k
        assert abs(synth.checksum(got)[1] - ref_sum[1]) <= 1e-3 * scale + 1e-9, k
        sl = got.reshape(-1)[:: max(1, got.size // 499)][:499]
        ref = g["gslice__" + k]
        worst = max(worst, float(np.abs(sl - ref).max() / (np.abs(ref).max() + 1e-12)))
        np.testing.assert_allclose(sl, ref, rtol=2e-3, atol=1e-7 + 2e-4 * np.abs(ref).max(), err_msg=k)
        if "gfull__" + k in g.files:
            ref = g["gfull__" + k]
            np.testing.assert_allclose(got, ref, rtol=2e-3, atol=1e-7 + 2e-4 * np.abs(ref).max(), err_msg=k)
    print(f"{tag}: worst relative gradient-slice error {worst:.2e}")
    ge = gd["embedding_a.weight"]
    assert not ge[int(g["unhit_image"])].any() and ge.abs().sum() > 0, "the image no ray belongs to: an exactly-zero gradient row"
    assert gd["affine.weight"].abs().sum() > 0 and gd["affine.bias"].abs().sum() > 0


def test_train_step_vs_reference_golden_fp32():
    g = np.load(os.path.join(G, "render_train_affine.npz"))
    N, S, chunk, seed = int(g["N"]), int(g["S"]), int(g["chunk"]), int(g["seed"])
    m = _model(torch.float32, seed, float(g["gate_scale"]))
    rays, _, rgbs = synth.make_rays(seed + 1, N)
    img = aw.affine_image_indices(seed, N)
    st = m.train_step(_dev(rgbs), _dev(rays), _dev(img), S, chunk, perturb=0.0, optimizer_step=False)
    c = st["ctx"]
    assert not c["tail_fused"] and m.kernel_set()["fused_backward"] is False
    assert int((c["idx"].cpu().numpy().reshape(N, S) != g["moe_gates"]).sum()) == 0, "top-1 expert indices must equal the reference's"
    np.testing.assert_allclose(c["rgb"].cpu().numpy(), g["rgb"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(c["raw"][:, 3].cpu().numpy().reshape(N, S), g["sigma"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(c["depth"].cpu().numpy(), g["depth"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(c["l_aux"].cpu().numpy(), g["gate_loss"], rtol=1e-5)
    np.testing.assert_allclose(st["loss"].item(), float(g["loss"]), rtol=1e-5)
    _check_grads(m, g, "affine")
    # the evaluation forward through the render_rays mirror: the same image, the per-point colours are the transformed ones
    from switch_nerf_amd.rendering import render_rays
    hp = Namespace(coarse_samples=S, fine_samples=0, model_chunk_size=chunk, perturb=1.0, use_sigma_noise=False, sigma_noise_std=0.0,
                   affine_appearance=True, return_pts_rgb=True)
    m.eval()
    res, _ = render_rays(m, None, _dev(rays), _dev(img), hp, None, None, True, True, False)
    np.testing.assert_allclose(res["rgb_coarse"].cpu().numpy(), g["rgb"], rtol=0, atol=1e-4)
    assert torch.equal(res["pts_rgb_coarse"].reshape(-1, 3), c["raw"][:, :3])


def test_mip_train_step_vs_reference_golden_fp32():
    g = np.load(os.path.join(G, "render_train_affine_mip.npz"))
    N, S, Fn, chunk, seed = int(g["N"]), int(g["S"]), int(g["F"]), int(g["chunk"]), int(g["seed"])
    m = _model(torch.float32, seed, float(g["gate_scale"]))
    rays, _, rgbs = synth.make_rays(seed + 1, N)
    img = aw.affine_image_indices(seed, N)
    st = m.train_step_mip(_dev(rgbs), _dev(rays), _dev(g["radii"]), _dev(img), S, Fn, chunk, optimizer_step=False, perturb=0.0)
    c, cf = st["ctx"], st["ctx_fine"]
    assert int((c["idx"].cpu().numpy().reshape(N, S - 1) != g["moe_gates_coarse"]).sum()) == 0
    assert int((cf["idx"].cpu().numpy().reshape(N, Fn - 1) != g["moe_gates_fine"]).sum()) == 0
    np.testing.assert_allclose(c["rgb"].cpu().numpy(), g["rgb_coarse"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(cf["rgb"].cpu().numpy(), g["rgb_fine"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(st["loss"].item(), float(g["loss"]), rtol=1e-5)
    _check_grads(m, g, "affine mip")


def test_model_call_vs_reference_golden():
    """SwitchNeRF.__call__ == NeRFMoE.forward with the transform on 4096 points (tolerance of model_fwd_*: 1e-4), sigma_only included."""
    g = np.load(os.path.join(G, "model_fwd_affine.npz"))
    m = _model(torch.float32, int(g["seed"]), float(g["gate_scale"]))
    m.eval()
    r = m(_dev(g["x"]), sigma_noise=_dev(g["sigma_noise"]))
    assert (r["extras"]["moe_gates"][0].cpu().numpy().reshape(-1) != g["moe_gates"].reshape(-1)).sum() == 0
    np.testing.assert_allclose(r["outputs"].cpu().numpy(), g["outputs"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(r["extras"]["moe_loss"].cpu().numpy(), g["moe_loss"], rtol=1e-5)
    r2 = m(_dev(g["x"]), sigma_only=True, sigma_noise=_dev(g["sigma_noise"]))
    assert torch.equal(r2["outputs"], r["outputs"])
    # the identity transform gives back the plain colour head: the transform really is what moves the colours
    sd = aw.make_affine_weights(int(g["seed"]))
    sd["affine.weight"] = np.zeros_like(sd["affine.weight"])
    sd["affine.bias"] = np.eye(3, 4, dtype=np.float32).reshape(-1)
    m.load_state_dict(sd)
    r3 = m(_dev(g["x"]), sigma_noise=_dev(g["sigma_noise"]))["outputs"]
    assert (r3[:, :3] - r["outputs"][:, :3]).abs().max().item() > 1e-2 and torch.equal(r3[:, 3], r["outputs"][:, 3])


def test_bf16_step_close_to_own_fp32_step():
    """The benchmarked dtype at the fixture's shape against this implementation's fp32 run with the same routing: rgb within 2 bf16 ulps
    of 1.0 (2^-7, the bound tests/test_fullsize_gpu.py states for it)."""
    N, S, chunk, seed = 64, 64, 1024, 151
    rays, _, rgbs = synth.make_rays(seed + 1, N)
    img = aw.affine_image_indices(seed, N)
    a = _model(torch.float32, seed).train_step(_dev(rgbs), _dev(rays), _dev(img), S, chunk, perturb=0.0, optimizer_step=False)
    m16 = _model(torch.bfloat16, seed)
    b = m16.train_step(_dev(rgbs), _dev(rays), _dev(img), S, chunk, perturb=0.0, optimizer_step=False, routing_override=a["ctx"]["idx"])
    d = (a["ctx"]["rgb"] - b["ctx"]["rgb"]).abs().max().item()
    print(f"affine bf16 vs fp32 (same routing): max |rgb diff| {d:.3e}")
    assert d <= 2.0 ** -7
    assert torch.isfinite(m16.grad).all() and m16.g["affine.w"].abs().sum() > 0 and not m16.g["emb"][aw.UNHIT_IMAGE].any()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_graphed_train_step_equals_eager(dtype):
    """Three optimizer steps replayed from the captured graph equal three eager steps bit for bit: parameters, Adam state, loss."""
    from switch_nerf_amd.graph import GraphedTrainStep
    N, S, chunk, seed = 128, 64, 4096, 41
    batches = [(synth.make_rays(300 + i, N), aw.affine_image_indices(300 + i, N)) for i in range(3)]
    ma, mb = _model(dtype, seed), _model(dtype, seed)
    (rays0, _, rgbs0), img0 = batches[0]
    step = GraphedTrainStep(ma, _dev(rgbs0), _dev(rays0), _dev(img0), S, chunk, perturb=0.0, noise_std=0.0)
    ma.load_state_dict(aw.make_affine_weights(seed, gate_scale=0.02))
    ma.m.zero_(); ma.v.zero_(); ma.step_count = 0
    ma.refresh_compute_copies()
    for (rays, _, rgbs), img in batches:
        ra = step(_dev(rgbs), _dev(rays), _dev(img))
        la = float(ra["loss"].item())
        rb = mb.train_step(_dev(rgbs), _dev(rays), _dev(img), S, chunk, perturb=0.0)
        assert torch.equal(ra["ctx"]["idx"], rb["ctx"]["idx"]) and la == float(rb["loss"].item())
    assert torch.equal(ma.flat, mb.flat) and torch.equal(ma.m, mb.m) and torch.equal(ma.v, mb.v)
    assert ma.step_count == mb.step_count == 3 and ma.m[ma.spec["affine.w"][0]: ma.spec["affine.w"][0] + 576].abs().sum() > 0


@pytest.mark.parametrize("fine", [0, 64])
def test_autograd_bridge_and_split_step_fill_the_same_gradient_bit_for_bit(fine):
    """loss.backward() through rendering.render_rays puts grad_step's gradient into flat_param.grad - hierarchical pass included - and
    torch.optim.Adam then moves the affine parameters; grad_step(split=True) + backward_net_b is the plain step."""
    from switch_nerf_amd.rendering import render_rays
    N, S, chunk, seed = 64, 64, 1024, 401
    rays, _, rgbs = synth.make_rays(402, N)
    img = aw.affine_image_indices(402, N)
    a, b = _model(torch.float32, seed), _model(torch.float32, seed)
    st = a.grad_step(_dev(rgbs), _dev(rays), _dev(img), S, chunk, perturb=0.0, fine_samples=fine)
    hp = Namespace(coarse_samples=S, fine_samples=fine, model_chunk_size=chunk, perturb=0.0, use_sigma_noise=False, sigma_noise_std=0.0,
                   use_cascade=False, affine_appearance=True)
    opt = torch.optim.Adam(b.trainable_parameters(), lr=5e-4)
    res, _ = render_rays(b, None, _dev(rays), _dev(img), hp, None, None, True, True, False)
    typ = "fine" if fine else "coarse"
    gate_loss = res["gate_loss_coarse"].mean()
    if fine:
        gate_loss = (res["gate_loss_fine"].mean() + gate_loss) / 2
    loss = torch.nn.functional.mse_loss(res[f"rgb_{typ}"], _dev(rgbs)) + b.wt * gate_loss
    loss.backward()
    assert torch.equal(b.flat_param.grad, a.grad), (b.flat_param.grad - a.grad).abs().max().item()
    assert a.g["affine.w"].abs().sum() > 0 and a.g["emb"].abs().sum() > 0 and not a.g["emb"][aw.UNHIT_IMAGE].any()
    before = b.p["affine.w"].clone()
    opt.step()
    assert not torch.equal(b.p["affine.w"], before)
    if not fine:
        c = _model(torch.float32, seed)
        st2 = c.grad_step(_dev(rgbs), _dev(rays), _dev(img), S, chunk, perturb=0.0, split=True)
        c.backward_net_b(st2["bwd_b"])
        torch.cuda.synchronize()
        assert torch.equal(c.grad, a.grad) and st2["loss"].item() == st["loss"].item()


def test_no_batch_and_ragged_evaluation_apply_the_transform():
    """Evaluation without token dropping (set_no_batch) and with a ragged last model chunk: raw equals the restatement on the pass's own
    y / h2 rows with each row's ray matrix; kept tokens of the capacity path agree with the no-batch path."""
    from switch_nerf_amd import ops as o
    seed = 151
    m = _model(torch.float32, seed)
    p = m.p

    def restated(c, S):
        T = o.affine_ray_fwd(p["emb"], c["image_indices"].contiguous(), p["affine.w"], p["affine.b"])
        parts = c.get("parts") or (c,)
        y, h2 = torch.cat([q["y"] for q in parts]).float(), torch.cat([q["h2"] for q in parts]).float()
        return _restate_heads(y, h2, p["sigma.w"], p["sigma.b"], p["color.w"], p["color.b"], 0.0, T, S)
    N, S = 64, 64
    rays, _, _ = synth.make_rays(seed + 1, N)
    img = _dev(aw.affine_image_indices(seed, N))
    cb = m.forward_rays(_dev(rays), img, S, 1024, training=False)
    assert _err("batch raw", cb["raw"], restated(cb, S)) <= 3e-6          # (before the next pass reuses the activation buffers)
    raw_b, kept = cb["raw"].clone(), (cb["tok2row"].view(-1) >= 0).clone()
    cn = m.forward_rays(_dev(rays), img, S, 1024, training=False, no_batch=True)
    assert _err("no-batch raw", cn["raw"], restated(cn, S)) <= 3e-6
    assert int(kept.sum()) > 0 and (raw_b[kept] - cn["raw"][kept]).abs().max().item() <= 1e-5
    # 5 rays x 13 samples in chunks of 32: two whole chunks + one row, rays cut by the chunk borders
    rays, _, _ = synth.make_rays(seed + 2, 5)
    img = _dev(aw.affine_image_indices(seed + 2, 5))
    cr = m.forward_rays(_dev(rays), img, 13, 32, training=False)
    assert cr.get("ragged") and cr["raw"].shape == (65, 4)
    assert _err("ragged raw", cr["raw"], restated(cr, 13)) <= 3e-6
    # the backward of a ragged training batch is not built: it says so
    rgbs = torch.rand(5, 3, device="cuda")
    with pytest.raises(NotImplementedError, match="affine_appearance"):
        m.train_step(rgbs, _dev(rays), img, 13, 32, perturb=0.0, optimizer_step=False)
