"""Dynamic MoE capacity (capacity_factor <= 0, tutel_fast_dispatch.py:210-216): cf = 0 keeps every token and trains on the packed row
space (swn_route_top1_packed + packed ReLU-mask slots, swn_chain_desc.packed_rows); cf < 0 is the static capacity of |cf| (the derivation
in SwitchNeRF.capacity).  Against the reference's own run (scripts/gen_golden_dyncap.py) and against the strided layout."""
import gc
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _model(dtype, seed, gate_scale=1.0, **kw):
    from switch_nerf_amd.model import SwitchNeRF
    m = SwitchNeRF(synth.BUILDING, dtype=dtype, **kw)
    m.load_state_dict(synth.make_weights(seed, synth.BUILDING, gate_scale=gate_scale))
    return m


@pytest.mark.parametrize("tag", ["cf000_bpr", "cf000_nobpr", "cfm050_bpr"])
def test_train_step_dyncap_vs_reference_golden_fp32(tag):
    """The fp32 step (64-row kernels with packed mask slots at cf = 0) against the reference at cf = 0 / -0.5: the assertions of
    test_model_gpu.test_train_step_vs_reference_golden_fp32."""
    g = np.load(os.path.join(G, f"render_train_{tag}.npz"))
    N, S, chunk = int(g["N"]), int(g["S"]), int(g["chunk"])
    cf = float(g["capacity_factor"])
    m = _model(torch.float32, int(g["seed"]), float(g["gate_scale"]), capacity_factor=cf, batch_prioritized=bool(int(g["bpr"])))
    rays, img, rgbs = synth.make_rays(52, N)
    st = m.train_step(_dev(rgbs), _dev(rays), _dev(img), S, chunk, perturb=0.0, optimizer_step=False)
    c = st["ctx"]
    if cf == 0:
        assert c["dyn"] and c["rows"] == N * S and c["packed_rows"] == N * S
        assert bool((c["tok2row"] >= 0).all()), "cf = 0 drops nothing"
    np.testing.assert_array_equal(c["idx"].cpu().numpy().reshape(N, S), g["moe_gates"])
    np.testing.assert_allclose(c["rgb"].cpu().numpy(), g["rgb"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(c["raw"][:, 3].cpu().numpy().reshape(N, S), g["sigma"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(c["depth_variance"].cpu().numpy(), g["depth_variance"], rtol=1e-3, atol=1e-6)
    np.testing.assert_allclose(c["l_aux"].cpu().numpy(), g["gate_loss"], rtol=1e-5)
    np.testing.assert_allclose(st["loss"].item(), float(g["loss"]), rtol=1e-5)
    for k, t in m.grad_dict().items():
        got = t.cpu().numpy()
        ref_sum = g["gsum__" + k]
        scale = max(1e-12, float(ref_sum[1]))
        assert abs(synth.checksum(got)[0] - ref_sum[0]) <= 1e-3 * scale + 1e-9, k
        assert abs(synth.checksum(got)[1] - ref_sum[1]) <= 1e-3 * scale + 1e-9, k
        sl = got.reshape(-1)[:: max(1, got.size // 499)][:499]
        ref = g["gslice__" + k]
        np.testing.assert_allclose(sl, ref, rtol=2e-3, atol=1e-7 + 2e-4 * np.abs(ref).max(), err_msg=k)


@pytest.mark.parametrize("E", [1, 2, 4, 8, 16, 32, 64])
def test_packed_routing_equals_route_top1_and_pack(E):
    """swn_route_top1_packed against swn_route_top1x + swn_route_pack: loc, counts, l_aux, begin, perm, tok2row bit-exact (segments of
    skewed load, ties from quantised gate values, BPR on and off)."""
    from switch_nerf_amd import ops
    gen = torch.Generator().manual_seed(900 + E)
    for seg_tokens, n_seg, skew, quant in ((1000, 3, 0.0, False), (4096, 2, 3.0, True), (37, 5, 1.0, False), (2048, 1, 6.0, True)):
        P = seg_tokens * n_seg
        logits = torch.randn(P, E, generator=gen) + skew * torch.linspace(0, 1, E)
        gates = torch.softmax(logits, 1)
        if quant:      # many exact ties of the ranking key
            gates = torch.softmax((logits * 4).round() / 4, 1)
        gmax, idx = gates.max(1)
        gates, gmax, idx = gates.cuda().contiguous(), gmax.cuda().contiguous(), idx.int().cuda().contiguous()
        for bpr in (True, False):
            loc, counts, perm, tok2row, l_aux = ops.route_top1(idx, gmax, gates, seg_tokens, E, seg_tokens, bpr, want_perm=False)
            begin, perm_p, tok2row_p = ops.route_pack(idx, loc, counts, seg_tokens, E)
            loc2, counts2, begin2, perm2, tok2row2, l_aux2 = ops.route_top1_packed(idx, gmax, gates, seg_tokens, E, bpr)
            torch.cuda.synchronize()
            for a, b, name in ((loc, loc2, "loc"), (counts, counts2, "counts"), (begin, begin2, "begin"), (perm_p, perm2, "perm"),
                               (tok2row_p, tok2row2, "tok2row")):
                assert torch.equal(a, b), (E, seg_tokens, n_seg, bpr, name)
            assert torch.equal(l_aux, l_aux2), (E, seg_tokens, bpr)


def _step(m, batch, S, chunk, **kw):
    rays, img, rgbs = batch
    return m.train_step(_dev(rgbs), _dev(rays), _dev(img), S, chunk, perturb=0.0, optimizer_step=False, **kw)


def _grads_close(a, b, rel=1e-4, exact=()):
    for (k, ta), tb in zip(a.grad_dict().items(), b.grad_dict().values()):
        if k in exact:
            assert torch.equal(ta, tb), k
        else:
            d = (ta - tb).abs().max().item()
            assert d <= rel * max(ta.abs().max().item(), 1e-12), (k, d)


def test_bf16_geometry7_step_cf0_equals_cf_e_and_memory():
    """bf16, 1024 rays x 256 samples, chunk 65536 (geometry 7, fused tail and fused backward): cf = 0 (packed rows) against cf = E
    (capacity = the segment: the same kept rows in the strided layout) - rgb, raw, loss and l_aux bit-identical (a row's chain
    arithmetic does not depend on where it sits).  Gradients: the expert weight gradients run on swn_wgrad_multi over the packed groups
    at cf = 0 and on the row-split swn_wgrad_blocks at cf = E, and the sigma head's fused weight gradient adds its per-tile partial sums
    over packed instead of strided slots - different fp32 summation orders: every gradient is bounded at 1e-4 of its largest entry.
    Peak memory of the cf = 0 step at most 1.15 x that of the cf = 1 step (the strided no-drop layout would need E
    times the ReLU masks)."""
    N, S, chunk = 1024, 256, 65536
    E = synth.BUILDING["num_experts"]
    batch = synth.make_rays(61, N)
    peaks, models, res = {}, {}, {}
    for cf in (1.0, float(E), 0.0):
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        m = _model(torch.bfloat16, 62, capacity_factor=cf)
        r = _step(m, batch, S, chunk)
        torch.cuda.synchronize()
        peaks[cf] = torch.cuda.max_memory_allocated() - base
        c = r["ctx"]
        res[cf] = dict(rgb=c["rgb"].clone(), raw=c["raw"].clone(), l_aux=c["l_aux"].clone(), loss=r["loss"].item(), tail=c["tail_fused"],
                       geom=c["geom"])
        if cf == 1.0:
            del m, r, c
        else:
            models[cf] = m
    a, b = res[0.0], res[float(E)]
    assert a["geom"] == 7 and a["tail"] and b["tail"]
    assert torch.equal(a["rgb"], b["rgb"]) and torch.equal(a["raw"], b["raw"]) and torch.equal(a["l_aux"], b["l_aux"])
    assert a["loss"] == b["loss"]
    _grads_close(models[0.0], models[float(E)])
    print(f"peak bytes: cf=1 {peaks[1.0] / 2**20:.0f} MiB, cf=0 {peaks[0.0] / 2**20:.0f} MiB, cf=E {peaks[float(E)] / 2**20:.0f} MiB")
    assert peaks[0.0] <= 1.15 * peaks[1.0], peaks


def test_graphed_step_cf0_is_bit_identical_to_eager():
    from switch_nerf_amd.graph import GraphedTrainStep
    N, S, chunk = 512, 64, 8192
    batches = [synth.make_rays(730 + i, N) for i in range(3)]
    a, b = _model(torch.bfloat16, 53, capacity_factor=0.0), _model(torch.bfloat16, 53, capacity_factor=0.0)
    rays0, img0, rgbs0 = batches[0]
    step = GraphedTrainStep(a, _dev(rgbs0), _dev(rays0), _dev(img0), S, chunk, perturb=0.0, noise_std=0.0)
    a.load_state_dict(synth.make_weights(53, synth.BUILDING))
    a.m.zero_(); a.v.zero_(); a.step_count = 0
    a.refresh_compute_copies()
    for it, (rays, img, rgbs) in enumerate(batches):
        ra = step(_dev(rgbs), _dev(rays), _dev(img))
        la = ra["loss"].item()
        rb = b.train_step(_dev(rgbs), _dev(rays), _dev(img), S, chunk, perturb=0.0)
        assert ra["ctx"]["dyn"] and torch.equal(ra["ctx"]["idx"], rb["ctx"]["idx"]), it
        assert la == rb["loss"].item(), it
        assert torch.equal(a.grad, b.grad), it
        assert torch.equal(a.flat, b.flat), it


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_hierarchical_fine_pass_cf0(dtype):
    """The coarse + fine step at cf = 0 against cf = E (the same kept rows, strided): forward outputs bit-identical, gradients within
    the summation-order bound of the test above."""
    N, S, F, chunk = 256, 64, 64, 4096
    E = synth.BUILDING["num_experts"]
    batch = synth.make_rays(71, N)
    a, b = _model(dtype, 72, capacity_factor=0.0), _model(dtype, 72, capacity_factor=float(E))
    ra, rb = _step(a, batch, S, chunk, fine_samples=F), _step(b, batch, S, chunk, fine_samples=F)
    assert ra["loss"].item() == rb["loss"].item()
    assert ra["ctx_fine"]["dyn"] and ra["ctx"]["dyn"]
    assert torch.equal(ra["rgb"], rb["rgb"])
    _grads_close(a, b, rel=1e-4 if dtype == torch.float32 else 1e-3)


def test_negative_cf_equals_static_capacity():
    """cf = -0.5 is the static capacity of 0.5 (SwitchNeRF.capacity): the same step bit for bit."""
    N, S, chunk = 512, 128, 16384
    batch = synth.make_rays(81, N)
    a, b = _model(torch.bfloat16, 82, capacity_factor=-0.5), _model(torch.bfloat16, 82, capacity_factor=0.5)
    ra, rb = _step(a, batch, S, chunk), _step(b, batch, S, chunk)
    assert ra["ctx"]["cap"] == rb["ctx"]["cap"] and not ra["ctx"]["dyn"]
    assert bool((ra["ctx"]["tok2row"] < 0).any()), "cf = -0.5 drops tokens like cf = 0.5"
    assert ra["loss"].item() == rb["loss"].item()
    assert torch.equal(ra["ctx"]["rgb"], rb["ctx"]["rgb"])
    assert torch.equal(a.grad, b.grad)


def test_cf0_refuses_expert_parallelism():
    from switch_nerf_amd.model import DYNCAP_EP_ERROR
    m = _model(torch.bfloat16, 83, capacity_factor=0.0)
    with pytest.raises(ValueError, match="expert parallelism"):
        m.set_expert_parallel(SimpleNamespace(E=m.E))
    assert m.ep is None and "capacity_factor = 0" in DYNCAP_EP_ERROR


def _mirror(k, cf, dtype):
    from switch_nerf_amd.moe import moe_layer
    cfg = synth.BUILDING
    return moe_layer(gate_type=dict(type="top", k=k, fp32_gate=True, capacity_factor=cf, batch_prioritized_routing=True, gate_noise=-1.0,
                                    compute_balance_loss=False, dispatcher_no_score=False, is_postscore=True, gate_dim=cfg["gate_hidden"]),
                     model_dim=cfg["model_dim"],
                     experts=dict(type="expertmlp", count_per_node=cfg["num_experts"], hidden_size_per_expert=cfg["model_dim"],
                                  layer_num=cfg["expert_layers"], skips=list(cfg["skips"])),
                     seeds=(1, 1, 1), return_gates=True, dtype=dtype).cuda()


@pytest.mark.parametrize("tag", ["top1_cf000", "top1_cfm050", "top2_cf000"])
def test_moe_layer_dyncap_vs_reference_golden_fp32(tag):
    g = np.load(os.path.join(G, f"moe_layer_dyncap_{tag}.npz"))
    seed, P, k, cf = int(g["seed"]), int(g["P"]), int(g["k"]), float(g["cf"])
    moe = _mirror(k, cf, torch.float32)
    sd = synth.make_weights(seed, synth.BUILDING)
    moe.load_state_dict({n[len("layers.0."):]: torch.from_numpy(v) for n, v in sd.items() if n.startswith("layers.0.")})
    rng = np.random.default_rng(seed + 1000)
    x = rng.standard_normal((P, 256)).astype(np.float32)
    gi = rng.standard_normal((P, 256)).astype(np.float32)
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    gt = torch.from_numpy(gi).cuda().requires_grad_(True)
    y = moe(xt, gate_input=gt)
    np.testing.assert_array_equal(y.gate_extras["gates"].cpu().numpy().reshape(-1), g["topk"].reshape(-1))
    np.testing.assert_allclose(y.l_aux.item(), float(g["l_aux"]), rtol=1e-5)
    dy = rng.standard_normal(tuple(y.shape)).astype(np.float32)
    (y * torch.from_numpy(dy).cuda()).sum().backward()
    # [P, 256] outputs: checksum + a strided slice holding 2 values of every token's row (the fixture keeps no more)
    for n, t, rtol in (("y", y.detach(), 1e-4), ("dx", xt.grad, 1e-3), ("dgate_input", gt.grad, 1e-3)):
        got = t.cpu().numpy()
        ref, ref_sum = g["slice__" + n], g["sum__" + n]
        atol = 5e-5 if n == "y" else 2e-4 * np.abs(ref).max()
        np.testing.assert_allclose(got.reshape(-1)[:: max(1, got.size // 2048)][:2048], ref, rtol=rtol, atol=atol, err_msg=n)
        np.testing.assert_allclose(synth.checksum(got)[1:], ref_sum[1:], rtol=1e-3, err_msg=n)
        assert abs(synth.checksum(got)[0] - ref_sum[0]) <= 1e-3 * ref_sum[1], n
    for n, p in moe.named_parameters():
        got = p.grad.cpu().numpy()
        ref_sum = g["gsum__" + n]
        scale = max(1e-12, float(ref_sum[1]))
        assert abs(synth.checksum(got)[0] - ref_sum[0]) <= 1e-3 * scale + 1e-9, n
        sl = got.reshape(-1)[:: max(1, got.size // 997)][:997]
        ref = g["gslice__" + n]
        np.testing.assert_allclose(sl, ref, rtol=2e-3, atol=1e-7 + 5e-4 * np.abs(ref).max(), err_msg=n)
