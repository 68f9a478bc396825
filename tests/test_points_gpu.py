"""Per-sample point outputs of render_rays (pts / pts_rgb / pts_alpha / alpha, rendering.py:299, :413-452) against the reference's own
eval-mode run (scripts/gen_golden_points.py), the device PLY packer (swn_points_pack) against the numpy restatement byte for byte,
the image export (points.render_image_points), and the absence of side effects on the rendered results."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import points_restate as PR
import synth

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
CENTER, RADIUS = synth.SPHERE_CENTER, synth.SPHERE_RADIUS
FLAGS = dict(return_pts=True, return_pts_rgb=True, return_pts_alpha=True, return_alpha=True)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _h(S, F, chunk, **kw):
    h = Namespace(coarse_samples=S, fine_samples=F, model_chunk_size=chunk, perturb=0.0, use_sigma_noise=False, sigma_noise_std=1.0,
                  use_cascade=False, moe_return_gates=True, return_sigma=False, moe_expert_num=synth.BUILDING["num_experts"],
                  appearance_dim=48)
    for k, v in kw.items():
        setattr(h, k, v)
    return h


def _scene(name, dtype=torch.float32):
    """(model, bg model or None, rays, image indices, hparams, fixture) of a points_* fixture, in eval mode."""
    from switch_nerf_amd.model import SwitchNeRF
    from switch_nerf_amd.dense import DenseNeRF
    g = np.load(os.path.join(G, f"points_{name}.npz"))
    N, S, F, chunk = int(g["N"]), int(g["S"]), int(g["F"]), int(g["chunk"])
    bg = None
    if name == "dense":
        m = DenseNeRF(synth.DENSE, dtype=dtype)
        m.load_state_dict(synth.make_dense_weights(int(g["seed"]), synth.DENSE))
        rays, img, _ = synth.make_rays(int(g["rays_seed"]), N)
        h = _h(S, F, chunk, moe_return_gates=False)
    else:
        m = SwitchNeRF(synth.BUILDING, dtype=dtype)
        m.load_state_dict(synth.make_weights(int(g["seed"]), synth.BUILDING, gate_scale=float(g["gate_scale"])))
        if name == "bg":
            bg = DenseNeRF(synth.DENSE_BG, dtype=dtype)
            bg.load_state_dict(synth.make_dense_weights(int(g["seed_bg"]), synth.DENSE_BG))
            bg.eval()
            rays, img, _ = synth.make_bg_rays(int(g["rays_seed"]), N)
        else:
            rays, img, _ = synth.make_rays(int(g["rays_seed"]), N)
        h = _h(S, F, chunk)
    m.eval()
    return m, bg, _dev(rays), _dev(img), h, g


def _render(m, bg, rays, img, h, **flags):
    from switch_nerf_amd import rendering
    hh = Namespace(**vars(h))
    for k, v in flags.items():
        setattr(hh, k, v)
    res, _ = rendering.render_rays(m, bg, rays, img, hh, CENTER if bg is not None else None, RADIUS if bg is not None else None,
                                   True, True, bg is not None)
    return res


@pytest.mark.parametrize("name", ["coarse", "fine", "bg", "dense"])
def test_point_keys_vs_reference_golden_fp32(name):
    m, bg, rays, img, h, g = _scene(name)
    res = _render(m, bg, rays, img, h, **FLAGS)
    N, S, F = int(g["N"]), int(g["S"]), int(g["F"])
    typs = ("coarse", "fine") if F else ("coarse",)
    for typ in typs:
        n = S if typ == "coarse" else F
        assert res[f"pts_{typ}"].shape == (N, n, 3) and res[f"pts_rgb_{typ}"].shape == (N, n, 3)
        assert res[f"pts_alpha_{typ}"].shape == (N, n)
        assert res[f"alpha_{typ}"].shape == ((N, S) if typ == "coarse" else (N, S + F))
        for k in ("pts", "pts_rgb", "pts_alpha", "alpha"):
            assert res[f"{k}_{typ}"].dtype == torch.float32 and not res[f"{k}_{typ}"].requires_grad
        ok = np.ones(N, bool)
        if name != "dense":
            gates = res[f"moe_gates_{typ}"].cpu().numpy().reshape(N, n)
            diff = gates != g[f"moe_gates_{typ}"]
            if name == "bg" and typ == "fine":
                # the fine depths of the bounded rays come from the importance sampler within ~1e-6 of the reference's, and a sample
                # whose router logits are that close to a tie may pick the other expert: at most 1 in 1000 samples, whose rays
                # are left out of the value checks below
                assert diff.mean() <= 1e-3, diff.sum()
                ok = ~diff.any(1)
            else:
                np.testing.assert_array_equal(gates, g[f"moe_gates_{typ}"], err_msg=typ)
        pts = res[f"pts_{typ}"].cpu().numpy()
        if typ == "coarse" and name != "bg":
            np.testing.assert_array_equal(pts, g[f"pts_{typ}"])                                   # bit-equal
        else:
            np.testing.assert_allclose(pts, g[f"pts_{typ}"], rtol=0, atol=1e-5, err_msg=typ)
        for k in ("pts_rgb", "pts_alpha", "alpha"):
            np.testing.assert_allclose(res[f"{k}_{typ}"].cpu().numpy()[ok], g[f"{k}_{typ}"][ok], rtol=0, atol=1e-4, err_msg=f"{k}_{typ}")
    if name == "bg":
        # rays with a background: the coarse alpha's last sample uses fg_far - max(z_coarse), not 1e10
        hb = g["has_bg"] > 0
        last = res["alpha_coarse"].cpu().numpy()[:, -1]
        assert (last[hb] < 1.0).any()
        np.testing.assert_allclose(last[hb], g["alpha_coarse"][hb, -1], rtol=0, atol=1e-4)


def _synthetic(R, S, E, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    pts = torch.randn(R, S, 3, device="cuda", generator=gen)
    raw = torch.rand(R * S, 4, device="cuda", generator=gen)
    alpha = torch.rand(R, S, device="cuda", generator=gen)
    # exact 0, 1 and k/255 boundaries (and their float32 neighbours) in the quantised channels
    k = torch.randint(0, 256, (R * S,), device="cuda", generator=gen).float() / 255.0
    edge = torch.stack([k, torch.nextafter(k, torch.zeros_like(k)), torch.nextafter(k, torch.ones_like(k)), torch.zeros_like(k),
                        torch.ones_like(k)], 1)
    pick = torch.randint(0, 5, (R * S, 4), device="cuda", generator=gen)
    sel = torch.rand(R * S, 4, device="cuda", generator=gen) < 0.5
    raw = torch.where(sel, edge.gather(1, pick.view(-1, 4)[:, :4] % 5), raw).clamp(0, 1).contiguous()
    alpha = torch.where(sel[:, 3].view(R, S), raw[:, 3].view(R, S), alpha).contiguous()
    # experts: only the even ones plus the last are used (empty experts in between)
    used = torch.tensor([e for e in range(E) if e % 2 == 0 or e == E - 1], device="cuda", dtype=torch.int32)
    idx = used[torch.randint(0, used.numel(), (R * S,), device="cuda", generator=gen)].contiguous()
    pixel = torch.rand(R, 3, device="cuda", generator=gen)
    pixel[::7] = 1.0
    pixel[1::7] = 0.0
    return pts, raw, alpha, idx, pixel


def _check_pack(mode, dev, host, skip, E, rgb_view=True):
    """dev, host: (pts, raw, alpha, idx, pixel) on the device / the same arrays in numpy."""
    from switch_nerf_amd import ops, points
    pts, raw, alpha, idx, pixel = dev
    R, S = pts.shape[:2]
    palette = torch.from_numpy(points.VOC_PALETTE[:E].copy()).cuda()
    rgb = raw[:, :3].view(R, S, 3) if rgb_view else raw[:, :3].reshape(R, S, 3).contiguous()
    out_all, out_exp, counts = ops.points_pack(pts, alpha, mode, skip, idx, E, rgb, pixel, palette)
    torch.cuda.synchronize()
    hp, hr, ha, hi, hx = host
    ref = PR.records(mode, hp, ha, skip, hi.reshape(R, S), hr[:, :3].reshape(R, S, 3), hx, points.VOC_PALETTE[:E])
    assert np.array_equal(out_all.cpu().numpy(), ref.view(np.uint8)), (mode, skip, E)
    parts = PR.by_expert(ref, hi.reshape(R, S), skip, E)
    assert counts.cpu().numpy().tolist() == [len(p) for p in parts]
    assert any(len(p) == 0 for p in parts)
    assert np.array_equal(out_exp.cpu().numpy(), np.concatenate(parts).view(np.uint8)), (mode, skip, E)
    return out_all, out_exp, counts


def test_points_pack_bytes_vs_restatement_large():
    R, S = 65536 + 37, 256
    for E, seed in ((8, 5), (16, 6)):
        dev = _synthetic(R, S, E, seed)
        host = [t.cpu().numpy() for t in dev]
        for skip in (1, 3, 4):
            _check_pack(PR.RGBA, dev, host, skip, E, rgb_view=(skip != 3))
        for mode, skip in ((PR.SEG_ALPHA, 3), (PR.SEG_RGB, 4), (PR.SEG_RGB, 1)):
            _check_pack(mode, dev, host, skip, E)
        del dev, host
        torch.cuda.empty_cache()


def test_points_pack_deterministic_and_small_shapes():
    from switch_nerf_amd import ops, points
    pts, raw, alpha, idx, pixel = _synthetic(4099, 37, 16, 9)
    rgb = raw[:, :3].view(4099, 37, 3)
    palette = torch.from_numpy(points.VOC_PALETTE[:16].copy()).cuda()
    a = ops.points_pack(pts, alpha, PR.SEG_ALPHA, 4, idx, 16, rgb, pixel, palette)
    b = ops.points_pack(pts, alpha, PR.SEG_ALPHA, 4, idx, 16, rgb, pixel, palette)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for R, S, skip in ((1, 1, 1), (3, 5, 7), (65, 64, 64), (200, 130, 2)):
        p, r, al, ix, px = _synthetic(R, S, 8, R + S)
        for mode in (PR.RGBA, PR.SEG_ALPHA, PR.SEG_RGB):
            out_all, out_exp, counts = ops.points_pack(p, al, mode, skip, ix, 8, r[:, :3].view(R, S, 3), px,
                                                       torch.from_numpy(points.VOC_PALETTE[:8].copy()).cuda())
            ref = PR.records(mode, p.cpu().numpy(), al.cpu().numpy(), skip, ix.cpu().numpy().reshape(R, S),
                             r[:, :3].reshape(R, S, 3).cpu().numpy(), px.cpu().numpy(), points.VOC_PALETTE[:8])
            assert np.array_equal(out_all.cpu().numpy(), ref.view(np.uint8))
            parts = PR.by_expert(ref, ix.cpu().numpy().reshape(R, S), skip, 8)
            assert np.array_equal(out_exp.cpu().numpy(), np.concatenate(parts).view(np.uint8))
    # the dense NeRF: no partition
    out_all, out_exp, counts = ops.points_pack(pts, alpha, PR.RGBA, 3, None, 1, rgb)
    assert out_exp is None and counts is None
    ref = PR.records(PR.RGBA, pts.cpu().numpy(), alpha.cpu().numpy(), 3, pts_rgb=raw[:, :3].reshape(4099, 37, 3).cpu().numpy())
    assert np.array_equal(out_all.cpu().numpy(), ref.view(np.uint8))


def _batched_keys(m, bg, rays, img, h, step, typs):
    """The GPU's own point keys of the same pixel batches render_image_points runs, concatenated over the image."""
    keys = {}
    for i in range(0, rays.shape[0], step):
        res = _render(m, bg, rays[i:i + step].contiguous(), img[i:i + step].contiguous(), h, return_pts=True, return_pts_rgb=True,
                      return_pts_alpha=True, moe_return_gates=True)
        res["pixel"] = res["rgb_fine"] if "rgb_fine" in res else res["rgb_coarse"]
        for k in ["pixel"] + [f"{a}_{t}" for t in typs for a in ("pts", "pts_rgb", "pts_alpha", "moe_gates")]:
            keys.setdefault(k, []).append(res[k].cpu())
    return {k: torch.cat(v).numpy() for k, v in keys.items()}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_render_image_points_files(tmp_path, dtype):
    from switch_nerf_amd import points
    m, bg, rays, img, h, g = _scene("coarse", dtype)
    N, S, E = int(g["N"]), int(g["S"]), synth.BUILDING["num_experts"]
    # pixel batches of 48 rays: ragged (48 + 16), each model chunk of 1024 samples holds the same 16 rays as the fixture's run
    h = _h(S, 0, int(g["chunk"]), image_pixel_batch_size=48, render_test_points_typ=["coarse"], render_test_points_sample_skip=3,
           return_pts_class_seg=True)
    out = points.render_image_points(m, None, rays, img, h, str(tmp_path), 7)
    names = points.point_file_names(7, "coarse", E, True)
    assert sorted(out) == sorted(names) == sorted(os.listdir(tmp_path))
    k = _batched_keys(m, None, rays, img, h, 48, ("coarse",))
    gates = k["moe_gates_coarse"].reshape(N, S)
    pal = points.VOC_PALETTE[:E]
    for mode, stem in ((PR.RGBA, "pts_rgba"), (PR.SEG_ALPHA, "top_0_alpha"), (PR.SEG_RGB, "top_0")):
        ref = PR.records(mode, k["pts_coarse"], k["pts_alpha_coarse"], 3, gates, k["pts_rgb_coarse"], k["pixel"], pal)
        parts = PR.by_expert(ref, gates, 3, E)
        all_name = f"007_coarse_{stem}.ply"
        exp_name = (lambda e: f"007_coarse_pts_rgba_top_0_exp_{e}.ply") if mode == PR.RGBA else (lambda e: f"007_coarse_{stem}_exp_{e}.ply")
        _, body = PR.read_ply(str(tmp_path / all_name))
        assert body.dtype == ref.dtype and np.array_equal(body, ref), all_name
        assert out[all_name] == len(ref)
        for e in range(E):
            _, body = PR.read_ply(str(tmp_path / exp_name(e)))
            assert np.array_equal(body, parts[e]), exp_name(e)
            assert out[exp_name(e)] == len(parts[e])
        if dtype == torch.float32 and mode == PR.RGBA:
            # against the reference's arrays: the same expert membership, quantised channels within one level
            gref = g["moe_gates_coarse"]
            gold = PR.records(mode, g["pts_coarse"], g["pts_alpha_coarse"], 3, gref, g["pts_rgb_coarse"], g["rgb"], pal)
            assert [len(p) for p in PR.by_expert(gold, gref, 3, E)] == [len(p) for p in parts]
            for c in ("red", "green", "blue", "alpha"):
                assert np.abs(gold[c].astype(int) - ref[c].astype(int)).max() <= 1, c
            np.testing.assert_allclose(ref["x"], gold["x"], rtol=0, atol=1e-5)


def test_render_image_points_dense_and_fine(tmp_path):
    from switch_nerf_amd import points
    m, _, rays, img, h, g = _scene("dense")
    h = _h(int(g["S"]), 0, int(g["chunk"]), moe_return_gates=False, image_pixel_batch_size=100, render_test_points_typ=["coarse"],
           render_test_points_sample_skip=4, return_pts_class_seg=True)
    out = points.render_image_points(m, None, rays, img, h, str(tmp_path / "d"), 0)
    assert list(out) == ["000_coarse_pts_rgba.ply"] and out["000_coarse_pts_rgba.ply"] == int(g["N"]) * 16
    m, _, rays, img, h, g = _scene("fine")
    h = _h(int(g["S"]), int(g["F"]), int(g["chunk"]), image_pixel_batch_size=40, render_test_points_typ=["coarse", "fine"],
           render_test_points_sample_skip=1)
    out = points.render_image_points(m, None, rays, img, h, str(tmp_path / "f"), 1)
    k = _batched_keys(m, None, rays, img, h, 40, ("fine",))
    N, F = int(g["N"]), int(g["F"])
    ref = PR.records(PR.RGBA, k["pts_fine"], k["pts_alpha_fine"], 1, pts_rgb=k["pts_rgb_fine"])
    _, body = PR.read_ply(str(tmp_path / "f" / "001_fine_pts_rgba.ply"))
    assert np.array_equal(body, ref)
    assert out["001_coarse_pts_rgba.ply"] == N * int(g["S"]) and out["001_fine_pts_rgba.ply"] == N * F
    assert sum(out[f"001_fine_pts_rgba_top_0_exp_{e}.ply"] for e in range(synth.BUILDING["num_experts"])) == N * F


@pytest.mark.parametrize("name", ["coarse", "fine", "bg"])
def test_point_flags_have_no_side_effects(name):
    m, bg, rays, img, h, _ = _scene(name)
    off = _render(m, bg, rays, img, h)
    on = _render(m, bg, rays, img, h, **FLAGS)
    for k, v in off.items():
        assert torch.equal(v, on[k]), k
    assert set(on) - set(off) and all(k.split("_")[0] in ("pts", "alpha") for k in set(on) - set(off))
    if bg is None:
        m.graph_eval = True
        try:
            gr = _render(m, bg, rays, img, h, **FLAGS)
        finally:
            m.graph_eval = False
        assert set(gr) == set(on)
        for k, v in on.items():
            assert torch.equal(v, gr[k]), k


def test_point_keys_in_training_branch():
    """Under autograd (training) the point keys come out detached and equal the eval keys' values at perturb 0, no noise."""
    m, _, rays, img, h, g = _scene("fine")
    ev = _render(m, None, rays, img, h, **FLAGS)
    m.train()
    tr = _render(m, None, rays, img, h, **FLAGS)
    assert tr["rgb_fine"].requires_grad
    for k in ("pts_coarse", "pts_fine", "pts_rgb_coarse", "pts_rgb_fine", "pts_alpha_fine", "alpha_fine", "alpha_coarse"):
        assert not tr[k].requires_grad, k
        assert tr[k].shape == ev[k].shape, k
    np.testing.assert_array_equal(tr["pts_coarse"].cpu().numpy(), ev["pts_coarse"].cpu().numpy())
