"""The Mega-NeRF spatial-cell model with spherical-harmonics sub-models on the HIP path (switch_nerf_amd/mega.py: cell router, DenseNeRF
cfg["sh_deg"] sub-models, swn_cells_blend_sh) against the reference's own MegaNeRF over NeRF(rgb_dim = 3 B), its eval_sh + sigmoid and its
render_rays (tests/golden/mega_sh_*.npz, scripts/gen_golden_mega_sh.py), at the tolerances of tests/test_mega_gpu.py: rgb 1e-4
absolute, sigma (and the raw coefficients, unbounded like it) 1e-4 relative + absolute; the render tests at that file's render bounds.
Points whose float32 membership is not the float64 one (excluded_*: none in the committed fixtures) are left out."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import mega_sh_restate as RS
import sh_weights as SW
import synth

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
_cache = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _load(name):
    return np.load(os.path.join(G, name + ".npz"))


def _mega(name, margin, dtype=torch.float32):
    """The model of a fixture, built once per (fixture, dtype): the margin is an attribute."""
    from switch_nerf_amd.mega import MegaNeRF
    g = _load(name)
    if (name, dtype) not in _cache:
        cfg = {k[5:]: (tuple(int(v) for v in g[k]) if g[k].ndim else int(g[k])) for k in g.files if k.startswith("cfg__")}
        sds = [SW.make_sh_weights(int(g["seed"]) + i, int(g["deg"]), cfg) for i in range(len(g["centroids"]))]
        for sd, ref in zip(sds, g["sd_checksums"]):
            np.testing.assert_allclose(np.sum([synth.checksum(v) for v in sd.values()], 0), ref, rtol=1e-12)
        # (cfg None: the configuration, sh_deg included, is read off the state dicts)
        _cache[(name, dtype)] = MegaNeRF.from_state_dicts(sds, g["centroids"], None, boundary_margin=margin, xyz_real=bool(g["xyz_real"]),
                                                         cluster_2d=bool(g["cluster_2d"]), dtype=dtype)
    m = _cache[(name, dtype)]
    m.boundary_margin = float(margin)
    assert m.sh_deg == int(g["deg"])
    return m, g


CASES = [("mega_sh_fg_d0", "m100", 1.0), ("mega_sh_fg_d0", "m115", 1.15), ("mega_sh_fg_d2", "m100", 1.0), ("mega_sh_fg_d2", "m115", 1.15),
         ("mega_sh_fg_d4", "m100", 1.0), ("mega_sh_fg_d4", "m115", 1.15), ("mega_sh_bg", "m115", 1.15)]


@pytest.mark.parametrize("name,tag,margin", CASES)
def test_mega_sh_forward_vs_reference_golden_fp32(name, tag, margin):
    m, g = _mega(name, margin)
    keep = ~g["excluded_" + tag]
    assert keep.mean() >= 0.99
    x, noise, dirs = _dev(g["x"]), _dev(g["sigma_noise"]), _dev(g["dirs"])
    B = (int(g["deg"]) + 1) ** 2
    # the module mirror: blended raw rows
    out = m(x, sigma_noise=noise).cpu().numpy()
    ref = g["out_" + tag]
    assert out.shape == ref.shape == (len(x), 3 * B + 1)
    np.testing.assert_allclose(out[keep], ref[keep], rtol=1e-4, atol=1e-4)
    rgb_of_rows = RS.eval_rows(out, g["dirs"], 1, int(g["deg"]))[:, :3]          # rendering.py:344-347 on the module's output
    np.testing.assert_allclose(rgb_of_rows[keep], g["raw_" + tag][keep, :3], rtol=0, atol=1e-4)
    # the fused form
    raw = m.call_rgb(x, dirs, 1, sigma_noise=noise).cpu().numpy()
    rr = g["raw_" + tag]
    assert raw.shape == rr.shape == (len(x), 4)
    print(f"{name} {tag}: rgb err {np.abs(raw - rr)[keep, :3].max():.3e}, sigma err {np.abs(raw - rr)[keep, 3].max():.3e}")
    np.testing.assert_allclose(raw[keep, :3], rr[keep, :3], rtol=0, atol=1e-4)
    np.testing.assert_allclose(raw[keep, 3], rr[keep, 3], rtol=1e-4, atol=1e-4)
    assert raw[:, 3].tobytes() == out[:, 3 * B].tobytes()                       # (one blend, two outputs)
    n_pos = 7 if bool(g["xyz_real"]) else 3
    sig = m(x[:, :n_pos].contiguous(), sigma_only=True, sigma_noise=noise).cpu().numpy()
    assert sig.shape == g["sigma_" + tag].shape == (len(ref), 1)
    np.testing.assert_allclose(sig[keep], g["sigma_" + tag][keep], rtol=1e-4, atol=1e-4)
    w, counts, begin, rows, slot = m.route(x)
    np.testing.assert_array_equal((w.cpu().numpy() > 0)[keep], (g["weights_" + tag] > 0)[keep])
    with pytest.raises(Exception, match="Unexpected input shape"):
        m(torch.cat([x, x[:, :3]], 1))                                          # (direction columns are not an SH model's input)


def test_mega_sh_one_direction_per_ray_and_chunks_are_bit_equal():
    """rows_per_group = 8 equals the per-point form with the direction repeated; evaluation in chunks (whole rays, with a ragged last
    chunk; and chunks shorter than a ray, which take per-point directions) equals the unchunked call bit for bit."""
    from switch_nerf_amd import mega
    m, g = _mega("mega_sh_fg_d2", 1.15)
    x = _dev(g["x"])
    P, S = len(x), 8
    dirs = _dev(g["dirs"][: P // S])
    whole = m.call_rgb(x, dirs, S)
    per_point = m.call_rgb(x, dirs.repeat_interleave(S, 0).contiguous(), 1)
    assert torch.equal(whole, per_point)
    for chunk in (1000, 72, 24, 9, 5):                  # 32 rays: one chunk; 9 rays x 3 + 5; 3 rays x 10 + 2; 1 ray each; 5 points (ragged: 256 = 51 x 5 + 1)
        assert torch.equal(mega._run(m, x, chunk, dirs), whole), chunk
    rows = m(x)
    assert torch.equal(torch.cat([m(x[i:i + 100]) for i in range(0, P, 100)], 0), rows)


@pytest.mark.parametrize("typ", ["coarse", "fine"])
def test_mega_sh_render_rays_vs_reference_golden(typ):
    """rendering.render_rays with hparams.sh_deg = 2 and both MegaNeRFs of a container: coarse with the ray's exit from the bound in
    front of the background points; fine (32 + 16 fine samples) with cluster_2d.  A ragged last model chunk (1000 points: 31 rays of 32
    samples + 8 points); a second chunk size gives the same bits."""
    from switch_nerf_amd.mega import MegaNeRF
    from switch_nerf_amd.rendering import render_rays
    g = _load("mega_sh_render")
    models = []
    for name, seed, xyz_real in (("mega_sh_fg_d2", int(g["seed"]), False), ("mega_sh_bg", int(g["seed_bg"]), True)):
        m, f = _mega(name, float(g["margin"]))
        assert int(f["seed"]) == seed
        models.append(MegaNeRF(m.sub_modules, g["centroids"], float(g["margin"]), xyz_real, bool(g["cluster_2d_" + typ])))
    rays, img = _dev(g["rays"]), _dev(g["image_indices"])
    h = Namespace(coarse_samples=int(g["S"]), fine_samples=int(g["F"]) if typ == "fine" else 0, model_chunk_size=1000, perturb=1.0,
                  use_sigma_noise=True, sigma_noise_std=1.0, sh_deg=int(g["deg"]), return_pts_rgb=True)
    res, present = render_rays(models[0], models[1], rays, img, h, g["sphere_center"], g["sphere_radius"], True, True, True)
    assert present is True
    r = {k: v.cpu().numpy() for k, v in res.items()}
    for k in ("rgb", "fg_rgb", "bg_rgb"):
        print(f"{typ} {k}: err {np.abs(r[k + '_' + typ] - g[k + '_' + typ]).max():.3e}")
    np.testing.assert_allclose(r["fg_rgb_" + typ], g["fg_rgb_" + typ], rtol=0, atol=1e-4)
    np.testing.assert_allclose(r["bg_rgb_" + typ], g["bg_rgb_" + typ], rtol=0, atol=1e-4)
    np.testing.assert_allclose(r["rgb_" + typ], g["rgb_" + typ], rtol=0, atol=1e-4)
    np.testing.assert_allclose(r["depth_" + typ], g["depth_" + typ], rtol=2e-3, atol=1e-4)
    np.testing.assert_allclose(r["depth_variance_" + typ], g["depth_variance_" + typ], rtol=2e-3, atol=1e-6)
    pts_rgb = r["pts_rgb_coarse"]                        # the point outputs report the colours behind the sigmoid
    assert pts_rgb.shape[-1] == 3 and ((pts_rgb > 0) & (pts_rgb < 1)).all()
    h.model_chunk_size = 7                               # (shorter than a ray: per-point directions)
    res2, _ = render_rays(models[0], models[1], rays, img, h, g["sphere_center"], g["sphere_radius"], True, True, True)
    assert set(res2) == set(res) and all(torch.equal(res2[k], res[k]) for k in res)


def test_sh_dense_xyz4_call_vs_reference_forward():
    """DenseNeRF(sh_deg, xyz_dim 4).__call__ on [P, 4 + 1] inverted-sphere points + image index -> [P, 3 B + 1], against the reference
    NeRF's forward on cell 0's points of the background fixture (its packed per-cell outputs); sigma_only on [P, 4] -> [P, 1]."""
    m, g = _mega("mega_sh_bg", 1.15)
    mask = g["weights_m115"][:, 0] > 0
    n = int(mask.sum())
    ref = g["sub_m115"][:n]
    sub = m.sub_modules[0]
    assert sub.xyz_dim == 4 and sub.sh_deg == 2
    x, noise = _dev(g["x"][mask][:, 3:]), _dev(g["sigma_noise"][mask])
    out = sub(x, sigma_noise=noise).cpu().numpy()
    assert out.shape == ref.shape == (n, 28)
    print(f"xyz_dim 4 sh call: max err {np.abs(out - ref).max():.3e}")
    np.testing.assert_allclose(out, ref, rtol=1e-4, atol=1e-4)
    sig = sub(x[:, :4].contiguous(), sigma_only=True, sigma_noise=noise)
    assert sig.shape == (n, 1) and sig.cpu().numpy().tobytes() == out[:, 27:28].tobytes()
    with pytest.raises(Exception, match="Unexpected input shape"):
        sub(torch.cat([x, x[:, :3]], 1))


def test_mega_sh_bf16_close_to_fp32():
    _, g = _mega("mega_sh_fg_d2", 1.15)
    x, dirs = _dev(g["x"]), _dev(g["dirs"])
    a = _mega("mega_sh_fg_d2", 1.15)[0].call_rgb(x, dirs).cpu().numpy()
    b = _mega("mega_sh_fg_d2", 1.15, torch.bfloat16)[0].call_rgb(x, dirs).cpu().numpy()
    assert np.isfinite(b).all()
    print(f"bf16 vs fp32: rgb {np.abs(a - b)[:, :3].max():.3e}, sigma {np.abs(a - b)[:, 3].max():.3e}")
    assert np.abs(a - b)[:, :3].max() < 3e-2           # the bound of tests/test_mega_gpu.py::test_mega_bf16_close_to_fp32
    assert np.abs(a - b)[:, 3].max() < 3e-2 * np.abs(a[:, 3]).max()


def test_mega_sh_refusals_that_remain():
    from switch_nerf_amd.background import BackgroundScene
    from switch_nerf_amd.dense import DenseNeRF
    from switch_nerf_amd.rendering import render_rays
    m, g = _mega("mega_sh_fg_d2", 1.15)
    bg, _ = _mega("mega_sh_bg", 1.15)
    r = _load("mega_sh_render")
    rays, img = _dev(r["rays"]), _dev(r["image_indices"])
    h = Namespace(coarse_samples=8, fine_samples=0, model_chunk_size=1000, sh_deg=2)
    with pytest.raises(NotImplementedError, match="inference only"):
        m.train()
    h.device_noise_seed = 3
    with pytest.raises(NotImplementedError, match="device noise"):
        render_rays(m, None, rays, img, h, None, None)
    h.device_noise_seed = None
    m.graph_eval = True
    with pytest.raises(NotImplementedError, match="graph capture"):
        render_rays(m, None, rays, img, h, None, None)
    m.graph_eval = False
    sub, sub_bg = m.sub_modules[0], bg.sub_modules[0]
    with pytest.raises(NotImplementedError, match="background"):          # a dense SH background model behind a dense SH foreground
        render_rays(sub, sub_bg, rays, img, h, r["sphere_center"], r["sphere_radius"])
    with pytest.raises(NotImplementedError, match="background"):          # ... and its forward_rays / training form
        sub_bg.forward_rays(rays, img, 8, 1000)
    with pytest.raises(NotImplementedError, match="not built"):
        BackgroundScene(sub, sub_bg, r["sphere_center"], r["sphere_radius"])
    with pytest.raises(NotImplementedError, match="a background model of another kind"):
        render_rays(m, sub_bg, rays, img, h, r["sphere_center"], r["sphere_radius"])
    with pytest.raises(NotImplementedError, match="NeRFMoE"):             # SwitchNeRF cannot carry the coefficients
        from switch_nerf_amd.model import SwitchNeRF
        SwitchNeRF(dict(synth.BUILDING, sh_deg=2), dtype=torch.float32)
