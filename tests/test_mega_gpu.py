"""The Mega-NeRF spatial-cell model on the HIP path (switch_nerf_amd/mega.py: cell router + three two-layer DenseNeRF sub-models of layer_dim 256,
the smallest width the dense NeRF's head kernels run) against
the reference's own MegaNeRF (tests/golden/mega_*.npz, scripts/gen_golden_mega.py), at the tolerances of the dense-NeRF golden test
(tests/test_dense_gpu.py: rgb 1e-4 absolute, sigma 1e-4 relative + absolute) and of the render mirrors (tests/test_model_gpu.py).
Points on a membership decision (excluded_*: none in the committed fixtures) may legitimately fall on either side and are left out."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _mega(g, margin, dtype=torch.float32):
    from switch_nerf_amd.mega import MegaNeRF
    cfg = {k[5:]: (tuple(int(v) for v in g[k]) if g[k].ndim else int(g[k])) for k in g.files if k.startswith("cfg__")}
    K = len(g["centroids"])
    sds = [synth.make_dense_weights(int(g["seed"]) + i, cfg) for i in range(K)]      # (the fixture stores the seed and a checksum)
    for sd, ref in zip(sds, g["sd_checksums"]):
        np.testing.assert_allclose(np.sum([synth.checksum(v) for v in sd.values()], 0), ref, rtol=1e-12)
    return MegaNeRF.from_state_dicts(sds, g["centroids"], cfg, boundary_margin=margin, xyz_real=bool(g["xyz_real"]),
                                     cluster_2d=bool(g["cluster_2d"]), dtype=dtype)


@pytest.mark.parametrize("name,tag,margin", [("mega_fg", "m100", 1.0), ("mega_fg", "m115", 1.15), ("mega_bg", "m115", 1.15)])
def test_mega_forward_vs_reference_golden_fp32(name, tag, margin):
    g = np.load(os.path.join(G, name + ".npz"))
    m = _mega(g, margin)
    keep = ~g["excluded_" + tag]
    assert keep.mean() >= 0.99
    x, noise = _dev(g["x"]), _dev(g["sigma_noise"])
    out = m(x, sigma_noise=noise).cpu().numpy()
    ref = g["out_" + tag]
    assert out.shape == ref.shape
    print(f"{name} {tag}: rgb err {np.abs(out - ref)[keep, :3].max():.3e}, sigma err {np.abs(out - ref)[keep, 3].max():.3e}")
    np.testing.assert_allclose(out[keep, :3], ref[keep, :3], rtol=0, atol=1e-4)
    np.testing.assert_allclose(out[keep, 3], ref[keep, 3], rtol=1e-4, atol=1e-4)
    n_pos = 7 if bool(g["xyz_real"]) else 3
    sig = m(x[:, :n_pos].contiguous(), sigma_only=True, sigma_noise=noise).cpu().numpy()
    assert sig.shape == g["sigma_" + tag].shape == (len(ref), 1)
    np.testing.assert_allclose(sig[keep], g["sigma_" + tag][keep], rtol=1e-4, atol=1e-4)
    # the router's own outputs are the reference's membership
    w, counts, begin, rows, slot = m.route(x)
    np.testing.assert_array_equal((w.cpu().numpy() > 0)[keep], (g["weights_" + tag] > 0)[keep])
    with pytest.raises(Exception, match="Unexpected input shape"):
        m(x[:, :5].contiguous())


def _hparams(g, fine):
    return Namespace(coarse_samples=int(g["S"]), fine_samples=fine, model_chunk_size=1000, perturb=1.0, use_sigma_noise=True,
                     sigma_noise_std=1.0)


def test_mega_render_rays_vs_reference_golden():
    """rendering.render_rays with a MegaNeRF foreground: 64 rays x 32 samples, a ragged last model chunk; then with 32 fine samples."""
    from switch_nerf_amd.rendering import render_rays
    g = np.load(os.path.join(G, "mega_render.npz"))
    m = _mega(np.load(os.path.join(G, "mega_fg.npz")), float(g["margin"]))
    rays, img = _dev(g["rays"]), _dev(g["image_indices"])
    res, bg = render_rays(m, None, rays, img, _hparams(g, 0), None, None, True, True, False)
    assert bg is False and set(res) == {"rgb_coarse", "depth_coarse", "depth_variance_coarse"}
    np.testing.assert_allclose(res["rgb_coarse"].cpu().numpy(), g["rgb_coarse"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(res["depth_coarse"].cpu().numpy(), g["depth_coarse"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(res["depth_variance_coarse"].cpu().numpy(), g["depth_variance_coarse"], rtol=1e-3, atol=1e-6)
    res, _ = render_rays(m, None, rays, img, _hparams(g, int(g["F"])), None, None, True, True, False)
    assert set(res) == {"rgb_fine", "depth_fine", "depth_variance_fine"}
    np.testing.assert_allclose(res["rgb_fine"].cpu().numpy(), g["rgb_fine"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(res["depth_fine"].cpu().numpy(), g["depth_fine"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(res["depth_variance_fine"].cpu().numpy(), g["depth_variance_fine"], rtol=1e-3, atol=1e-6)


@pytest.mark.parametrize("typ", ["coarse", "fine"])
def test_mega_render_rays_with_background_vs_reference_golden(typ):
    """rendering.render_rays with both MegaNeRFs of a container (the reference's render_rays with hparams.container_path set): 64 rays
    of which 39 leave the ellipsoidal bound.  coarse: the ray's exit from the bound in front of the background points; fine: cluster_2d,
    the samples' own real positions, 32 + 16 fine samples.  Tolerances of tests/test_background_gpu.py's render mirror."""
    from switch_nerf_amd.mega import MegaNeRF
    from switch_nerf_amd.rendering import render_rays
    g = np.load(os.path.join(G, "mega_render_bg.npz"))
    models = []
    for name, seed, xyz_real in (("mega_fg", int(g["seed"]), False), ("mega_bg", int(g["seed_bg"]), True)):
        f = np.load(os.path.join(G, name + ".npz"))
        assert int(f["seed"]) == seed
        m = _mega(f, float(g["margin"]))
        models.append(MegaNeRF(m.sub_modules, g["centroids"], float(g["margin"]), xyz_real, bool(g["cluster_2d_" + typ])))
    rays, img = _dev(g["rays"]), _dev(g["image_indices"])
    res, present = render_rays(models[0], models[1], rays, img, _hparams(g, int(g["F"]) if typ == "fine" else 0), g["sphere_center"],
                               g["sphere_radius"], True, True, True)
    assert present is True
    assert set(res) == {k + "_" + typ for k in ("rgb", "depth", "depth_variance", "fg_rgb", "bg_rgb", "fg_depth", "bg_depth")}
    r = {k: v.cpu().numpy() for k, v in res.items()}
    for k in ("rgb", "fg_rgb", "bg_rgb"):
        print(f"{typ} {k}: err {np.abs(r[k + '_' + typ] - g[k + '_' + typ]).max():.3e}")
    np.testing.assert_allclose(r["fg_rgb_" + typ], g["fg_rgb_" + typ], rtol=0, atol=1e-4)
    np.testing.assert_allclose(r["bg_rgb_" + typ], g["bg_rgb_" + typ], rtol=0, atol=1e-4)
    np.testing.assert_allclose(r["rgb_" + typ], g["rgb_" + typ], rtol=0, atol=1e-4)
    np.testing.assert_allclose(r["depth_" + typ], g["depth_" + typ], rtol=2e-3, atol=1e-4)
    np.testing.assert_allclose(r["depth_variance_" + typ], g["depth_variance_" + typ], rtol=2e-3, atol=1e-6)


def test_mega_render_rays_rejects_what_is_left_out():
    from switch_nerf_amd.rendering import render_rays
    g = np.load(os.path.join(G, "mega_render.npz"))
    fg = np.load(os.path.join(G, "mega_fg.npz"))
    m = _mega(fg, 1.15)
    rays, img = _dev(g["rays"]), _dev(g["image_indices"])
    h = _hparams(g, 0)
    with pytest.raises(NotImplementedError, match="background"):      # (a background model that is not the xyz_real MegaNeRF)
        render_rays(m, m, rays, img, h, None, None, True, True, False)
    h.device_noise_seed = 3
    with pytest.raises(NotImplementedError, match="device noise"):
        render_rays(m, None, rays, img, h, None, None, True, True, False)


def test_mega_bf16_close_to_fp32():
    g = np.load(os.path.join(G, "mega_fg.npz"))
    x = _dev(g["x"])
    a = _mega(g, 1.15)(x).cpu().numpy()
    b = _mega(g, 1.15, torch.bfloat16)(x).cpu().numpy()
    assert np.isfinite(b).all()
    print(f"bf16 vs fp32: rgb {np.abs(a - b)[:, :3].max():.3e}, sigma {np.abs(a - b)[:, 3].max():.3e}")
    assert np.abs(a - b)[:, :3].max() < 3e-2           # the bar of tests/test_dense_gpu.py::test_dense_bf16_close_to_fp32
    # the density is not confined to [0, 1] like the colours: the same bar relative to its range in the fp32 run, the way that test
    # bounds its unbounded quantities (the loss against its own size, a gradient against its largest entry)
    assert np.abs(a - b)[:, 3].max() < 3e-2 * np.abs(a[:, 3]).max()
