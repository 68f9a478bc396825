"""GPU: rendering.render_image_nerf / render_image_nerf_mip (Runner.render_image_nerf / render_image_nerf_mip from a camera) on the 7 x 4
fixture camera with image_pixel_batch_size = 10 (three batches, the last of 8 pixels) and the smallest dense and mip models of
tests/synth.py: every returned key equals, bit for bit, a hand-written loop that slices the whole image's rays (and radii) and calls
render_rays / render_rays_mip per batch with image_indices=None and the reference's flags."""
from argparse import Namespace

import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu

BATCH = 10
NEAR, FAR = 2.0, 6.0


@pytest.fixture(scope="module")
def scene(golden_dir):
    from switch_nerf_amd import nerf_rays as nr
    g = np.load(f"{golden_dir}/nerf_rays.npz")
    cam = nr.PinholeCamera(int(g["b7x4_W"]), int(g["b7x4_H"]), g["b7x4_K"], g["b7x4_c2w"])
    assert (cam.W, cam.H) == (7, 4) and cam.W * cam.H % BATCH != 0
    return cam, float(g["scene_scaling_factor"]), g["scene_origin"], float(g["b7x4_focal"])


def _hparams(**kw):
    base = dict(coarse_samples=16, fine_samples=0, model_chunk_size=2048, perturb=1.0, use_sigma_noise=True, sigma_noise_std=1.0,
                image_pixel_batch_size=BATCH, appearance_dim=48)
    base.update(kw)
    return Namespace(**base)


def _dense():
    from switch_nerf_amd.dense import DenseNeRF
    m = DenseNeRF(synth.DENSE, dtype=torch.float32)
    m.load_state_dict(synth.make_dense_weights(12, synth.DENSE))
    m.eval()
    return m


def _mip():
    from switch_nerf_amd.model import SwitchNeRF
    m = SwitchNeRF(synth.BUILDING, dtype=torch.float32)
    m.load_state_dict(synth.make_weights(11, synth.BUILDING, gate_scale=0.02))
    m.eval()
    return m


def by_hand(P, step, render):
    out = {}
    for b in range(0, P, step):
        res, _ = render(b, min(b + step, P))
        for k, v in res.items():
            out.setdefault(k, []).append(v.clone())
    return {k: torch.stack(v) if v[0].dim() == 0 else torch.cat(v) for k, v in out.items()}


def same(got, want):
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k in want:
        assert got[k].is_cuda and got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("mode", ["normalized", "ndc", "raw"])
def test_render_image_nerf_equals_render_rays_per_batch(scene, mode):
    from switch_nerf_amd import nerf_rays as nr
    from switch_nerf_amd.rendering import render_image_nerf, render_rays
    cam, _, _, focal = scene
    P = cam.W * cam.H
    m, hp = _dense(), _hparams()
    near, far = (0.0, 1.0) if mode == "ndc" else (NEAR, FAR)
    whole = nr.camera_rays(cam, mode, near, far, focal=focal)
    want = by_hand(P, BATCH, lambda b, e: render_rays(m, None, whole[b:e].contiguous(), None, hp, None, None, True, False, False))
    got = render_image_nerf(m, cam, hp, near, far, mode=mode, focal=focal)
    same(got, want)
    assert got["rgb_coarse"].shape == (P, 3) and got["depth_coarse"].shape == (P,) and "depth_variance_coarse" not in got
    assert torch.isfinite(got["rgb_coarse"]).all() and not any(k.startswith(("fg_", "bg_")) for k in got)


@pytest.mark.parametrize("ray_nearfar,fine", [("sphere", 8), ("flat", 0)])
def test_render_image_nerf_mip_equals_render_rays_mip_per_batch(scene, ray_nearfar, fine):
    from switch_nerf_amd import nerf_rays as nr
    from switch_nerf_amd.rendering import render_image_nerf_mip, render_rays_mip
    cam, scale, origin, _ = scene
    P = cam.W * cam.H
    m, hp = _mip(), _hparams(coarse_samples=17, fine_samples=fine + 1 if fine else 0, perturb=0.0)
    rays, radii = nr.bungee_rays(cam, scale, origin, ray_nearfar)
    want = by_hand(P, BATCH, lambda b, e: render_rays_mip(m, rays[b:e].contiguous(), radii[b:e].contiguous(), None, hp, True, False))
    got = render_image_nerf_mip(m, cam, hp, scale, origin, ray_nearfar)
    same(got, want)
    typ = "fine" if fine else "coarse"
    assert got[f"rgb_{typ}"].shape == (P, 3) and got[f"depth_{typ}"].shape == (P,) and f"depth_variance_{typ}" not in got
    assert torch.isfinite(got[f"rgb_{typ}"]).all()
    assert all(v.dim() == 1 for k, v in got.items() if k.startswith("gate_loss"))


def test_both_refuse_a_model_in_training_mode(scene):
    from switch_nerf_amd.rendering import render_image_nerf, render_image_nerf_mip
    cam, scale, origin, _ = scene
    d, m = _dense(), _mip()
    d.train()
    m.train()
    with pytest.raises(RuntimeError, match="render_image_nerf: nerf is in training mode"):
        render_image_nerf(d, cam, _hparams(), NEAR, FAR)
    with pytest.raises(RuntimeError, match="render_image_nerf_mip: nerf is in training mode"):
        render_image_nerf_mip(m, cam, _hparams(), scale, origin, "sphere")
