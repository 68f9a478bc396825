"""GPU: rendering.render_image / validate_image (Runner.render_image from a camera) at 37 x 29 with image_pixel_batch_size = 256 (five
batches, the last of 49 rays) on the smallest model configurations tests/synth.py offers: every returned key equals, bit for bit, a
hand-written loop that slices the whole image's rays and calls render_rays per batch with the reference's three flags; with
graph_eval the rays are generated into the captured graphs' static inputs and a second camera reuses the graphs."""
from argparse import Namespace

import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu

W, H, BATCH = 37, 29, 256
P = W * H
NEAR, FAR, ALT = 0.05, 1.5, [-0.3, 0.45]
MEGA_CFG = dict(layer_dim=256, layers=2, skip_layers=(1,), pos_xyz_dim=3, pos_dir_dim=2, appearance_dim=8, appearance_count=4, xyz_dim=3)


def _look(origin, forward):
    """c2w [3, 4] of a camera at origin looking along forward (x down; the camera looks along its -z)."""
    f = np.asarray(forward, np.float64)
    f = f / np.linalg.norm(f)
    r = np.cross(f, np.array([-1.0, 0.0, 0.0]))
    r = r / np.linalg.norm(r)
    return torch.from_numpy(np.concatenate([np.stack([r, np.cross(r, f), -f], 1), np.asarray(origin, np.float64)[:, None]], 1)).float()


def _camera(which=0, index=2):
    """0, 1: two cameras above both altitude planes; 2: one inside synth's foreground ellipsoid (the background scene's bound)."""
    from switch_nerf_amd.rays import Camera
    pose = (_look([-0.6, 0.02, 0.03], [1.0, 0.2, -0.3]), _look([-0.55, -0.05, 0.0], [1.0, -0.3, 0.25]),
            _look([-0.3, 0.02, 0.03], [1.0, 0.2, -0.3]))[which]
    return Camera(W, H, [40.0, 43.5, 17.25, 15.625], pose, index)


def _hparams(**kw):
    base = dict(coarse_samples=16, fine_samples=0, model_chunk_size=2048, perturb=1.0, use_sigma_noise=True, sigma_noise_std=1.0,
                image_pixel_batch_size=BATCH, appearance_dim=48, center_pixels=True)
    base.update(kw)
    return Namespace(**base)


def _switch(seed=11):
    from switch_nerf_amd.model import SwitchNeRF
    m = SwitchNeRF(synth.BUILDING, dtype=torch.float32)
    m.load_state_dict(synth.make_weights(seed, synth.BUILDING, gate_scale=0.02))
    m.eval()
    return m


def _dense(cfg=synth.DENSE, seed=12):
    from switch_nerf_amd.dense import DenseNeRF
    m = DenseNeRF(cfg, dtype=torch.float32)
    m.load_state_dict(synth.make_dense_weights(seed, cfg))
    m.eval()
    return m


def _mega():
    from switch_nerf_amd.mega import MegaNeRF
    sds = [synth.make_dense_weights(21 + i, MEGA_CFG) for i in range(2)]
    m = MegaNeRF.from_state_dicts(sds, np.array([[0.0, -0.3, 0.0], [0.0, 0.3, 0.0]], np.float32), MEGA_CFG, boundary_margin=1.15)
    m.eval()
    return m


def by_hand(nerf, bg_nerf, cam, hp, alt, center=None, radius=None):
    """What a user of render_rays writes: the whole image's rays, sliced per batch, results concatenated (0-dim values stacked)."""
    from switch_nerf_amd import rays
    from switch_nerf_amd.rendering import render_rays
    whole = rays.camera_rays(cam, NEAR, FAR, alt, hp.center_pixels)
    idx = torch.full((P,), cam.image_index, dtype=torch.long, device="cuda")
    out = {}
    step = hp.image_pixel_batch_size
    for b in range(0, P, step):
        res, _ = render_rays(nerf, bg_nerf, whole[b:b + step].contiguous(), idx[b:b + step].contiguous() if hp.appearance_dim > 0 else None,
                             hp, center, radius, True, False, True)
        for k, v in res.items():
            out.setdefault(k, []).append(v.clone())
    return {k: torch.stack(v) if v[0].dim() == 0 else torch.cat(v) for k, v in out.items()}, whole


def same(got, want):
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k in want:
        assert got[k].is_cuda and got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert torch.equal(got[k], want[k]), k


def check_model(nerf, bg_nerf, hp, alt, typ, center=None, radius=None, extra=(), cam=None):
    from switch_nerf_amd.rendering import render_image
    cam = _camera() if cam is None else cam
    want, whole = by_hand(nerf, bg_nerf, cam, hp, alt, center, radius)
    got, rays = render_image(nerf, bg_nerf, cam, hp, NEAR, FAR, alt, center, radius)
    same(got, want)
    assert rays.shape == (P, 8) and torch.equal(rays, whole)
    assert got[f"rgb_{typ}"].shape == (P, 3) and got[f"depth_{typ}"].shape == (P,) and f"depth_variance_{typ}" not in got
    assert torch.isfinite(got[f"rgb_{typ}"]).all()
    for k in extra:
        assert k in got, k
    return got


def test_render_image_switch_nerf_hierarchical():
    got = check_model(_switch(), None, _hparams(fine_samples=8), ALT, "fine")
    assert all(v.dim() == 1 for k, v in got.items() if k.startswith("gate_loss"))


def test_render_image_dense_nerf_without_appearance_indices():
    """hparams.appearance_dim == 0 hands render_rays no image indices (it then uses index 0), as the reference's loop does."""
    m = _dense()
    check_model(m, None, _hparams(), ALT, "coarse")
    check_model(m, None, _hparams(appearance_dim=0, image_pixel_batch_size=BATCH), None, "coarse")


def test_render_image_foreground_background_pair():
    got = check_model(_switch(), _dense(synth.DENSE_BG, 13), _hparams(), None, "coarse", synth.SPHERE_CENTER, synth.SPHERE_RADIUS,
                      extra=("fg_rgb_coarse", "bg_rgb_coarse", "fg_depth_coarse", "bg_depth_coarse"), cam=_camera(2))
    assert (got["bg_rgb_coarse"].abs().sum(-1) > 0).any()                     # some rays leave the bound


def test_render_image_two_cell_mega_nerf():
    check_model(_mega(), None, _hparams(appearance_dim=8, model_chunk_size=1000), ALT, "coarse")


@pytest.mark.parametrize("batch", [5000, 1000])
def test_render_image_batch_sizes(batch):
    """A batch larger than the image (one call, no padding), and one that leaves a tail of 73."""
    check_model(_dense(), None, _hparams(image_pixel_batch_size=batch), ALT, "coarse")


def test_render_image_graph_eval_writes_into_the_static_rays():
    from switch_nerf_amd import rays
    from switch_nerf_amd.rendering import render_image
    hp = _hparams(fine_samples=8)
    ma, mb = _switch(), _switch()
    ma.graph_eval = mb.graph_eval = True
    cam = _camera()
    want, whole = by_hand(ma, None, cam, hp, ALT)                              # the hand-written loop, itself with graph_eval
    got, r = render_image(mb, None, cam, hp, NEAR, FAR, ALT)
    same(got, want)
    assert torch.equal(r, whole)
    graphs = dict(mb._render_graphs)
    assert len(graphs) == 2 and sorted(k[0] for k in graphs) == [49, BATCH]        # the last batch has its own graph
    # the static inputs hold the last batch each graph ran: generated in place, never copied in
    for key, g in graphs.items():
        begin = 1024 if key[0] == 49 else 768
        assert torch.equal(g.rays, whole[begin:begin + key[0]]) and (g.idx == cam.image_index).all()
    # a second image from another camera of the same size: no new capture
    cam2 = _camera(1, index=5)
    got2, r2 = render_image(mb, None, cam2, hp, NEAR, FAR, ALT)
    assert len(mb._render_graphs) == 2 and all(mb._render_graphs[k] is g for k, g in graphs.items())
    want2, _ = by_hand(ma, None, cam2, hp, ALT)
    same(got2, want2)
    assert torch.equal(r2, rays.camera_rays(cam2, NEAR, FAR, ALT, True)) and not torch.equal(got2["rgb_fine"], got["rgb_fine"])


def test_validate_image_scores_the_picture_where_it_lies():
    from switch_nerf_amd import metrics
    from switch_nerf_amd.rendering import render_image, validate_image
    m, cam, hp = _dense(), _camera(), _hparams()
    rng = np.random.default_rng(5)
    target = torch.from_numpy(rng.uniform(0, 1, (H, W, 3)).astype(np.float32)).cuda()
    mask = torch.from_numpy(rng.uniform(0, 1, (H, W)) > 0.4).cuda()
    res, _ = render_image(m, None, cam, hp, NEAR, FAR, ALT)
    want = metrics.image_metrics(res["rgb_coarse"].view(H, W, 3), target, valid_mask=mask)
    got, image = validate_image(m, None, cam, target, hp, NEAR, FAR, ALT, valid_mask=mask)
    assert image.shape == (H, W, 3) and image.is_cuda and torch.equal(image, res["rgb_coarse"].view(H, W, 3))
    assert set(got) == set(want) == {"psnr", "ssim", "mse", "psnr_mask", "ssim_mask"}
    for k in want:
        assert got[k].is_cuda and torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), k
    plain, _ = validate_image(m, None, cam, target, hp, NEAR, FAR, ALT)
    assert set(plain) == {"psnr", "ssim", "mse"} and torch.equal(plain["psnr"], got["psnr"])
