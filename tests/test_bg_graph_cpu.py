"""CPU-only parts of the padded background step: the checks behind the one readback of (n_bg, n_out), the padding ray, the bindings."""
import numpy as np
import pytest
import torch

import synth


def _scene():
    from switch_nerf_amd.background import BackgroundScene
    return BackgroundScene.__new__(BackgroundScene)        # read_counts uses no state of the scene


def _ctx(n_bg, n_out, C=8, N=32):
    return dict(C=C, N=N, Nb=None, counts_dev=torch.tensor([n_bg, n_out], dtype=torch.int32))


def test_read_counts_fills_the_context_and_checks_it():
    scene = _scene()
    ctx = _ctx(5, 0)
    scene.read_counts(ctx)
    assert ctx["Nb"] == 5 and ctx["n_out"] == 0
    ctx = _ctx(8, 0)
    scene.read_counts(ctx)                                  # n_bg == C fits
    with pytest.raises(RuntimeError, match=r"n_bg = 9 .* bg_capacity = 8"):
        scene.read_counts(_ctx(9, 0))
    with pytest.raises(Exception, match="bounded by the unit sphere"):
        scene.read_counts(_ctx(3, 2))
    compact = dict(Nb=4)                                    # a compact context: nothing to read, nothing to check
    scene.read_counts(compact)
    assert compact == dict(Nb=4)


def test_padding_ray_layout():
    from switch_nerf_amd import ops
    c, r = synth.SPHERE_CENTER, synth.SPHERE_RADIUS
    pad = np.array(list(ops.bg_pad_ray(c, r)), np.float32)
    np.testing.assert_array_equal(pad, np.array([c[0], c[1], c[2], 0, 0, 1, 0, 2 * r[2]], np.float32))
    np.testing.assert_array_equal(np.array(list(ops.bg_pad_ray(None, None)), np.float32), np.array([0, 0, 0, 0, 0, 1, 0, 2], np.float32))
    np.testing.assert_array_equal(np.array(list(ops.bg_pad_ray(torch.from_numpy(c), torch.from_numpy(r))), np.float32), pad)


def test_bindings_and_interfaces_exist():
    import inspect
    from switch_nerf_amd import _lib, graph
    from switch_nerf_amd.background import BackgroundScene
    for name in ("swn_bg_compact", "swn_bg_blend_fwd", "swn_bg_blend_bwd"):
        assert name in _lib.SIGNATURES
    for fn in (BackgroundScene.forward, BackgroundScene.train_step, BackgroundScene.grad_step):
        assert inspect.signature(fn).parameters["bg_capacity"].default is None
    p = inspect.signature(graph.GraphedBackgroundStep.__init__).parameters
    assert [k for k in p][1:] == ["scene", "rgbs", "rays", "image_indices", "n_samples", "seg_tokens", "perturb", "noise_std", "bg_capacity",
                                  "warmup"]
    assert (p["perturb"].default, p["noise_std"].default, p["bg_capacity"].default, p["warmup"].default) == (1.0, 1.0, None, 2)
