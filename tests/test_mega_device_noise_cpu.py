"""CPU-only: the host side of the seeded device noise of Mega-NeRF joint training - the ABI of swn_cells_gather_rng /
swn_cells_gather_padded_rng (csrc/cells.hip), their checks (each fires before anything is launched), and the switch on
switch_nerf_amd.mega.MegaNeRF.  Nothing here touches a device."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import synth

CFG = dict(layer_dim=256, layers=2, skip_layers=(1,), pos_xyz_dim=3, pos_dir_dim=2, appearance_dim=8, appearance_count=4, xyz_dim=3)
CEN = np.array([[-0.5, -0.4, 0.1], [0.5, -0.3, -0.2], [0.0, 0.5, 0.3]], np.float32)
I64_MAX = (1 << 63) - 1


def _subs(cfg=CFG, dtype=torch.float32):
    from switch_nerf_amd.dense import DenseNeRF
    subs = []
    for i in range(3):
        m = DenseNeRF(cfg, dtype=dtype, device="cpu")
        if cfg.get("sh_deg") is None:
            m.load_state_dict(synth.make_dense_weights(501 + i, cfg))
        subs.append(m)
    return subs


def test_signatures_and_exports():
    from switch_nerf_amd import _lib, ops
    lib = _lib.load()
    for name in ("swn_cells_gather_rng", "swn_cells_gather_padded_rng"):
        assert name in _lib.SIGNATURES
        assert callable(getattr(lib, name))
    # the plain entry's arguments with (seed, step_dev, stream_id, rows_per_ray, ray_base, scale) in place of the noise tensor
    assert len(_lib.SIGNATURES["swn_cells_gather_rng"]) == len(_lib.SIGNATURES["swn_cells_gather"]) + 5
    assert len(_lib.SIGNATURES["swn_cells_gather_padded_rng"]) == len(_lib.SIGNATURES["swn_cells_gather_padded"]) + 5
    assert callable(ops.cells_gather_rng) and callable(ops.cells_gather_padded_rng)
    assert (ops.RNG_SIGMA, ops.RNG_SIGMA_FINE) == (1, 3)


def test_gather_rng_validates_before_launch():
    from switch_nerf_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(0x1000)
    err = lambda: lib.swn_last_error().decode()
    # (x, stride, col0, rows, total, n_points, seed, step_dev, stream_id, rows_per_ray, ray_base, scale, x_out, noise_out, stream)
    f = lib.swn_cells_gather_rng
    for null in (0, 3, 7, 12, 13):
        a = [p, 7, 0, p, 16, 35, 1, p, 1, 5, 3, 1.0, p, p, None]
        a[null] = None
        assert f(*a) != 0 and "null pointer" in err(), null
    assert f(p, 7, 0, p, 16, 35, 1, p, 1, 5, 3, 0.0, p, p, None) != 0 and "scale" in err()
    assert f(p, 7, 0, p, 16, 35, 1, p, 1, 5, 3, -1.0, p, p, None) != 0 and "scale" in err()
    for stream_id in (0, 2, 4, 5, 6, -1):
        assert f(p, 7, 0, p, 16, 35, 1, p, stream_id, 5, 3, 1.0, p, p, None) != 0 and "stream id" in err(), stream_id
    assert f(p, 7, 0, p, 16, 35, 1, p, 1, 0, 3, 1.0, p, p, None) != 0 and "rows_per_ray" in err()
    assert f(p, 7, 0, p, 16, 35, 1, p, 3, -5, 3, 1.0, p, p, None) != 0 and "rows_per_ray" in err()
    assert f(p, 7, 0, p, 16, 35, 1, p, 1, 5, -1, 1.0, p, p, None) != 0 and "ray_base" in err()
    assert f(p, 7, 0, p, 16, 35, 1, p, 1, 5, I64_MAX // 5, 1.0, p, p, None) != 0 and "ray_base" in err()
    assert f(p, 7, 7, p, 16, 35, 1, p, 1, 5, 3, 1.0, p, p, None) != 0 and "bad sizes" in err()
    assert f(p, 7, 0, p, 0, 35, 1, p, 3, 5, 3, 1.0, p, p, None) == 0                  # no rows: nothing launched


def test_gather_padded_rng_validates_before_launch():
    from switch_nerf_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(0x1000)
    err = lambda: lib.swn_last_error().decode()
    # (x, stride, col0, rows, centroids, n_cells, capacity, n_points, seed, step_dev, stream_id, rows_per_ray, ray_base, scale, x_out,
    #  noise_out, stream)
    f = lib.swn_cells_gather_padded_rng
    for null in (0, 3, 4, 9, 14, 15):
        a = [p, 7, 0, p, p, 3, 16, 35, 1, p, 1, 5, 3, 1.0, p, p, None]
        a[null] = None
        assert f(*a) != 0 and "null pointer" in err(), null
    assert f(p, 7, 0, p, p, 3, 16, 35, 1, p, 1, 5, 3, 0.0, p, p, None) != 0 and "scale" in err()
    for stream_id in (0, 2, 4, 6):
        assert f(p, 7, 0, p, p, 3, 16, 35, 1, p, stream_id, 5, 3, 1.0, p, p, None) != 0 and "stream id" in err(), stream_id
    assert f(p, 7, 0, p, p, 3, 16, 35, 1, p, 3, 0, 3, 1.0, p, p, None) != 0 and "rows_per_ray" in err()
    assert f(p, 7, 0, p, p, 3, 16, 35, 1, p, 3, 5, -2, 1.0, p, p, None) != 0 and "ray_base" in err()
    assert f(p, 7, 0, p, p, 65, 16, 35, 1, p, 3, 5, 3, 1.0, p, p, None) != 0 and "n_cells" in err()
    assert f(p, 8, 0, p, p, 3, 16, 35, 1, p, 3, 5, 3, 1.0, p, p, None) != 0 and "7" in err()
    assert f(p, 7, 0, p, p, 64, 1 << 26, 35, 1, p, 3, 5, 3, 1.0, p, p, None) != 0 and "32-bit row space" in err()


def test_the_switch_on_the_model():
    from switch_nerf_amd.mega import MegaNeRF
    from switch_nerf_amd.noise import DeviceNoise
    for f in (MegaNeRF.grad_step, MegaNeRF.train_step):
        assert inspect.signature(f).parameters["sigma_noise_std"].default == 0.0
    assert inspect.signature(MegaNeRF.forward_points).parameters["sigma_rng"].default is None
    m = MegaNeRF(_subs(), CEN, 1.15, False, False, joint_training=True)
    assert isinstance(m.noise, DeviceNoise) and not m.device_noise
    assert m.noise_state_dict() == {"seed": None, "step": 0, "ray_base": 0}
    # these models are host-resident (device "cpu": parameters only, no kernel runs on them): the switch needs a GPU model, where
    # tests/test_mega_device_noise_gpu.py turns it on; off is always taken
    with pytest.raises(NotImplementedError, match="device noise needs the model on a GPU"):
        m.set_device_noise(7, step=5, ray_base=64)
    with pytest.raises(NotImplementedError, match="device noise needs the model on a GPU"):
        m.load_noise_state_dict({"seed": 9, "step": 2, "ray_base": 3})
    m.set_device_noise(None)
    m.load_noise_state_dict({"seed": None})
    assert not m.device_noise
    # the delegation, on the state object itself (the class is device-agnostic; only the kernels need the counter on the device)
    m.noise.set(7, 5, 64, "cpu")
    assert m.device_noise and m.noise_state_dict() == {"seed": 7, "step": 5, "ray_base": 64}
    assert not any(s.device_noise for s in m.sub_modules)                    # the cells' own stay off
    m.set_ray_base(128)
    assert m.noise_state_dict() == {"seed": 7, "step": 5, "ray_base": 128}
    with pytest.raises(ValueError, match="device noise"):
        m.set_ray_base(-1)
    m.set_device_noise(None)
    assert not m.device_noise and m.noise_state_dict()["seed"] is None
    # a tensor and a draw request exclude each other; a request needs the noise on
    x = torch.zeros(4, 7)
    with pytest.raises(ValueError, match="device noise, which is off"):
        m.forward_points(x, sigma_rng=(1, 2, 1.0))
    m.noise.set(7, 0, 0, "cpu")
    with pytest.raises(ValueError, match="exclude each other"):
        m.forward_points(x, torch.zeros(4), sigma_rng=(1, 2, 1.0))


def test_what_stays_refused():
    from argparse import Namespace
    from switch_nerf_amd import graph, mega
    from switch_nerf_amd.mega import MegaNeRF
    # the inference-only model: evaluation draws nothing
    inf = MegaNeRF(_subs(), CEN, 1.15, False, False)
    with pytest.raises(NotImplementedError, match="device noise.*joint_training=True"):
        inf.set_device_noise(7)
    inf.set_device_noise(None)
    for call in (inf.noise_state_dict, lambda: inf.set_ray_base(3), lambda: inf.load_noise_state_dict({"seed": 1})):
        with pytest.raises(NotImplementedError, match="inference only"):
            call()
    h = Namespace(coarse_samples=2, fine_samples=0, model_chunk_size=8, device_noise_seed=3)
    with pytest.raises(NotImplementedError, match="device_noise_seed.*evaluation.*MegaNeRF.set_device_noise"):
        mega.render_rays(inf, None, torch.zeros(4, 8), torch.zeros(4, dtype=torch.long), h)
    # a cell with its own noise on: refused, and the message names the model's switch
    subs = _subs()
    subs[1].set_device_noise(3)
    with pytest.raises(NotImplementedError, match="device noise.*MegaNeRF.set_device_noise"):
        MegaNeRF(subs, CEN, 1.0, False, False, joint_training=True)
    with pytest.raises(NotImplementedError, match="fp16"):
        MegaNeRF(_subs(dtype=torch.float16), CEN, 1.0, False, False, joint_training=True)
    with pytest.raises(NotImplementedError, match="xyz_real"):
        MegaNeRF(_subs(dict(CFG, xyz_dim=4)), CEN, 1.0, True, False, joint_training=True)
    # with the noise on, the rest of what joint training refuses stays refused - and never moves the step counter
    m = MegaNeRF(_subs(), CEN, 1.15, False, False, joint_training=True)
    m.noise.set(7, 4, 0, "cpu")           # (host-resident models: the state object directly)
    with pytest.raises(NotImplementedError, match="accumulation"):
        m.set_accumulation(2)
    with pytest.raises(NotImplementedError, match="finite guard"):
        m.set_check_finite(True)
    with pytest.raises(NotImplementedError, match="data parallelism"):
        m.apply_step(lambda flat: 1.0, True, dict(cell_overflow=None))
    sh = MegaNeRF(_subs(dict(CFG, pos_dir_dim=0, sh_deg=1)), CEN, 1.0, False, False, joint_training=True, sh_training=True)
    sh.noise.set(7, 4, 0, "cpu")
    rays, img = torch.zeros(4, 8), torch.zeros(4, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="cell_capacity.*spherical-harmonics"):
        sh.train_step(torch.zeros(4, 3), rays, img, 2, cell_capacity=(8, 4), sigma_noise_std=1.0)
    with pytest.raises(NotImplementedError, match="cell_capacity.*spherical-harmonics"):
        graph.GraphedMegaStep(sh, torch.zeros(4, 3), rays, img, 2, 8)
    assert m.noise_state_dict()["step"] == 4 and sh.noise_state_dict()["step"] == 4


def test_documents_name_the_feature():
    from switch_nerf_amd import graph, mega
    doc = " ".join(mega.__doc__.split())
    assert "MegaNeRF.set_device_noise" in doc and "cells_gather_rng" in doc
    assert "set_device_noise" in " ".join(graph.GraphedMegaStep.__doc__.split())
