"""CPU-only: the restatement of the seeded noise generator (tests/philox_restate.py) against the known answers of Philox4x32-10 and
the element addressing of csrc/philox.hpp; the host-side checks of the new entry points (no launch)."""
import ctypes as C

import numpy as np
import pytest

import philox_restate as R


def test_known_answers():
    for counter, key, out in R.KNOWN_ANSWERS:
        assert R.philox4x32_10(counter, key) == out, (counter, key)


def test_vectorised_restatement_equals_scalar():
    seed = 0x0123456789ABCDEF
    w = R.words(seed, 3, 4, 5, 23)
    assert [int(x) for x in w] == [R.element_word(seed, 3, 4, 5 + i) for i in range(23)]


@pytest.mark.parametrize("e", [0, 1, 2, 3, 4, 7, (1 << 34) - 1, 1 << 34, (1 << 34) + 5, (1 << 40) + 2])
def test_element_addressing(e):
    """Element e is word e & 3 of block e >> 2; the block index carries into the second counter word at e = 2^34."""
    seed, step, stream = 0xA4093822299F31D0, 7, 2
    block = e >> 2
    ctr = (block & 0xFFFFFFFF, block >> 32, step, stream)
    assert R.block_counter(block, step, stream) == ctr
    assert R.element_word(seed, step, stream, e) == R.philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))[e & 3]
    assert int(R.words(seed, step, stream, e, 1)[0]) == R.element_word(seed, step, stream, e)


def test_block_carry_changes_the_counter():
    """e = 2^34 - 1 and e = 2^34 live in blocks 2^32 - 1 and 2^32: counters {ffffffff, 0, ..} and {0, 1, ..}."""
    assert R.block_counter(((1 << 34) - 1) >> 2, 0, 0) == (0xFFFFFFFF, 0, 0, 0)
    assert R.block_counter((1 << 34) >> 2, 0, 0) == (0, 1, 0, 0)
    w = R.words(1, 0, 0, (1 << 34) - 6, 12)            # a run across the carry equals the per-element values
    assert [int(x) for x in w] == [R.element_word(1, 0, 0, (1 << 34) - 6 + i) for i in range(12)]


def test_uniform_and_normal_maps():
    seed = 0x0123456789ABCDEF
    u = R.uniform(seed, 0, 0, 3, 1027)
    assert u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 1.0
    n = R.normal(seed, 0, 1, 3, 1027)                   # odd base: the first element is the sin half of its pair
    full = R.normal(seed, 0, 1, 0, 1032)
    assert np.array_equal(n, full[3:1030]) and np.isfinite(n).all()
    assert np.array_equal(R.normal(seed, 0, 1, 0, 64, scale=0.5), 0.5 * R.normal(seed, 0, 1, 0, 64))


def test_moments_of_the_gpu_tests_seed():
    """The seed / step / stream tests/test_device_noise_gpu.py draws its 2^20 normals with passes the moment bounds in the float64
    restatement (the draw is deterministic: this is the check made before the seed was committed)."""
    x = R.normal(0x0123456789ABCDEF, 0, 1, 0, 1 << 20)
    assert np.isfinite(x).all()
    assert abs(x.mean()) < 0.005 and abs(x.var() - 1.0) < 0.007, (x.mean(), x.var())


def test_entry_points_validate_before_launch():
    from switch_nerf_amd import _lib, ops
    lib = _lib.load()
    p = C.c_void_p(0x1000)
    err = lambda: lib.swn_last_error().decode()
    assert lib.swn_rng_fill(p, 16, 0, 2, 1.0, 1, p, 0, None) != 0 and "kind" in err()
    assert lib.swn_rng_fill(p, 16, 0, 0, 1.0, 1, p, 9, None) != 0 and "stream id" in err()
    assert lib.swn_rng_fill(p, -1, 0, 0, 1.0, 1, p, 0, None) != 0 and ">= 0" in err()
    assert lib.swn_rng_fill(p, 16, 0, 0, 1.0, 1, None, 0, None) != 0 and "null pointer" in err()
    assert lib.swn_rng_fill(None, 0, 0, 0, 1.0, 1, None, 0, None) == 0                  # nothing to fill: nothing launched
    assert lib.swn_rng_advance(None, None) != 0 and "null pointer" in err()
    assert lib.swn_sample_pe_rng(p, p, 1, None, 0, 1.0, 4, 8, 12, 4, _lib.F32, p, p, 128, None, 0, None) != 0 and "null pointer" in err()
    assert lib.swn_sample_pe_rng(p, p, 1, p, -1, 1.0, 4, 8, 12, 4, _lib.F32, p, p, 128, None, 0, None) != 0 and "ray_base" in err()
    with pytest.raises(ValueError, match="2\\^32"):
        ops.rng_check_step(1 << 32)
    with pytest.raises(ValueError):
        ops.rng_check_step(-1)
    assert ops.rng_check_step((1 << 32) - 1) == (1 << 32) - 1
    assert (ops.RNG_JITTER, ops.RNG_SIGMA, ops.RNG_FINE_U, ops.RNG_SIGMA_FINE, ops.RNG_GATE) == (0, 1, 2, 3, 4)


def test_render_rays_switch_keeps_the_models_ray_base():
    """rendering._device_noise on SwitchNeRF's own noise-state methods (a CPU stand-in object): hparams.device_noise_seed without
    hparams.ray_base leaves the ray_base that parallel.shard_rays(..., model=) set - before or after the switch-on - alone; with
    hparams.ray_base it is honoured; a bg_nerf is refused."""
    import types
    import torch
    from switch_nerf_amd import parallel, rendering
    from switch_nerf_amd.model import SwitchNeRF
    from switch_nerf_amd.noise import DeviceNoise

    class Stub:
        dev = torch.device("cpu")

        def __init__(self):
            self.noise = DeviceNoise()
        set_device_noise, set_ray_base = SwitchNeRF.set_device_noise, SwitchNeRF.set_ray_base
        device_noise, noise_state_dict = SwitchNeRF.device_noise, SwitchNeRF.noise_state_dict

    hp = types.SimpleNamespace(device_noise_seed=9)
    m = Stub()
    assert parallel.shard_rays(1024, 3, 4, model=m) == (768, 1024)             # ahead of the switch-on
    assert rendering._device_noise(m, None, hp) and m.noise_state_dict() == dict(seed=9, step=0, ray_base=768)
    assert rendering._device_noise(m, None, hp) and m.noise_state_dict()["ray_base"] == 768
    parallel.shard_rays(1024, 1, 4, model=m)                                   # after it
    assert rendering._device_noise(m, None, hp) and m.noise_state_dict()["ray_base"] == 256
    assert rendering._device_noise(m, None, types.SimpleNamespace(device_noise_seed=9, ray_base=None)) and m.noise.base == 256
    assert rendering._device_noise(m, None, types.SimpleNamespace(device_noise_seed=9, ray_base=5)) and m.noise.base == 5
    assert rendering._device_noise(m, None, types.SimpleNamespace()) is True   # on, nothing in hparams: stays as it is
    assert m.noise.base == 5
    with pytest.raises(NotImplementedError, match="device_noise_seed"):
        rendering._device_noise(m, object(), hp)
    assert rendering._device_noise(Stub(), None, types.SimpleNamespace()) is False
