"""CPU-only: the host-side checks of the row-addressed noise entry points (swn_rng_fill_rows, swn_bg_sample_pe_rng: nothing is launched)
and the row-addressing restatement (tests/philox_rows_restate.py) against tests/philox_restate.py."""
import ctypes as C

import numpy as np

import philox_restate as R
import philox_rows_restate as RR

SEED = 0x0123456789ABCDEF
I64_MAX = (1 << 63) - 1


def test_fill_rows_validates_before_launch():
    from switch_nerf_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(0x1000)
    err = lambda: lib.swn_last_error().decode()
    # (out, n_rows, per_row, row_base, row_index, index_limit, kind, scale, seed, step_dev, stream_id, domain, stream)
    f = lib.swn_rng_fill_rows
    assert f(p, 4, 8, 0, p, 16, 2, 1.0, 1, p, 0, 0, None) != 0 and "kind" in err()
    assert f(p, 4, 8, 0, p, 16, 0, 1.0, 1, p, 6, 0, None) != 0 and "stream id" in err()
    assert f(p, 4, 8, 0, p, 16, 0, 1.0, 1, p, 0, 2, None) != 0 and "domain" in err()
    assert f(p, 4, 8, 0, p, 16, 0, 1.0, 1, None, 0, 0, None) != 0 and "step_dev" in err()
    assert f(None, 4, 8, 0, p, 16, 0, 1.0, 1, p, 0, 0, None) != 0 and "out" in err()
    assert f(p, 4, 8, -1, p, 16, 0, 1.0, 1, p, 0, 0, None) != 0 and "row_base" in err()
    assert f(p, -1, 8, 0, p, 16, 0, 1.0, 1, p, 0, 0, None) != 0 and "n_rows" in err()
    assert f(p, 4, -1, 0, p, 16, 0, 1.0, 1, p, 0, 0, None) != 0 and "per_row" in err()
    # (row_base + index_limit) * per_row must fit int64: with and without a row index (NULL: the limit is at least n_rows)
    assert f(p, 4, 8, I64_MAX // 8 - 15, p, 16, 0, 1.0, 1, p, 0, 0, None) != 0 and "per_row" in err()
    assert f(p, 4, 8, I64_MAX // 8 - 3, None, 0, 0, 1.0, 1, p, 0, 0, None) != 0 and "per_row" in err()
    assert f(p, 4, 1 << 62, 0, p, 16, 0, 1.0, 1, p, 0, 0, None) != 0 and "per_row" in err()
    assert f(p, 4, 8, I64_MAX - 3, p, 16, 0, 1.0, 1, p, 0, 0, None) != 0 and "row_base" in err()
    assert f(None, 0, 8, 0, None, 0, 0, 1.0, 1, None, 0, 0, None) == 0                # no rows: nothing launched


def test_bg_sample_pe_rng_validates_before_launch():
    from switch_nerf_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(0x1000)
    err = lambda: lib.swn_last_error().decode()
    # (rays, center, radius, t_steps, seed, step_dev, ray_base, row_index, index_limit, perturb, n_rays, n_samples, l_xyz, dtype, z_out,
    #  depth_real, pe, pe_stride, stream)
    f = lib.swn_bg_sample_pe_rng
    assert f(p, None, None, p, 1, None, 0, p, 16, 1.0, 4, 8, 12, _lib.F32, p, p, p, 128, None) != 0 and "step_dev" in err()
    assert f(p, None, None, p, 1, p, -1, p, 16, 1.0, 4, 8, 12, _lib.F32, p, p, p, 128, None) != 0 and "ray_base" in err()
    assert f(p, None, None, p, 1, p, I64_MAX // 8 - 15, p, 16, 1.0, 4, 8, 12, _lib.F32, p, p, p, 128, None) != 0 and "n_samples" in err()
    assert f(p, None, None, p, 1, p, 0, p, 16, 1.0, 4, 0, 12, _lib.F32, p, p, p, 128, None) != 0 and "n_samples" in err()
    assert f(p, None, None, p, 1, p, 0, p, 16, 1.0, 4, 8, 12, 7, p, p, p, 128, None) != 0 and "dtype" in err()
    assert f(p, None, None, p, 1, p, 0, p, 16, 1.0, 4, 8, 12, _lib.F32, p, p, None, 128, None) != 0 and "null pointer" in err()
    assert f(p, None, None, p, 1, p, 0, None, 0, 1.0, 0, 8, 12, _lib.F32, p, p, p, 128, None) == 0     # no rays: nothing launched


def test_constants_and_abi():
    from switch_nerf_amd import _lib, ops
    assert (ops.RNG_DOMAIN_FG, ops.RNG_DOMAIN_BG) == (0, 1)
    assert "swn_rng_fill_rows" in _lib.SIGNATURES and "swn_bg_sample_pe_rng" in _lib.SIGNATURES
    assert callable(ops.rng_fill_rows) and callable(ops.bg_sample_pe_rng)


def test_row_restatement_identity_equals_the_contiguous_run():
    """Identity index: the rows are consecutive runs, so the whole equals philox_restate over [row_base * per_row, + n_rows * per_row)."""
    for per_row in (1, 7, 13, 16):
        for row_base in (0, 5, (1 << 33) - 3):
            rows = RR.uniform_rows(SEED, 3, 2, 0, row_base, None, per_row, n_rows=9)
            assert np.array_equal(rows.reshape(-1), R.uniform(SEED, 3, 2, row_base * per_row, 9 * per_row))
            nrm = RR.normal_rows(SEED, 3, 1, 0, row_base, None, per_row, n_rows=9, scale=0.5)
            assert np.array_equal(nrm.reshape(-1), R.normal(SEED, 3, 1, row_base * per_row, 9 * per_row, scale=0.5))


def test_row_restatement_index_and_domain():
    idx = [4, 0, 4, 199, 17]
    rows = RR.uniform_rows(SEED, 0, 0, 1, 5, idx, 7)
    for j, i in enumerate(idx):                                # row j = element run of global row 5 + i, domain in bits 8.. of word 3
        for s in range(7):
            e = (5 + i) * 7 + s
            w = R.philox4x32_10(((e >> 2) & R.MASK, (e >> 2) >> 32, 0, 0 | (1 << 8)), (SEED & R.MASK, SEED >> 32))[e & 3]
            assert rows[j, s] == np.float32((w >> 8) * 2.0 ** -24)
    assert np.array_equal(rows[0], rows[2])
    assert not np.array_equal(rows, RR.uniform_rows(SEED, 0, 0, 0, 5, idx, 7))
    assert RR.counter_word(3, 1) == 0x103 and RR.counter_word(3, 0) == 3
