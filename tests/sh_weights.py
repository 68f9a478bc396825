"""Seeded weights of the spherical-harmonics colour branch of the dense NeRF (models/nerf.py:82-83, :123-143 with rgb_dim = 3 (d + 1)^2,
pos_dir_dim = 0) with the reference model's names and shapes.  The fixture generator (scripts/gen_golden_sh.py) and the tests
regenerate them; no fixture stores them."""
from __future__ import annotations

import numpy as np

import synth

SH_RGB_SCALE = 4.0      # the colour head's init scaled up: the coefficients are O(1), so the higher bands move the colour visibly

# layer_dim 256 is the narrowest model the dense head kernels take; everything else is small (a fixture stores its seed, not weights)
SH_CFG = dict(layer_dim=256, layers=3, skip_layers=(1,), pos_xyz_dim=4, pos_dir_dim=0, appearance_dim=8, appearance_count=4, xyz_dim=3)


def sh_cfg(deg: int, cfg=SH_CFG):
    return dict(cfg, sh_deg=int(deg))


def make_sh_weights(seed: int, deg: int, cfg=SH_CFG):
    """{state_dict key: np.float32 array}: synth.make_dense_weights(seed) with dir_a_encoding cut to its [xyz_encoding_final, embedding]
    columns (in_channels_dir = 0: no direction block) and rgb.weight [3 B, W / 2] / rgb.bias [3 B], B = (deg + 1)^2."""
    assert cfg["pos_dir_dim"] == 0
    sd = synth.make_dense_weights(seed, cfg)
    W, B = cfg["layer_dim"], (deg + 1) ** 2
    sd["dir_a_encoding.0.weight"] = np.ascontiguousarray(sd["dir_a_encoding.0.weight"][:, : W + cfg["appearance_dim"]])
    rng = np.random.default_rng(seed + 9200)
    sd["rgb.weight"], sd["rgb.bias"] = synth._linear(rng, 3 * B, W // 2, scale=SH_RGB_SCALE)
    return sd


# ---- inputs of the kernel-level tests (tests/test_sh_kernels_gpu.py); scripts/gen_golden_sh.py runs the reference formulation in fp32 on
# the same arrays and stores its error against fp64 (tests/golden/sh_heads_bounds.npz), which is what the fp32 bounds are made of
HEAD_SHAPES = ((1, 1), (5, 13), (3, 64), (7, 37), (300, 96))
HEAD_M, HEAD_H2 = 256, 128


def head_cases():
    """(deg, N, S, rows_per_group, noise): every degree on every shape with rows_per_group = S (noise on every other case), and
    rows_per_group = 1 - every row its own direction - on two shapes."""
    out = []
    for deg in range(5):
        for i, (N, S) in enumerate(HEAD_SHAPES):
            out.append((deg, N, S, S, (deg + i) % 2 == 1))
        out += [(deg, 5, 13, 1, True), (deg, 7, 37, 1, False)]
    return out


def case_key(deg, N, S, rpg, noise):
    return f"d{deg}_n{N}_s{S}_g{rpg}_z{int(noise)}"


def head_case(deg, N, S, rpg, noise, seed=4100):
    """fp32 inputs of one case: post-ReLU activations (exact zeros included), directions of length 0.5 .. 2 (never normalised), a zero
    suffix in d_raw (the last quarter of the rows)."""
    rng = np.random.default_rng(seed + 1000 * deg + 7 * N + S + 3 * rpg)
    P, B, M, H2 = N * S, (deg + 1) ** 2, HEAD_M, HEAD_H2
    f = lambda a: np.ascontiguousarray(a, np.float32)
    d = rng.standard_normal((P // rpg, 3))
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (P // rpg, 1))
    c = dict(y=f(np.maximum(rng.standard_normal((P, M)), 0)), h2=f(np.maximum(rng.standard_normal((P, H2)), 0)),
             ws=f(rng.uniform(-1, 1, M) / 16), bs=f(rng.uniform(-1, 1, 1)), wc=f(rng.uniform(-1, 1, (3 * B, H2)) / 8),
             bc=f(rng.uniform(-1, 1, 3 * B)), dirs=f(d), noise=f(rng.standard_normal(P)) if noise else None,
             d_raw=f(rng.standard_normal((P, 4))))
    c["d_raw"][P - P // 4:] = 0
    return c
