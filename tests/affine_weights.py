"""Seeded weights and image indices of the affine_appearance branch (models/nerf_moe.py:153-161, 436-438) with the reference model's
names and shapes.  The fixture generator (scripts/gen_golden_affine.py) and the tests regenerate them; no fixture stores them."""
from __future__ import annotations

import numpy as np

import synth

AFFINE_SCALE = 0.5      # the matrices are the identity map plus entries of ~0.3 (unit-variance embeddings of 48 values)
UNHIT_IMAGE = 3         # no ray of affine_image_indices() belongs to this image: its embedding row gets an exactly-zero gradient


def affine_cfg(cfg=synth.BUILDING):
    return dict(cfg, affine_appearance=True)


def make_affine_weights(seed: int, cfg=synth.BUILDING, gate_scale: float = 1.0):
    """{state_dict key: np.float32 array} of an affine model: synth.make_weights(seed) with layer "2" cut to its [h, PE(dir)] columns
    (in_ch = M + 27: the embedding no longer enters it) plus affine.weight [12, appearance_dim] / affine.bias [12]."""
    sd = synth.make_weights(seed, cfg, gate_scale=gate_scale)
    in_dir = 3 + 3 * 2 * cfg["pos_dir_dim"]
    sd["layers.2.fcs.0.weight"] = np.ascontiguousarray(sd["layers.2.fcs.0.weight"][:, : cfg["model_dim"] + in_dir])
    rng = np.random.default_rng(seed + 9000)
    w, b = synth._linear(rng, 12, cfg["appearance_dim"], scale=AFFINE_SCALE)
    sd["affine.weight"] = w
    sd["affine.bias"] = (b + np.eye(3, 4, dtype=np.float32).reshape(-1)).astype(np.float32)
    return sd


def affine_image_indices(seed: int, n: int, appearance_count: int = 10):
    """n image indices over the images other than UNHIT_IMAGE (several rays share an image once n exceeds the image count)."""
    rng = np.random.default_rng(seed + 9100)
    pool = np.array([i for i in range(appearance_count) if i != UNHIT_IMAGE], np.int64)
    return pool[rng.integers(0, len(pool), size=(n,))]
