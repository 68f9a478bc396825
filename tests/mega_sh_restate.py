"""Numpy restatement of the Mega-NeRF blend for sub-models with spherical-harmonics colour: the reference's loop over the cells
(models/mega_nerf.py:34-49) on rows of 3 B coefficients + sigma, then rendering.py:344-349, rgb = sigmoid(eval_sh(deg, coefficients,
direction)).  Written from those formulas in any numpy dtype: in float64 it is the yardstick of the kernel tests
(tests/test_mega_sh_kernels_gpu.py) and of the fixtures' error figure (scripts/gen_golden_mega_sh.py); tests/test_mega_sh_cpu.py pins it
on the reference's own results.  The membership and the packing are tests/mega_restate.py's; the basis is tests/sh_restate.py's."""
import numpy as np
import torch

import sh_restate as SR


def basis(deg, dirs, dtype=np.float64):
    """Y [N, (deg + 1)^2] at dirs [N, 3], taken as given (not normalised)."""
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(dirs, dtype)))
    return SR.basis(int(deg), t).numpy()


def blend_rows(weights, slot, begin, sub_out, hard, dtype=np.float64):
    """[P, C]: out[mask_i] (+)= sub_out rows of cell i (* weights[:, i]), the cells in ascending order."""
    w, sub = np.asarray(weights, dtype), np.asarray(sub_out, dtype)
    slot, begin = np.asarray(slot, np.int64), np.asarray(begin, np.int64)
    out = np.zeros((w.shape[0], sub.shape[1]), dtype)
    for i in range(w.shape[1]):
        m = slot[:, i] >= 0
        r = sub[begin[i] + slot[m, i]]
        if hard:
            out[m] = r
        else:
            out[m] += r * w[m, i][:, None]
    return out


def eval_rows(rows, dirs, rows_per_group, deg, dtype=np.float64):
    """rows [P, 3 B + 1] (coefficients row-major [3, B], then sigma), point p seen along dirs[p // rows_per_group] -> [P, 4]."""
    rows = np.asarray(rows, dtype)
    P, B = rows.shape[0], (deg + 1) ** 2
    assert rows.shape[1] == 3 * B + 1 and P % rows_per_group == 0
    Y = np.repeat(basis(deg, dirs, dtype), rows_per_group, 0)                  # [P, B]
    lin = (rows[:, :3 * B].reshape(P, 3, B) * Y[:, None, :]).sum(-1)
    return np.concatenate([1 / (1 + np.exp(-lin)), rows[:, 3 * B:]], 1)


def blend_sh(weights, slot, begin, sub_out, dirs, rows_per_group, deg, hard, dtype=np.float64):
    """-> (raw [P, 4], blended rows [P, 3 B + 1]): what swn_cells_blend_sh computes."""
    rows = blend_rows(weights, slot, begin, sub_out, hard, dtype)
    return eval_rows(rows, dirs, rows_per_group, deg, dtype), rows
