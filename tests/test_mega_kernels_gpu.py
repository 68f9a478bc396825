"""The spatial-cell kernels of the Mega-NeRF model (csrc/cells.hip: swn_cells_assign / _pack / _gather / _blend) against the pure-torch
restatement (tests/mega_restate.py, pinned on the reference by tests/test_mega_cpu.py) at the smallest shapes that can still go wrong:
below a wave, a ragged last block, several blocks for the scan; one cell, an odd count, a multiple of four.

What decides an order (counts, begin, rows, slot) and what is copied (the gathered rows) must equal the restatement's exactly.  The
weights and the blend are bounded by the reference's own float32-versus-float64 error on the fixture, times 4 (weights_tol / blend_tol
of tests/golden/mega_fg.npz, measured by scripts/gen_golden_mega.py - not derived from the kernels)."""
import os

import numpy as np
import pytest
import torch

import mega_restate as R

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tols():
    g = np.load(os.path.join(G, "mega_fg.npz"))
    return float(g["weights_tol"]), float(g["blend_tol"])


def _inputs(seed, P, K, xyz_real, centroids=None):
    rng = np.random.default_rng(seed)
    stride = 11 if xyz_real else 7
    x = rng.uniform(-1, 1, (P, stride)).astype(np.float32)
    cen = rng.uniform(-0.8, 0.8, (K, 3)).astype(np.float32) if centroids is None else np.asarray(centroids, np.float32)
    noise = rng.standard_normal(P).astype(np.float32)
    return x, cen, noise


def _run(x, cen, noise, dim_start, margin, xyz_real, subs):
    """Everything the four entry points produce for one input, as numpy arrays."""
    from switch_nerf_amd import ops
    xd = _dev(x)
    w, counts = ops.cells_assign(xd, _dev(cen), dim_start, margin)
    begin, rows, slot = ops.cells_pack(w, counts)
    total = int(counts.sum().item())
    xin, nin = ops.cells_gather(xd, rows, total, 3 if xyz_real else 0, _dev(noise))
    outs = [ops.cells_blend(w, slot, begin, _dev(s[:total]), margin == 1) for s in subs]
    return [t.cpu().numpy() for t in (w, counts, begin, rows[:total], slot, xin, nin, *outs)]


def _check(x, cen, noise, dim_start, margin, xyz_real, seed):
    w_tol, b_tol = _tols()
    P, K = len(x), len(cen)
    w_ref = R.assign(x, cen, dim_start, margin)
    counts, begin, rows, slot = R.pack(w_ref)
    rng = np.random.default_rng(seed + 1)
    subs = [rng.uniform(0, 1, (P * K, C)).astype(np.float32) for C in (1, 4)]
    got = _run(x, cen, noise, dim_start, margin, xyz_real, subs)
    w, g_counts, g_begin, g_rows, g_slot, xin, nin, out1, out4 = got
    np.testing.assert_array_equal(g_counts, counts)
    np.testing.assert_array_equal(g_begin, begin)
    np.testing.assert_array_equal(g_rows, rows)
    np.testing.assert_array_equal(g_slot, slot)
    err = np.abs(w - w_ref.numpy()).max()
    xin_ref, nin_ref = R.gather(x, rows, 3 if xyz_real else 0, noise)
    np.testing.assert_array_equal(xin, xin_ref.numpy())
    np.testing.assert_array_equal(nin, nin_ref.numpy())
    total = int(begin[-1])
    b_err = 0.0
    for out, sub in ((out1, subs[0]), (out4, subs[1])):
        ref = R.blend(w_ref, slot, begin, sub[:total], margin == 1).numpy()
        assert out.shape == ref.shape
        b_err = max(b_err, float(np.abs(out - ref).max()))
    print(f"P {P} K {K} margin {margin} dim_start {dim_start}: weights err {err:.3e} (bound {w_tol:.3e}), blend err {b_err:.3e} (bound {b_tol:.3e})")
    assert err <= w_tol and b_err <= b_tol
    again = _run(x, cen, noise, dim_start, margin, xyz_real, subs)      # two runs: the same bits
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()
    return got


@pytest.mark.parametrize("margin", [1.0, 1.15, 2.0])
@pytest.mark.parametrize("K", [1, 5, 8])
@pytest.mark.parametrize("P", [1, 63, 1000, 4097])
def test_cells_vs_restatement(P, K, margin):
    seed = 1000 * K + P + int(margin * 100)
    flag = (P + K) % 2 == 1              # cluster_2d and xyz_real on for half of the shapes, in both combinations over the grid
    cluster_2d, xyz_real = flag, (K % 2 == 1) != flag
    x, cen, noise = _inputs(seed, P, K, xyz_real)
    _check(x, cen, noise, 1 if cluster_2d else 0, margin, xyz_real, seed)


@pytest.mark.parametrize("margin", [1.0, 1.15])
def test_cells_empty_cell(margin):
    """One centroid far away: its cell has no member, begin repeats, the cells behind it are packed right after the ones before."""
    x, cen, noise = _inputs(71, 1000, 5, False)
    cen[2] = (40.0, -40.0, 40.0)
    got = _check(x, cen, noise, 0, margin, False, 71)
    assert got[1][2] == 0 and got[2][2] == got[2][3] and (got[4][:, 2] == -1).all()


@pytest.mark.parametrize("margin", [1.0, 1.15])
def test_cells_exact_ties(margin):
    """Two identical centroids: the hard assignment takes the first index (argmin); with a margin both are members with equal weights."""
    x, cen, noise = _inputs(72, 1000, 5, False)
    cen[3] = cen[1]
    got = _check(x, cen, noise, 0, margin, False, 72)
    w, counts = got[0], got[1]
    if margin == 1:
        assert counts[3] == 0 and counts[1] > 0
    else:
        assert counts[3] == counts[1] > 0 and np.array_equal(w[:, 1], w[:, 3])


@pytest.mark.parametrize("margin", [1.0, 1.15])
def test_cells_largest_cell_count(margin):
    """K = 64, the most the kernels hold: the whole 192-float centroid load, bit 63 of the membership mask, and the scan's narrowest
    layout (16 runs of blocks per cell) over five blocks."""
    x, cen, noise = _inputs(74, 1100, 64, False)
    got = _check(x, cen, noise, 0, margin, False, 74)
    assert got[1][63] > 0            # (the last cell has members, so its mask bit and its scan column are exercised)


def test_cells_more_than_64_cells_is_an_error():
    from switch_nerf_amd import ops
    x, cen, _ = _inputs(73, 63, 65, False)
    with pytest.raises(RuntimeError, match=r"n_cells 65 outside \[1, 64\]"):
        ops.cells_assign(_dev(x), _dev(cen), 0, 1.15)
    w = torch.zeros(63, 65, device="cuda")
    with pytest.raises(RuntimeError, match=r"n_cells 65 outside \[1, 64\]"):
        ops.cells_pack(w, torch.zeros(65, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match=r"n_cells 65 outside \[1, 64\]"):
        ops.cells_blend(w, torch.zeros(63, 65, dtype=torch.int32, device="cuda"), torch.zeros(66, dtype=torch.int32, device="cuda"),
                        torch.zeros(63, 4, device="cuda"), False)
