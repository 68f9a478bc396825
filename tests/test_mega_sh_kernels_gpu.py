"""swn_cells_blend_sh (csrc/sh.hip: the Mega-NeRF blend of rows of 3 B coefficients + sigma, fused with sigmoid(eval_sh)) against the
float64 restatement (tests/mega_sh_restate.py, pinned on the reference by tests/test_mega_sh_cpu.py), fp32, at the smallest shapes
that can still go wrong: below a 16-lane group, around a wave, a ragged last 64-point tile, several tiles; one cell, an odd count,
all four 16-cell rounds of the slot reads (K = 64); rows of 4, 28 and 76 floats (1, 2 and 5 values per lane).

Bound: blend_sh_tol of tests/golden/mega_sh_fg_d{deg}.npz - 4 x the reference's own float32-against-float64 error of the same formula
on that fixture (scripts/gen_golden_mega_sh.py), not derived from the kernel.  The inputs here are no larger than the fixture's
(coefficients and sigma in [-1, 1], directions of length 0.8 .. 1.25 like its, weights that sum to 1), so the absolute bound carries over; with every cell a member (margin 1e6, 64
terms) the float32 formula evaluated on the CPU in the reference's order stays below 1.7e-7 against bounds of 2.8e-7 .. 5e-7.
The membership, the packing and the weights come from the restatement of the router (tests/mega_restate.py) and are given to the kernel
and to the yardstick alike."""
import os

import numpy as np
import pytest
import torch

import mega_restate as R
import mega_sh_restate as RS

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tol(deg):
    return float(np.load(os.path.join(G, f"mega_sh_fg_d{deg}.npz"))["blend_sh_tol"])


def _case(seed, P, K, deg, margin, rpg, centroids=None):
    """weights / slot / begin of P points among K cells, packed rows of 3 B + 1 floats, directions of length 0.8 .. 1.25: not
    normalised, and inside the range of the fixture's own - a degree-4 basis grows with the fourth power of the length, and with it
    the size of the sums the absolute bound was measured on."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (P, 4)).astype(np.float32)
    cen = rng.uniform(-0.8, 0.8, (K, 3)).astype(np.float32) if centroids is None else np.asarray(centroids, np.float32)
    w = R.assign(x, cen, 0, margin).numpy()
    counts, begin, rows, slot = R.pack(w)
    sub = rng.uniform(-1, 1, (int(begin[-1]), 3 * (deg + 1) ** 2 + 1)).astype(np.float32)
    d = rng.standard_normal((P // rpg, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.8, 1.25, (P // rpg, 1))).astype(np.float32)
    return dict(w=w, counts=counts, begin=begin, slot=slot, sub=sub, dirs=d, rpg=rpg, deg=deg, hard=margin == 1)


def _run(c, want_coef=True, hard=None):
    from switch_nerf_amd import ops
    out = ops.cells_blend_sh(_dev(c["w"]), _dev(c["slot"]), _dev(c["begin"]), _dev(c["sub"]), _dev(c["dirs"]), c["rpg"], c["deg"],
                             c["hard"] if hard is None else hard, want_coef=want_coef)
    return tuple(t.cpu().numpy() for t in out) if want_coef else out.cpu().numpy()


def _check(c):
    raw, coef = _run(c)
    ref_raw, ref_rows = RS.blend_sh(c["w"], c["slot"], c["begin"], c["sub"], c["dirs"], c["rpg"], c["deg"], c["hard"])
    tol = _tol(c["deg"])
    assert raw.shape == ref_raw.shape and coef.shape == ref_rows.shape
    e_raw, e_coef = float(np.abs(raw - ref_raw).max()), float(np.abs(coef - ref_rows).max())
    print(f"P {len(c['w'])} K {c['w'].shape[1]} deg {c['deg']} rpg {c['rpg']} hard {c['hard']}: raw err {e_raw:.3e}, rows err {e_coef:.3e} (bound {tol:.3e})")
    assert e_raw <= tol and e_coef <= tol
    only = _run(c, want_coef=False)                     # raw: the same bits with and without coef_out, and from one run to the next
    assert only.tobytes() == raw.tobytes()
    again = _run(c)
    assert again[0].tobytes() == raw.tobytes() and again[1].tobytes() == coef.tobytes()
    return raw, coef


@pytest.mark.parametrize("rpg", [1, 8])
@pytest.mark.parametrize("margin", [1.0, 1.15, 1e6])
@pytest.mark.parametrize("deg", [0, 2, 4])
@pytest.mark.parametrize("K", [1, 3, 64])
@pytest.mark.parametrize("P", [1, 63, 65, 1000])
def test_blend_sh_vs_restatement(P, K, deg, margin, rpg):
    if P % rpg:
        P = (P + rpg - 1) // rpg * rpg                  # 1 -> 8, 63 -> 64, 65 -> 72 with one direction per 8 rows: still below / around / past a tile
    c = _case(10000 * deg + 100 * K + P + int(margin * 7) % 97 + rpg, P, K, deg, margin, rpg)
    if margin == 1e6:
        assert (c["slot"] >= 0).all()                   # every cell a member of every point
    _check(c)


@pytest.mark.parametrize("margin", [1.0, 1.15])
def test_blend_sh_empty_cell(margin):
    rng = np.random.default_rng(5)
    cen = rng.uniform(-0.8, 0.8, (5, 3)).astype(np.float32)
    cen[2] = (40.0, -40.0, 40.0)
    c = _case(81, 1000, 5, 2, margin, 8, cen)
    assert c["counts"][2] == 0 and c["begin"][2] == c["begin"][3] and (c["slot"][:, 2] == -1).all()
    _check(c)


@pytest.mark.parametrize("margin", [1.0, 1.15])
def test_blend_sh_exact_ties(margin):
    """Two identical centroids: hard - only the first is a member; soft - both, with equal weights, added in ascending cell order."""
    rng = np.random.default_rng(6)
    cen = rng.uniform(-0.8, 0.8, (5, 3)).astype(np.float32)
    cen[3] = cen[1]
    c = _case(82, 1000, 5, 4, margin, 1, cen)
    if margin == 1:
        assert c["counts"][3] == 0 and c["counts"][1] > 0
    else:
        assert c["counts"][3] == c["counts"][1] > 0 and np.array_equal(c["w"][:, 1], c["w"][:, 3])
    _check(c)


def test_blend_sh_single_member_under_a_soft_margin():
    """A point in exactly one cell under a soft margin: weight 1 (the reference still multiplies), the row and its evaluation unchanged."""
    c = _case(83, 1000, 3, 2, 1.15, 8)
    single = (c["slot"] >= 0).sum(1) == 1
    assert 0 < single.sum() < len(single) and (c["w"][single].max(1) == 1).all()
    raw, coef = _check(c)
    i = np.nonzero(single)[0]
    cell = (c["slot"][i] >= 0).argmax(1)
    member = c["sub"][c["begin"][cell] + c["slot"][i, cell]]
    np.testing.assert_array_equal(coef[i], member + np.float32(0))      # 0 + row * 1: the row (a -0 would come out as +0)
    np.testing.assert_array_equal(raw[i, 3], coef[i, -1])


@pytest.mark.parametrize("deg", [0, 2, 4])
def test_blend_sh_hard_copies_the_member_row(deg):
    """hard: the blended rows ARE the member rows (no multiply), and raw is bit-equal to the member rows alone pushed through the same
    evaluation (one cell, identity packing)."""
    from switch_nerf_amd import ops
    P, K = 1000, 5
    c = _case(84 + deg, P, K, deg, 1.0, 8)
    c["sub"][3::11, 0] = np.float32(-0.0)                               # a copy keeps the sign of zero, 0 + (-0 * 1) does not
    c["w"] = c["w"] * np.float32(0.5)                                   # (hard never reads the weights' values)
    raw, coef = _run(c)
    cell = (c["slot"] >= 0).argmax(1)
    member = c["sub"][c["begin"][cell] + c["slot"][np.arange(P), cell]]
    assert coef.tobytes() == member.tobytes()
    one = dict(c, w=np.ones((P, 1), np.float32), slot=np.arange(P, dtype=np.int32)[:, None], begin=np.array([0, P], np.int32), sub=member)
    raw1, coef1 = _run(one)
    assert raw1.tobytes() == raw.tobytes() and coef1.tobytes() == member.tobytes()


def test_blend_sh_sigma_channel_is_cells_blend_at_degree_0():
    """B = 1: the rows are four floats like swn_cells_blend's; the blended rows agree with it bit for bit (sigma and the coefficients)."""
    from switch_nerf_amd import ops
    for margin in (1.0, 1.15, 1e6):
        c = _case(90 + int(margin) % 7, 1000, 8, 0, margin, 1)
        _, coef = _run(c)
        ref = ops.cells_blend(_dev(c["w"]), _dev(c["slot"]), _dev(c["begin"]), _dev(c["sub"]), c["hard"]).cpu().numpy()
        assert coef[:, 3].tobytes() == ref[:, 3].tobytes() and coef.tobytes() == ref.tobytes()


def test_blend_sh_error_codes():
    from switch_nerf_amd import ops
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")
    def call(P=64, K=3, deg=2, rpg=8, n_dirs=None, width=None):
        n_dirs = max(P // max(rpg, 1), 1) if n_dirs is None else n_dirs
        return ops.cells_blend_sh(z(P, K), z(P, K, dt=torch.int32), z(K + 1, dt=torch.int32), z(P, 28 if width is None else width), z(n_dirs, 3),
                                  rpg, deg, False)
    assert call().shape == (64, 4)
    with pytest.raises(RuntimeError, match=r"n_cells 65 outside \[1, 64\]"):
        call(K=65)
    for deg in (-1, 5):
        with pytest.raises(RuntimeError, match=rf"deg {deg} outside 0\.\.4"):
            call(deg=deg)
    for rpg in (0, -3):
        with pytest.raises(RuntimeError, match=rf"rows_per_group {rpg} < 1"):
            call(rpg=rpg)
    with pytest.raises(RuntimeError, match=r"n_points 63 is no multiple of rows_per_group 8"):
        call(P=63, n_dirs=8)
