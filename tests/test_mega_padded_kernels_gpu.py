"""The padded row space of the Mega-NeRF cells (csrc/cells.hip: swn_cells_pack_padded, swn_cells_gather_padded, and swn_cells_blend /
swn_cells_blend_bwd on the fixed begin[] it returns) against a numpy construction from swn_cells_assign's own weights and against the
compact layout's kernels (ops.cells_pack / cells_blend / cells_blend_bwd), bit for bit.

Sizes: P on both sides of a wave (63, 64, 65), one point, a non-multiple of the 256-point block (1000) and several blocks of the scan
(8193); K = 1, 3 and the 64 the kernels hold; hard and soft margin; capacity C = the largest cell's count (everything fits exactly),
one less (at least one membership dropped: a handled input, asserted in range) and P (mostly padding).  C = max count - 1 does not exist
where the largest cell has one member (capacity 0 is not a capacity: the entry point refuses it, asserted below).
Buffers passed to the library directly carry a guard band behind K C rows that must come back untouched."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GUARD = 64
SENT_I, SENT_F = -77, 12345.0


def _points(P, K, seed, far=()):
    """x [P, 7] (position, direction, image index), sigma noise [P], centroids [K, 3]; the centroids in `far` are moved out of reach."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (P, 7)).astype(np.float32)
    x[:, 6] = rng.integers(0, 4, P)
    cen = rng.uniform(-1, 1, (K, 3)).astype(np.float32)
    for i in far:
        cen[i] = 1e3 + i
    return x, rng.standard_normal(P).astype(np.float32), cen


def _reference(w, C):
    """(rows [K C], slot [P, K], counts [K], overflow) of the membership w > 0, by the definition: ranks ascend with the point index."""
    P, K = w.shape
    member = w > 0
    counts = member.sum(0).astype(np.int32)
    rank = np.cumsum(member, 0) - 1
    fits = member & (rank < C)
    slot = np.where(fits, rank, -1).astype(np.int32)
    rows = np.full(K * C, -1, np.int32)
    p, i = np.nonzero(fits)
    rows[i * C + rank[p, i]] = p
    return rows, slot, counts, int(np.maximum(counts - C, 0).sum())


def _run(x, noise, cen, margin, C):
    """Every padded kernel once, on buffers with a guard band -> dict of host arrays (guards included)."""
    from switch_nerf_amd import _lib, ops
    P, K = x.shape[0], cen.shape[0]
    hard = margin == 1.0
    dx, dn, dc = (torch.from_numpy(a).cuda() for a in (x, noise, cen))
    w, counts = ops.cells_assign(dx, dc, 0, margin)
    begin = torch.full((K + 1 + GUARD,), SENT_I, dtype=torch.int32, device="cuda")
    rows = torch.full((K * C + GUARD,), SENT_I, dtype=torch.int32, device="cuda")
    slot = torch.full((P * K + GUARD,), SENT_I, dtype=torch.int32, device="cuda")
    over = torch.full((1 + GUARD,), SENT_I, dtype=torch.int32, device="cuda")
    need = ctypes.c_size_t(0)
    _lib.call("swn_cells_pack_workspace_bytes", P, K, ctypes.byref(need))
    ws = torch.empty(max(1, need.value // 4), dtype=torch.int32, device="cuda")
    _lib.call("swn_cells_pack_padded", ops._p(w), ops._p(counts), P, K, C, ops._p(begin), ops._p(rows), ops._p(slot), ops._p(over), ops._p(ws),
              need.value, ops._stream())
    x_out = torch.full((K * C * 7 + GUARD,), SENT_F, dtype=torch.float32, device="cuda")
    n_out = torch.full((K * C + GUARD,), SENT_F, dtype=torch.float32, device="cuda")
    _lib.call("swn_cells_gather_padded", ops._p(dx), 7, 0, ops._p(rows), ops._p(dc), K, C, P, ops._p(dn), ops._p(x_out), ops._p(n_out),
              ops._stream())
    # the compact layout of the same weights, a sub-model output per compact row, and the same rows laid out padded (NaN elsewhere: a
    # padding row that reached a blend would show)
    cb, crows, cslot = ops.cells_pack(w, counts)
    nc = counts.cpu().numpy()
    total = int(nc.sum())
    rng = np.random.default_rng(7)
    sub_c = rng.standard_normal((max(total, 1), 4)).astype(np.float32)
    sub_p = np.full((K * C, 4), np.nan, np.float32)
    cbeg = np.concatenate([[0], np.cumsum(nc)])
    for i in range(K):
        n = min(int(nc[i]), C)
        sub_p[i * C:i * C + n] = sub_c[cbeg[i]:cbeg[i] + n]
    b, r, s = begin[:K + 1].contiguous(), rows[:K * C].contiguous(), slot[:P * K].view(P, K).contiguous()
    out_p = ops.cells_blend(w, s, b, torch.from_numpy(sub_p).cuda(), hard)
    out_c = ops.cells_blend(w, cslot, cb, torch.from_numpy(sub_c).cuda(), hard)
    d_out = torch.from_numpy(rng.standard_normal((P, 4)).astype(np.float32)).cuda()
    d_sub = torch.full((K * C * 4 + GUARD,), SENT_F, dtype=torch.float32, device="cuda")
    _lib.call("swn_cells_blend_bwd", ops._p(w), ops._p(r), ops._p(b), ops._p(d_out), K * C, P, K, 4, 1 if hard else 0, ops._p(d_sub), ops._stream())
    d_sub_c = ops.cells_blend_bwd(w, crows, cb, d_out, total, hard)
    torch.cuda.synchronize()
    host = dict(w=w, counts=counts, begin=begin, rows=rows, slot=slot, over=over, x_out=x_out, n_out=n_out, out_p=out_p, out_c=out_c, d_sub=d_sub,
                d_sub_c=d_sub_c, cslot=cslot)
    return {k: v.cpu().numpy() for k, v in host.items()}, cbeg


def _check(x, noise, cen, margin, C):
    P, K = x.shape[0], cen.shape[0]
    g, cbeg = _run(x, noise, cen, margin, C)
    ref_rows, ref_slot, ref_counts, ref_over = _reference(g["w"], C)
    # pack: rows, slot, the true counts (also above C), the overflow count, the fixed begin[]; nothing behind K C
    np.testing.assert_array_equal(g["counts"], ref_counts)
    np.testing.assert_array_equal(g["begin"][:K + 1], np.arange(K + 1) * C)
    np.testing.assert_array_equal(g["rows"][:K * C], ref_rows)
    np.testing.assert_array_equal(g["slot"][:P * K].reshape(P, K), ref_slot)
    assert g["over"][0] == ref_over
    for name, n in (("begin", K + 1), ("rows", K * C), ("slot", P * K), ("over", 1)):
        assert (g[name][n:] == SENT_I).all(), name
    # gather: real rows are x[rows] bit for bit, padding rows (centroid, (0, 0, 1), 0) with noise 0; the guard band untouched
    real = ref_rows >= 0
    xo, no = g["x_out"][:K * C * 7].reshape(K * C, 7), g["n_out"][:K * C]
    assert np.array_equal(xo[real].view(np.uint32), x[ref_rows[real]].view(np.uint32))
    assert np.array_equal(no[real].view(np.uint32), noise[ref_rows[real]].view(np.uint32))
    pad = np.concatenate([np.repeat(cen, C, 0), np.tile(np.array([0, 0, 1, 0], np.float32), (K * C, 1))], 1)
    assert np.array_equal(xo[~real].view(np.uint32), pad[~real].view(np.uint32))
    assert not no[~real].view(np.uint32).any()
    assert (g["x_out"][K * C * 7:] == SENT_F).all() and (g["n_out"][K * C:] == SENT_F).all()
    # blend: a point with no dropped member equals the compact layout's blend bit for bit; one with every member dropped is zero
    member = g["w"] > 0
    dropped = member & (ref_slot < 0)
    whole, none = ~dropped.any(1), member.any(1) & (dropped == member).all(1)
    assert np.array_equal(g["out_p"][whole].view(np.uint32), g["out_c"][whole].view(np.uint32))
    assert not g["out_p"][none].view(np.uint32).any()
    assert np.isfinite(g["out_p"]).all()              # (no padding row, NaN in this test, was read)
    if ref_over == 0:
        assert whole.all()
    else:
        assert not whole.all()
    # blend backward: a real row equals the compact layout's row of the same (point, cell); a padding row is +0; nothing behind K C
    ds = g["d_sub"][:K * C * 4].reshape(K * C, 4)
    cell = np.arange(K * C) // C
    compact_row = cbeg[cell[real]] + g["cslot"][ref_rows[real], cell[real]]
    assert np.array_equal(ds[real].view(np.uint32), g["d_sub_c"][compact_row].view(np.uint32))
    assert not ds[~real].view(np.uint32).any()        # == 0 and no sign bit
    assert (g["d_sub"][K * C * 4:] == SENT_F).all()
    # two runs give the same bits
    g2, _ = _run(x, noise, cen, margin, C)
    for k in ("rows", "slot", "over", "x_out", "n_out", "out_p", "d_sub"):
        assert np.array_equal(g[k].view(np.uint32), g2[k].view(np.uint32)), k
    return ref_counts, ref_over


def _max_count(x, cen, margin):
    from switch_nerf_amd import ops
    _, counts = ops.cells_assign(torch.from_numpy(x).cuda(), torch.from_numpy(cen).cuda(), 0, margin)
    return int(counts.max().item())


@pytest.mark.parametrize("margin", [1.0, 1.15])
@pytest.mark.parametrize("K", [1, 3, 64])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 1000, 8193])
def test_padded_kernels_vs_reference_construction(P, K, margin):
    x, noise, cen = _points(P, K, 1000 * K + P)
    top = _max_count(x, cen, margin)
    for C in (top, top - 1, P):
        if C < 1:          # the largest cell has one member: there is no smaller capacity
            continue
        counts, over = _check(x, noise, cen, margin, C)
        assert (over == 0) == (C >= top) and (C != top - 1 or over >= 1)
        print(f"P {P} K {K} margin {margin} C {C}: largest cell {counts.max()}, dropped {over}, padding rows {K * C - int(np.minimum(counts, C).sum())}")


@pytest.mark.parametrize("margin", [1.0, 1.15])
def test_padded_kernels_with_an_empty_cell_and_with_one_cell_holding_everything(margin):
    P = 1000
    x, noise, cen = _points(P, 3, 5, far=(1,))                     # cell 1 out of reach: empty, its range all padding
    top = _max_count(x, cen, margin)
    for C in (top, top - 1, P):
        counts, _ = _check(x, noise, cen, margin, C)
        assert counts[1] == 0 and counts[0] > 0 and counts[2] > 0
    x, noise, cen = _points(P, 3, 6, far=(0, 2))                   # every point in cell 1
    for C in (P, P - 1):
        counts, over = _check(x, noise, cen, margin, C)
        assert counts.tolist() == [0, P, 0] and over == P - C


def test_padded_entry_points_validate_before_launch():
    from switch_nerf_amd import _lib, ops
    lib = _lib.load()
    p = torch.zeros(64, dtype=torch.float32, device="cuda")
    q = ops._p(p)
    err = lambda: lib.swn_last_error().decode()
    assert lib.swn_cells_pack_padded(q, q, 4, 3, 0, q, q, q, q, q, 1024, None) != 0 and "capacity 0" in err()
    assert lib.swn_cells_pack_padded(q, q, 4, 65, 4, q, q, q, q, q, 1024, None) != 0 and "n_cells" in err()
    assert lib.swn_cells_pack_padded(q, q, 4, 3, 4, q, q, q, None, q, 1024, None) != 0 and "null pointer" in err()
    assert lib.swn_cells_pack_padded(q, q, 4, 64, 1 << 26, q, q, q, q, q, 1024, None) != 0 and "32-bit row space" in err()
    assert lib.swn_cells_pack_padded(q, q, 1000, 3, 4, q, q, q, q, q, 8, None) != 0 and "workspace" in err()
    assert lib.swn_cells_gather_padded(q, 8, 0, q, q, 3, 4, 4, None, q, None, None) != 0 and "7" in err()
    assert lib.swn_cells_gather_padded(q, 7, 0, q, q, 3, 0, 4, None, q, None, None) != 0 and "capacity 0" in err()
    assert lib.swn_cells_gather_padded(q, 7, 0, q, q, 3, 4, 4, q, q, None, None) != 0 and "come together" in err()
    assert lib.swn_cells_gather_padded(q, 7, 0, q, None, 3, 4, 4, None, q, None, None) != 0 and "null pointer" in err()
