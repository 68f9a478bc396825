"""swn_cells_blend_bwd (csrc/cells.hip), the backward of the Mega-NeRF cell blend, against torch's autograd through the restated blend
(tests/mega_train_restate.py -> tests/mega_restate.blend) on the CPU.

The operation is one copy (hard) or one float32 multiply (soft) per element - no sum - so the derived bound is equality of the bits:
assert_array_equal.  Shapes: below a block, a block, one over, several blocks with a ragged last one; one cell, an odd count, the
most the kernels hold (64: the whole staged begin[] and the longest bisection); 1 and 4 channels; the hard copy, the soft blend at
1.15, and a margin so wide that every point belongs to every cell (total = P K, the longest row list)."""
import numpy as np
import pytest
import torch

import mega_restate as R
import mega_train_restate as RT

pytestmark = pytest.mark.gpu
MARGINS = [1.0, 1.15, 1e6]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _case(seed, P, K, margin, far=()):
    """weights (mega_restate.assign) and packing of P random points among K random centroids; the cells named in `far` get no member."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (P, 3)).astype(np.float32)
    cen = rng.uniform(-0.8, 0.8, (K, 3)).astype(np.float32)
    for i in far:
        cen[i] = (4e7, -4e7, 4e7)           # (beyond even the 1e6 margin of the nearest cell's distance)
    w = R.assign(x, cen, 0, margin)
    counts, begin, rows, slot = R.pack(w)
    return w, counts, begin, rows, slot, rng


def _check(w, begin, rows, slot, rng, margin):
    from switch_nerf_amd import ops
    P, K = w.shape
    total, hard = int(begin[-1]), margin == 1
    wd, rd, bd = w.cuda().contiguous(), _dev(rows), _dev(begin)
    for C in (1, 4):
        d_out = rng.standard_normal((P, C)).astype(np.float32)
        ref = RT.blend_bwd(w, slot, begin, d_out, total, hard).numpy()
        got = ops.cells_blend_bwd(wd, rd, bd, _dev(d_out), total, hard)
        assert tuple(got.shape) == (total, C)
        np.testing.assert_array_equal(got.cpu().numpy(), ref)
        again = ops.cells_blend_bwd(wd, rd, bd, _dev(d_out), total, hard)
        assert torch.equal(got, again)


@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("K", [1, 3, 64])
@pytest.mark.parametrize("P", [1, 255, 256, 257, 1000])
def test_cells_blend_bwd_vs_autograd(P, K, margin):
    w, counts, begin, rows, slot, rng = _case(7000 + 100 * K + P + int(margin), P, K, margin)
    if margin == 1:
        assert begin[-1] == P
    if margin == 1e6:
        assert begin[-1] == P * K           # every point belongs to every cell
    _check(w, begin, rows, slot, rng, margin)


@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("empty", [0, 2, 4])
def test_cells_blend_bwd_empty_cell(empty, margin):
    """A cell without members at the first, a middle and the last index: begin repeats there and the bisection must never land on it."""
    w, counts, begin, rows, slot, rng = _case(7100 + empty, 1000, 5, margin, far=(empty,))
    assert counts[empty] == 0 and begin[empty] == begin[empty + 1] and (np.delete(counts, empty) > 0).all()
    _check(w, begin, rows, slot, rng, margin)


@pytest.mark.parametrize("margin", [1.0, 1.15])
@pytest.mark.parametrize("C", [1, 4])
def test_cells_blend_bwd_writes_its_rows_only(C, margin):
    """A d_sub buffer longer than total, filled with a canary: the first total rows are the result, the tail is untouched.  total == 0
    launches nothing."""
    from switch_nerf_amd import _lib, ops
    P, K, extra = 257, 3, 300
    w, counts, begin, rows, slot, rng = _case(7200 + C, P, K, margin)
    total, hard = int(begin[-1]), margin == 1
    d_out = rng.standard_normal((P, C)).astype(np.float32)
    ref = RT.blend_bwd(w, slot, begin, d_out, total, hard).numpy()
    canary = np.float32(-12345.5)
    buf = torch.full((total + extra, C), float(canary), device="cuda")
    args = [ops._p(t) for t in (w.cuda().contiguous(), _dev(rows), _dev(begin), _dev(d_out))]
    _lib.call("swn_cells_blend_bwd", *args, total, P, K, C, 1 if hard else 0, ops._p(buf), ops._stream())
    got = buf.cpu().numpy()
    np.testing.assert_array_equal(got[:total], ref)
    assert (got[total:] == canary).all()
    buf.fill_(float(canary))
    _lib.call("swn_cells_blend_bwd", *args, 0, P, K, C, 1 if hard else 0, ops._p(buf), ops._stream())
    assert (buf.cpu().numpy() == canary).all()
    assert tuple(ops.cells_blend_bwd(w.cuda().contiguous(), _dev(rows), _dev(begin), _dev(d_out), 0, hard).shape) == (0, C)


def test_cells_blend_bwd_error_returns():
    from switch_nerf_amd import _lib, ops
    P = 63
    d4 = torch.zeros(P, 4, device="cuda")
    rows = torch.zeros(P, dtype=torch.int32, device="cuda")
    for K in (0, 65):
        with pytest.raises(RuntimeError, match=rf"n_cells {K} outside \[1, 64\]"):
            ops.cells_blend_bwd(torch.zeros(P, K, device="cuda"), rows, torch.zeros(K + 1, dtype=torch.int32, device="cuda"), d4, P, False)
    w, begin = torch.zeros(P, 3, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    for C in (2, 3, 5):
        with pytest.raises(RuntimeError, match=rf"channels {C} is neither 1 nor 4"):
            ops.cells_blend_bwd(w, rows, begin, torch.zeros(P, C, device="cuda"), P, False)
    good = [w, rows, begin, d4]
    out = torch.zeros(P, 4, device="cuda")
    for hard, missing in ((0, (0, 1, 2, 3, 4)), (1, (1, 3, 4))):      # (the hard copy reads neither the weights nor begin)
        for k in missing:
            ptrs = [ops._p(t) for t in good] + [ops._p(out)]
            ptrs[k] = None
            with pytest.raises(RuntimeError, match="swn_cells_blend_bwd: null pointer"):
                _lib.call("swn_cells_blend_bwd", *ptrs[:4], P, P, 3, 4, hard, ptrs[4], ops._stream())
