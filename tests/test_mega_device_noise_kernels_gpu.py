"""swn_cells_gather_rng / swn_cells_gather_padded_rng (csrc/cells.hip): the cells' gathers with the sigma noise drawn at the packed row.
The draw of packed row r (point p = rows[r]) must be the bits swn_rng_fill writes for element ray_base * R + p, whatever the membership,
the row space or the cut of the batch; x_out must be the plain gathers' bytes.  7 rays x 5 rows (R and P odd), ray_base 3 (odd), three
cells of which one is empty, three points in two cells; padded capacities 16 (cell 2 overflows) and 3 (both non-empty cells overflow).
The float64 comparison uses the bound tests/test_device_noise_gpu.py derives for the normal fill from tests/philox_restate.py: 1e-5 x
scale absolute."""
import numpy as np
import pytest
import torch

import philox_restate as R

pytestmark = pytest.mark.gpu
SEED = 0x0123456789ABCDEF
STEP = 2
N, RPR, K, RAY_BASE = 7, 5, 3, 3
P = N * RPR


def _bits(t):
    return t.contiguous().view(torch.int32)


def _step():
    from switch_nerf_amd import ops
    return ops.rng_step_tensor(STEP, "cuda")


def _x(P_=P):
    g = torch.Generator().manual_seed(5)
    return torch.randn(P, 7, generator=g)[P - P_:].contiguous().cuda()          # (a cut batch keeps the LAST P_ points' values)


def _soft_membership(P_=P, first=0):
    """weights [P_, 3] of the points first .. first + P_ - 1: cell 0 holds p % 3 == 0, cell 1 nothing, cell 2 p % 3 != 0 and p % 15 == 0."""
    p = np.arange(first, first + P_)
    w = np.zeros((P_, K), np.float32)
    w[p % 3 == 0, 0] = 0.25
    w[(p % 3 != 0) | (p % 15 == 0), 2] = 0.75
    return w


def _hard_membership(P_=P, first=0):
    p = np.arange(first, first + P_)
    w = np.zeros((P_, K), np.float32)
    w[np.arange(P_), (p // 2) % 3] = 1.0
    return w


def _dev_membership(w):
    return torch.from_numpy(w).cuda(), torch.from_numpy((w > 0).sum(0).astype(np.int32)).cuda()


def _fill(stream_id, scale, n=P, ray_base=RAY_BASE):
    from switch_nerf_amd import ops
    return ops.rng_fill(n, ray_base * RPR, ops.RNG_NORMAL, SEED, _step(), stream_id, scale)


def _expect(fill, rows, n_points):
    """fill[rows] on real rows, +0.0 on the others -> (values f32, real mask)."""
    real = (rows >= 0) & (rows < n_points)
    return torch.where(real, fill[rows.clamp(0, n_points - 1).long()], torch.zeros_like(fill[:1])), real


def _check(noise, x_out, x_plain, rows, stream_id, scale, n_points=P, ray_base=RAY_BASE):
    exp, real = _expect(_fill(stream_id, scale, n_points, ray_base), rows, n_points)
    assert torch.equal(_bits(noise), _bits(exp))                               # bit for bit what rng_fill writes, gathered
    assert not _bits(noise)[~real].any()                                       # +0.0 (all bits clear) on padding / out-of-range rows
    assert torch.equal(_bits(x_out), _bits(x_plain))                           # the plain gather's bytes
    ref = R.normal(SEED, STEP, stream_id, ray_base * RPR, n_points, scale=scale)
    r = rows.cpu().numpy()
    ok = real.cpu().numpy()
    err = np.abs(noise.cpu().numpy().astype(np.float64)[ok] - ref[r[ok]]).max()
    print(f"stream {stream_id} scale {scale}: {int(ok.sum())} real rows of {r.size}, max abs err against float64 {err:.3e} (bound {1e-5 * scale:.1e})")
    assert err <= 1e-5 * scale, err


@pytest.mark.parametrize("stream_id,scale", [(1, 1.0), (3, 0.5)])
def test_drawn_noise_is_the_gathered_fill(stream_id, scale):
    from switch_nerf_amd import ops
    x, step = _x(), _step()
    w = _soft_membership()
    assert ((w > 0).sum(1) == 2).sum() == 3 and (w > 0).sum(0).tolist() == [12, 0, 26]
    weights, counts = _dev_membership(w)
    # compact
    begin, rows, slot = ops.cells_pack(weights, counts)
    total = int(counts.sum().item())
    assert total == 38
    x_plain, _ = ops.cells_gather(x, rows, total, 0, None)
    x_out, noise = ops.cells_gather_rng(x, rows, total, 0, SEED, step, stream_id, RPR, RAY_BASE, scale)
    assert (rows[:total] >= 0).all()
    _check(noise, x_out, x_plain, rows[:total], stream_id, scale)
    # compact, a hand-made row list with a negative and an out-of-range entry: both get +0 and read nothing
    odd = torch.tensor([4, -1, 34, P, 0, 4, 17], dtype=torch.int32, device="cuda")
    x_plain, _ = ops.cells_gather(x, odd, odd.numel(), 0, None)
    x_out, noise = ops.cells_gather_rng(x, odd, odd.numel(), 0, SEED, step, stream_id, RPR, RAY_BASE, scale)
    _check(noise, x_out, x_plain, odd, stream_id, scale)
    assert _bits(noise)[[1, 3]].tolist() == [0, 0] and _bits(noise)[0] == _bits(noise)[5]
    # padded
    cen = torch.tensor([[-0.5, -0.4, 0.1], [0.5, -0.3, -0.2], [0.0, 0.5, 0.3]], device="cuda")
    for cap, dropped in ((16, 10), (3, 9 + 23)):
        begin, rows, slot, overflow = ops.cells_pack_padded(weights, counts, cap)
        assert int(overflow.item()) == dropped and rows.numel() == K * cap
        x_plain, _ = ops.cells_gather_padded(x, rows, cen, cap, 0, None)
        x_out, noise = ops.cells_gather_padded_rng(x, rows, cen, cap, 0, SEED, step, stream_id, RPR, RAY_BASE, scale)
        assert int((rows < 0).sum().item()) == K * cap - (38 - dropped)
        _check(noise, x_out, x_plain, rows, stream_id, scale)
    assert int(step.item()) == STEP                                            # the gathers read the counter; only rng_advance moves it


def _by_point(rows, noise, n_points):
    """int32 bits [n_points] of each point's noise (-1 where the point has no row); every row of a point must hold the same bits."""
    rows, bits = rows.cpu().numpy(), _bits(noise).cpu().numpy()
    out = {}
    for r, b in zip(rows, bits):
        if r >= 0:
            assert out.setdefault(int(r), int(b)) == int(b), r
    return out


def test_noise_of_a_point_does_not_depend_on_membership_row_space_or_cut():
    from switch_nerf_amd import ops
    step = _step()
    cen = torch.zeros(K, 3, device="cuda")
    want = {p: int(b) for p, b in enumerate(_bits(_fill(1, 1.0)).cpu().numpy())}
    seen = []
    for first, member in ((0, _soft_membership), (0, _hard_membership), (3 * RPR, _soft_membership), (3 * RPR, _hard_membership)):
        P_ = P - first                                                         # first = 15: the first 3 rays cut off, ray_base raised by 3
        x = _x(P_)
        weights, counts = _dev_membership(member(P_, first))
        base = RAY_BASE + first // RPR
        begin, rows, slot = ops.cells_pack(weights, counts)
        total = int(counts.sum().item())
        _, noise = ops.cells_gather_rng(x, rows, total, 0, SEED, step, 1, RPR, base, 1.0)
        seen.append({p + first: b for p, b in _by_point(rows[:total], noise, P_).items()})
        begin, rows, slot, overflow = ops.cells_pack_padded(weights, counts, P)
        assert int(overflow.item()) == 0
        _, noise = ops.cells_gather_padded_rng(x, rows, cen, P, 0, SEED, step, 1, RPR, base, 1.0)
        seen.append({p + first: b for p, b in _by_point(rows, noise, P_).items()})
    for got in seen:
        assert len(got) >= P - 3 * RPR
        for p, b in got.items():
            assert b == want[p], p
    assert set(seen[0]) == set(range(P)) and set(seen[4]) == set(range(3 * RPR, P))
    # another stream, step or seed is another draw
    other = _bits(ops.rng_fill(P, RAY_BASE * RPR, ops.RNG_NORMAL, SEED, step, 3, 1.0)).cpu().numpy()
    assert not np.array_equal(other, np.array([want[p] for p in range(P)], other.dtype))
