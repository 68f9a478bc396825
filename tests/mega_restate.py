"""Pure-torch restatement of the spatial-cell router of the Mega-NeRF model (the reference's models/mega_nerf.py:19-61), with DIRECT
distances: d = sqrt((x0 - c0)^2 + (x1 - c1)^2 + (x2 - c2)^2) added left to right over the coordinates j >= dim_start, where the reference's
torch.cdist switches to the |x|^2 + |c|^2 - 2 x.c matmul form above 25 rows and carries its cancellation error.  In float32 it runs the
operations of csrc/cells.hip in the same order (tests/test_mega_kernels_gpu.py compares bits where an order is decided); in float64 it
is the yardstick the fixtures' error figures are measured against (scripts/gen_golden_mega.py).  tests/test_mega_cpu.py pins it on the
reference's own results."""
import numpy as np
import torch


def distances(x, centroids, dim_start=0, dtype=torch.float32):
    """[P, K] direct distances of x[:, :3] to the centroids over the coordinates dim_start .. 2."""
    x = torch.as_tensor(x)[:, :3].to(dtype)
    c = torch.as_tensor(centroids).to(dtype)
    s = None
    for j in range(dim_start, 3):
        d = x[:, j:j + 1] - c[None, :, j]
        s = d * d if s is None else s + d * d
    return torch.sqrt(s)


def assign(x, centroids, dim_start, margin, dtype=torch.float32):
    """weights [P, K]: margin == 1 the one-hot of the first nearest cell; margin > 1 mega_nerf.py:21-27 (1 / (d + 1e-8), zero where
    d > margin * d_min, over its row sum taken in ascending cell order).  A member is a cell of weight > 0."""
    d = distances(x, centroids, dim_start, dtype)
    if margin == 1:
        w = torch.zeros_like(d)
        w[torch.arange(d.shape[0]), d.argmin(dim=1)] = 1          # (argmin: the first index of the minimum)
        return w
    inv = 1 / (d + torch.tensor(1e-8, dtype=dtype))
    dmin = d.min(dim=1, keepdim=True)[0]
    inv[d > torch.tensor(margin, dtype=dtype) * dmin] = 0
    s = torch.zeros(d.shape[0], dtype=dtype)
    for i in range(d.shape[1]):
        s = s + inv[:, i]
    return inv / s[:, None]


def boundary_gap(x, centroids, dim_start, margin):
    """[P] float64: how far (in distance) every point is from the nearest membership decision: the gap between its two nearest
    cells (margin == 1), or min_i |d_i - margin d_min| (margin > 1)."""
    d = distances(x, centroids, dim_start, torch.float64)
    if d.shape[1] == 1:
        return torch.full((d.shape[0],), float("inf"), dtype=torch.float64)
    if margin == 1:
        two = torch.topk(d, 2, dim=1, largest=False)[0]
        return two[:, 1] - two[:, 0]
    dmin, imin = d.min(dim=1, keepdim=True)
    gap = (d - margin * dmin).abs()
    gap.scatter_(1, imin, float("inf"))                            # (the nearest cell is a member on either side)
    return gap.min(dim=1)[0]


def pack(weights):
    """counts [K], begin [K + 1], rows [total] (point indices by cell, ascending inside a cell: the order of x[cluster_mask]),
    slot [P, K] (row inside the cell, or -1) as int32 numpy arrays."""
    m = (torch.as_tensor(weights) > 0).numpy()
    P, K = m.shape
    counts = m.sum(0).astype(np.int32)
    begin = np.zeros(K + 1, np.int32)
    begin[1:] = np.cumsum(counts)
    rows = np.concatenate([np.nonzero(m[:, i])[0] for i in range(K)]).astype(np.int32)
    slot = np.where(m, np.cumsum(m, 0) - 1, -1).astype(np.int32)
    return counts, begin, rows, slot


def gather(x, rows, col0=0, sigma_noise=None):
    x = torch.as_tensor(x)
    idx = torch.as_tensor(rows).long()
    return x[idx, col0:], (None if sigma_noise is None else torch.as_tensor(sigma_noise).reshape(-1)[idx])


def blend(weights, slot, begin, sub_out, hard):
    """out [P, C]: the reference's loop (mega_nerf.py:34-49) on packed per-cell outputs sub_out [total, C]."""
    w = torch.as_tensor(weights)
    sub = torch.as_tensor(sub_out).to(w.dtype)
    slot, begin = torch.as_tensor(slot).long(), torch.as_tensor(begin).long()
    out = torch.zeros(w.shape[0], sub.shape[1], dtype=w.dtype)
    for i in range(w.shape[1]):
        mask = slot[:, i] >= 0
        r = sub[begin[i] + slot[mask, i]]
        if hard:
            out[mask] = r
        else:
            out[mask] += r * w[mask, i].unsqueeze(-1)
    return out
