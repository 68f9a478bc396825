"""The pieces of the hierarchical pass (rendering.py:236-268, :419-433) that every renderer shares - SwitchNeRF.hier_passes /
render_backward, BackgroundScene.forward and the MegaNeRF paths, whose passes run through their own cells and so stay inline there."""
from __future__ import annotations

import torch

from . import ops


def default_fine_u(lin, N: int, F: int, perturb: float, dev):
    """The u [N, F] of sample_pdf where the caller supplies none: det = (perturb == 0) -> linspace, else rand (rendering.py:605-609).
    lin: a model's _linspace (the tensor cached on the device: no host-to-device copy inside a step)."""
    return lin(F).expand(N, F).contiguous() if perturb == 0 else torch.rand(N, F, device=dev)


def merge_flipped(z_f, z_b, raw_f, raw_b, dreal_f, dreal_b):
    """The background's merge: the descending sort of the union (:421 descending=flip) = the ascending sort of the negated depths, and
    depth_real in the same order (:432-433) -> z_m, order, raw_m, dreal_m."""
    zneg, order, raw_m = ops.merge_samples((-z_f).contiguous(), (-z_b).contiguous(), raw_f, raw_b)
    return -zneg, order, raw_m, torch.gather(torch.cat([dreal_f, dreal_b], 1), 1, order.long())


def merged_bwd(out, d_rgb):
    """Backward of the merged compositing (out = {raw, z, order, z_fine}) -> dL/d raw of the fine and of the coarse pass."""
    F = out["z_fine"].shape[1]
    return ops.unmerge_grad(ops.composite_bwd(out["raw"], out["z"], d_rgb), out["order"], F, out["z"].shape[1] - F)
