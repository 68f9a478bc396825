"""The backward of the Mega-NeRF cell blend, restated: torch's autograd through tests/mega_restate.blend (the reference's loop,
mega_nerf.py:34-49, on packed per-cell outputs) with respect to those outputs.  What swn_cells_blend_bwd is compared against
(tests/test_mega_train_kernels_gpu.py); mega_restate.py itself is untouched."""
import torch

import mega_restate as R


def blend_bwd(weights, slot, begin, d_out, total, hard):
    """d_sub [total, C] = d(sum(blend(weights, slot, begin, sub, hard) * d_out)) / d sub, float32 on the CPU.  Every packed row enters
    exactly one output row with one factor (1 for hard), so each element is one copy or one float32 product: no sum, no rounding choice."""
    d_out = torch.as_tensor(d_out)
    sub = torch.zeros(int(total), d_out.shape[1], dtype=torch.float32, requires_grad=True)
    out = R.blend(torch.as_tensor(weights), slot, begin, sub, hard)
    out.backward(d_out)
    return sub.grad
