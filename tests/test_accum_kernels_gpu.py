"""swn_grad_accum / swn_adam_accum_step (csrc/accum.hip) against their contract, bit for bit: acc + grad * scale as two separately
rounded fp32 operations, and the fused last micro-step = swn_grad_accum followed by swn_adam_step on the buffer, which leaves cleared.
Sizes: below one 16-byte piece, around one block, a ragged tail, and one past the block cap (4096 blocks x 256 threads x 4 floats), which
forces the grid-stride loop; every size also from a pointer offset by one float (the unaligned head)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 255, 256, 257, 1027, 4096 * 256 * 4 + 5]
SCALES = [1.0, 0.5, 1.0 / 3.0]
PAD = 8           # guard elements on either side of [0, n)
SPECIAL = [0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -3e-39, float("inf"), -float("inf"), float("nan"), 3.4028235e38, -3.4028235e38, 1.0]


@pytest.fixture(autouse=True)
def _bf16_build():
    from switch_nerf_amd import _lib
    _lib.use_half("bf16")            # the shadow below is bfloat16


@functools.lru_cache(maxsize=None)
def _inputs(n):
    """(acc, grad) on the CPU: normal values with signed zeros, denormals, inf, nan and the largest finite value at fixed places."""
    g = torch.Generator().manual_seed(1000 + n % 997)
    acc, grad = torch.randn(n, generator=g), torch.randn(n, generator=g) * 3.0
    sp = torch.tensor(SPECIAL)
    k = min(n, len(SPECIAL))
    acc[:k] = sp[:k]                                # special + normal
    if n > 2 * len(SPECIAL):
        grad[len(SPECIAL):2 * len(SPECIAL)] = sp    # normal + special
        acc[-len(SPECIAL):] = sp                    # special + special (inf - inf, 0 * inf among them), in the tail
        grad[-len(SPECIAL):] = sp.flip(0)
    return acc, grad


def _guarded(t, offset, fill):
    """t inside a buffer with PAD guard elements on either side, starting `offset` floats past a 16-byte boundary -> (buffer, view)."""
    buf = torch.full((offset + 2 * PAD + t.numel() + 4,), fill, dtype=t.dtype, device="cuda")
    view = buf[offset + PAD: offset + PAD + t.numel()]
    view.copy_(t)
    return buf, view


def _guards_intact(buf, view, offset, fill):
    n = view.numel()
    lo, hi = buf[: offset + PAD], buf[offset + PAD + n:]
    return bool((lo == fill).all() and (hi == fill).all())


def _same(a, b):
    """Bitwise-equal values, nan positions compared as positions (a nan's payload is not part of the contract)."""
    a, b = a.cpu(), b.cpu()
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(torch.where(na, torch.zeros_like(a), a).view(torch.int32),
                                               torch.where(nb, torch.zeros_like(b), b).view(torch.int32))


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_grad_accum_is_fp32_add_of_product(n, offset):
    from switch_nerf_amd import ops
    acc0, grad = _inputs(n)
    for scale in SCALES:
        ref = acc0 + grad * torch.tensor(scale, dtype=torch.float32)             # two fp32 operations, no FMA
        abuf, acc = _guarded(acc0, offset, 7.0)
        gbuf, g = _guarded(grad, offset, 9.0)
        ops.grad_accum(acc, g, scale)
        torch.cuda.synchronize()
        assert _same(acc, ref), (n, offset, scale)
        assert _same(g, grad) and _guards_intact(abuf, acc, offset, 7.0) and _guards_intact(gbuf, g, offset, 9.0)


def test_grad_accum_mixed_alignment():
    """Buffers whose offsets inside a 16-byte line differ take the element-by-element path: same bits."""
    from switch_nerf_amd import ops
    acc0, grad = _inputs(1027)
    abuf, acc = _guarded(acc0, 1, 7.0)
    gbuf, g = _guarded(grad, 2, 9.0)
    ops.grad_accum(acc, g, 1.0 / 3.0)
    assert _same(acc, acc0 + grad * torch.tensor(1.0 / 3.0, dtype=torch.float32))
    assert _guards_intact(abuf, acc, 1, 7.0) and _guards_intact(gbuf, g, 2, 9.0)


def _adam_state(n):
    g = torch.Generator().manual_seed(77 + n % 991)
    p = torch.randn(n, generator=g)
    m = torch.randn(n, generator=g) * 1e-2
    v = torch.rand(n, generator=g) * 1e-3
    return p, m, v


@pytest.mark.parametrize("with_grad", [True, False])
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_adam_accum_step_equals_accum_then_adam(n, offset, with_grad):
    from switch_nerf_amd import ops
    acc0, grad = _inputs(n)
    p0, m0, v0 = _adam_state(n)
    for scale, gscale, step in zip(SCALES, (1.0, 0.25, 1.0 / 65536.0), (1, 2, 7)):
        # the two-launch form
        _, acc_r = _guarded(acc0, offset, 7.0)
        _, g_r = _guarded(grad, offset, 9.0)
        p_r, m_r, v_r = (_guarded(t, offset, 5.0)[1] for t in (p0, m0, v0))
        sh_r = torch.zeros(n + 2, dtype=torch.bfloat16, device="cuda")[offset: offset + n]
        if with_grad:
            ops.grad_accum(acc_r, g_r, scale)
        ops.adam_step(p_r, acc_r, m_r, v_r, sh_r, step, 5e-4, grad_scale=gscale)
        # the fused form
        abuf, acc = _guarded(acc0, offset, 7.0)
        gbuf, g = _guarded(grad, offset, 9.0)
        (pbuf, p), (mbuf, m), (vbuf, v) = (_guarded(t, offset, 5.0) for t in (p0, m0, v0))
        shbuf = torch.full((n + 2 * PAD + 2,), 3.0, dtype=torch.bfloat16, device="cuda")
        sh = shbuf[PAD + offset: PAD + offset + n]
        ops.adam_accum_step(p, acc, g if with_grad else None, m, v, sh, step, 5e-4, accum_scale=scale, grad_scale=gscale)
        torch.cuda.synchronize()
        what = (n, offset, with_grad, scale)
        assert _same(p, p_r) and _same(m, m_r) and _same(v, v_r), what
        assert _same(sh.float(), sh_r.float()), what
        assert bool((acc == 0).all()) and not bool(torch.signbit(acc).any()), what              # cleared for the next window
        assert _same(g, grad), what
        for buf, view, fill in ((abuf, acc, 7.0), (gbuf, g, 9.0), (pbuf, p, 5.0), (mbuf, m, 5.0), (vbuf, v, 5.0)):
            assert _guards_intact(buf, view, offset, fill), what
        assert bool((shbuf[: PAD + offset] == 3.0).all() and (shbuf[PAD + offset + n:] == 3.0).all()), what


def test_adam_accum_step_fp32_shadow_and_no_shadow():
    from switch_nerf_amd import ops
    n = 1027
    acc0, grad = _inputs(n)
    p0, m0, v0 = _adam_state(n)
    dev = lambda *ts: [t.clone().cuda() for t in ts]
    acc_r, g_r, p_r, m_r, v_r = dev(acc0, grad, p0, m0, v0)
    ops.grad_accum(acc_r, g_r, 0.5)
    ops.adam_step(p_r, acc_r, m_r, v_r, None, 3, 5e-4)
    for shadow in (None, torch.zeros(n, device="cuda")):
        acc, g, p, m, v = dev(acc0, grad, p0, m0, v0)
        ops.adam_accum_step(p, acc, g, m, v, shadow, 3, 5e-4, accum_scale=0.5)
        assert _same(p, p_r) and _same(m, m_r) and _same(v, v_r) and bool((acc == 0).all())
        if shadow is not None:
            assert _same(shadow, p_r)


def test_bad_arguments_are_refused_before_any_launch():
    from switch_nerf_amd import ops
    t = torch.zeros(8, device="cuda")
    with pytest.raises(RuntimeError, match="swn_adam_accum_step"):
        ops.adam_accum_step(t, t.clone(), None, t.clone(), t.clone(), None, 0, 5e-4)          # step 0
