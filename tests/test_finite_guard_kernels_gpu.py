"""The finite guard's kernels (csrc/finite_guard.hip, the guarded launches of csrc/accum.hip): the flag and its counter on hand-made
metric vectors, and the guarded Adam / accumulate-Adam launches against the unguarded ones, bit for bit, between canaries."""
import pytest
import torch

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
PAD = 8                                   # canary elements on both sides of every buffer
# 1 .. 257: one element, around the 64-lane wave and the 256-thread workgroup; 5003: not a multiple of 4 (the 16-byte pieces) or of 256
# (a workgroup's span per pass); 4096 * 256 * 4 + 77: past one pass of the capped grid (4096 workgroups of 256 threads, 4 elements each)
SHORT = [1, 63, 64, 65, 257, 5003]
LONG = 4096 * 256 * 4 + 77               # (runs once per kernel: plain buffers)
LENGTHS = SHORT + [LONG]


def _flags():
    return torch.ones(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")


@pytest.mark.parametrize("n,psnr", [(4, 3), (5, 4)])
def test_guard_flag_per_slot_and_counter(n, psnr):
    from switch_nerf_amd import ops
    ok, skipped = _flags()
    good = [0.25, 0.5, 0.75, 1.0, 21.5][:n]
    expect = 0

    def run(vec):
        ops.finite_guard(torch.tensor(vec, dtype=torch.float32, device="cuda"), psnr, ok, skipped)
        return int(ok.item())

    assert run(good) == 1 and int(skipped.item()) == 0
    for slot in range(n):
        for bad in (NAN, INF, -INF):
            vec = list(good)
            vec[slot] = bad
            want = 1 if (slot == psnr and bad == INF) else 0       # +inf is a psnr (photo loss 0); nothing else that is not finite passes
            assert run(vec) == want, (slot, bad)
            expect += 1 - want
            assert int(skipped.item()) == expect                   # accumulates over the calls
    assert run(good) == 1 and int(skipped.item()) == expect == 3 * n - 1
    # every slot bad at once; no counter given (several ranks count behind their all-reduce)
    ops.finite_guard(torch.full((n,), NAN, device="cuda"), psnr, ok, None)
    assert int(ok.item()) == 0 and int(skipped.item()) == expect
    with pytest.raises(RuntimeError, match="swn_finite_guard"):
        ops.finite_guard(torch.zeros(65, device="cuda"), 3, ok, skipped)
    with pytest.raises(RuntimeError, match="psnr slot"):
        ops.finite_guard(torch.zeros(4, device="cuda"), 4, ok, skipped)


def _buffers(n, seed, dtype):
    """-> dict of padded buffers (canary value 7.5 around [PAD, PAD + n)) with a realistic optimizer state."""
    g = torch.Generator().manual_seed(seed)
    def pad(x):
        full = torch.full((n + 2 * PAD,), 7.5, dtype=x.dtype)
        full[PAD:PAD + n] = x
        return full.cuda()
    b = dict(p=pad(torch.randn(n, generator=g)), g=pad(torch.randn(n, generator=g) * 1e-2), m=pad(torch.randn(n, generator=g) * 1e-3),
             v=pad(torch.rand(n, generator=g) * 1e-5), acc=pad(torch.randn(n, generator=g) * 1e-2))
    b["shadow"] = pad(torch.zeros(n)).to(dtype) if dtype is not None else None
    return b


def _inner(b):
    return {k: (None if t is None else t[PAD:-PAD]) for k, t in b.items()}


def _clone(b):
    return {k: (None if t is None else t.clone()) for k, t in b.items()}


def _assert_same(a, b, keys, what):
    for k in keys:
        if a[k] is not None:
            assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), (what, k)      # bits, padding included


def _state(step):
    return torch.tensor([step, 0], dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("n,shadow", [(n, sh) for n in SHORT for sh in (None, torch.float32, torch.bfloat16)] + [(LONG, None)])
def test_guarded_adam_step(n, shadow):
    from switch_nerf_amd import ops
    b0 = _buffers(n, n, shadow)
    ok, _ = _flags()
    for step in (0, 6, 20000):                       # the first step, a later one, one past the table's end (both corrections 1)
        ref, got, off = _clone(b0), _clone(b0), _clone(b0)
        r, g_, o = _inner(ref), _inner(got), _inner(off)
        ops.adam_step(r["p"], r["g"], r["m"], r["v"], r["shadow"], step + 1, 5e-4, grad_scale=0.5)
        st = _state(step)
        ok.fill_(1)
        ops.adam_step_guarded(g_["p"], g_["g"], g_["m"], g_["v"], g_["shadow"], st, ok, 5e-4, grad_scale=0.5)
        _assert_same(ref, got, ("p", "g", "m", "v", "shadow"), "ok=1")
        assert st.tolist() == [step + 1, 0]
        ok.fill_(0)
        st = _state(step)
        ops.adam_step_guarded(o["p"], o["g"], o["m"], o["v"], o["shadow"], st, ok, 5e-4, grad_scale=0.5)
        _assert_same(b0, off, ("p", "g", "m", "v", "shadow"), "ok=0")      # (an unguarded step leaves the gradient as it is, too)
        assert st.tolist() == [step, 0]


@pytest.mark.parametrize("n,with_grad,shadow,offset", [(n, wg, sh, off) for n in SHORT for wg in (True, False)
                                                       for sh, off in ((None, 0), (torch.bfloat16, 0), (None, 1))] + [(LONG, True, None, 0)])
def test_guarded_adam_accum_step(n, with_grad, shadow, offset):
    """offset 1: the buffers start one element past a 16-byte line (head elements in front of the 16-byte body)."""
    from switch_nerf_amd import ops
    b0 = _buffers(n + offset, 1000 + n, shadow)
    cut = lambda b: {k: (None if t is None else t[PAD + offset:-PAD]) for k, t in b.items()}
    ok, _ = _flags()
    ref, got, off = _clone(b0), _clone(b0), _clone(b0)
    r, g_, o = cut(ref), cut(got), cut(off)
    kw = dict(accum_scale=0.5, grad_scale=0.25)
    ops.adam_accum_step(r["p"], r["acc"], r["g"] if with_grad else None, r["m"], r["v"], r["shadow"], 4, 5e-4, **kw)
    st = _state(3)
    ops.adam_accum_step_guarded(g_["p"], g_["acc"], g_["g"] if with_grad else None, g_["m"], g_["v"], g_["shadow"], st, ok, 5e-4, **kw)
    _assert_same(ref, got, ("p", "g", "m", "v", "shadow", "acc"), "ok=1")
    assert st.tolist() == [4, 0] and not bool(g_["acc"].any())
    ok.fill_(0)
    st = _state(3)
    ops.adam_accum_step_guarded(o["p"], o["acc"], o["g"] if with_grad else None, o["m"], o["v"], o["shadow"], st, ok, 5e-4, **kw)
    _assert_same(b0, off, ("p", "g", "m", "v", "shadow"), "ok=0")
    _assert_same(ref, off, ("acc", "g"), "ok=0: what the unguarded step leaves")      # cleared inside [0, n), canaries intact
    assert st.tolist() == [3, 0]


@pytest.mark.parametrize("n", LENGTHS)
def test_guarded_grad_accum(n):
    from switch_nerf_amd import ops
    b0 = _buffers(n, 2000 + n, None)
    ok, _ = _flags()
    ref, got, off = _clone(b0), _clone(b0), _clone(b0)
    ops.grad_accum(_inner(ref)["acc"], _inner(ref)["g"], 0.5)
    ops.grad_accum_guarded(_inner(got)["acc"], _inner(got)["g"], 0.5, ok)
    _assert_same(ref, got, ("acc", "g"), "ok=1")
    ok.fill_(0)
    ops.grad_accum_guarded(_inner(off)["acc"], _inner(off)["g"], 0.5, ok)
    want = b0["acc"].clone()
    want[PAD:-PAD] = 0.0
    assert torch.equal(off["acc"], want) and torch.equal(off["g"], b0["g"])


def test_bias_table_shape_and_end():
    """Row t - 1 of the table against 1 - beta^t in the arithmetic of the entry point (fp32 powf / sqrtf of the host's libm, which
    numpy's float32 power does not promise to be): the table is checked through the kernels above; here its shape and its end."""
    from switch_nerf_amd import ops
    t = ops.adam_bias_table(torch.device("cuda"))
    assert t.dtype == torch.float32 and t.shape[1] == 2 and 17000 < t.shape[0] < 18000
    assert t[-1].tolist() == [1.0, 1.0] and t[-2].tolist() != [1.0, 1.0]
    import numpy as np
    one, b1, b2 = np.float32(1.0), np.float32(0.9), np.float32(0.999)          # step 1 in fp32: 1 - beta as the launch forms it
    assert abs(t[0, 0].item() - float(one - b1)) < 1e-7 and abs(t[0, 1].item() - float(np.sqrt(one - b2))) < 1e-7
    assert bool((t[1:] >= t[:-1]).all())
