"""swn_heads_sh_fwd / swn_heads_sh_bwd (csrc/sh.hip) against the fp64 restatement (tests/sh_restate.py, pinned on the reference in
tests/test_sh_cpu.py).

fp32 bounds: tests/golden/sh_heads_bounds.npz holds, for every case below, max |fp32 - fp64| of the reference formulation of the
heads (F.linear + eval_sh + sigmoid, softplus; backward by autograd) on the SAME inputs (scripts/gen_golden_sh.py); a kernel output
may be 8 x that far from fp64 (the convention of profiles/r11_topk_gate_kernel_parity.md).  16-bit builds: the restatement runs on the
inputs rounded to the 16-bit type, so all fp32 outputs keep the fp32 bounds; dh2 is STORED in the 16-bit type and gets half an ulp of
its value on top (bfloat16: 8 significand bits, spacing 2^-7 in [1, 2), half of it 2^-8 relative; half: 11 bits, 2^-11), its per-ray
column sums that times the rows of a ray.

d_bs (the gradient of the sigma bias) is ONE scalar summed over every point, signed terms that cancel; its reference figure is the error
of torch's cascade sum, e.g. 7.1e-07 at 300 x 96.  A plain fixed-order fp32 sum of the block partials sat at 8.8e-06 there, so the kernel
carries that sum as a compensated pair and forms its terms in double (csrc/sh.hip); profiles/r14_sh_colour.md has the figures."""
import os

import numpy as np
import pytest
import torch

import sh_restate as R
import sh_weights as SW

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
NAMES = ("rgb", "sigma", "coef", "dh2", "dsig", "d_ws", "d_bs", "d_wc", "d_bc", "colsum")
_BOUNDS = {}


def _bounds(case):
    if not _BOUNDS:
        g = np.load(os.path.join(G, "sh_heads_bounds.npz"))
        assert tuple(str(n) for n in g["names"]) == NAMES
        _BOUNDS.update({k: g[k] for k in g.files if k != "names"})
    return dict(zip(NAMES, 8.0 * _BOUNDS[SW.case_key(*case)]))


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _run(c, deg, rpg, dtype, want_coef=True):
    """One forward and one backward on the device -> dict of fp64 CPU tensors (and the raw device tensors for bitwise checks)."""
    from switch_nerf_amd import ops as o
    P, B = c["y"].shape[0], (deg + 1) ** 2
    y, h2 = _dev(c["y"], dtype), _dev(c["h2"], dtype)
    ws, bs, wc, bc, dirs = (_dev(c[k]) for k in ("ws", "bs", "wc", "bc", "dirs"))
    noise = None if c["noise"] is None else _dev(c["noise"])
    out = o.heads_sh_fwd(y, h2, ws, bs, wc, bc, noise, dirs, rpg, deg, want_coef=want_coef)
    raw, coef = out if want_coef else (out, None)
    acc = [torch.zeros(c["y"].shape[1], device=DEV), torch.zeros(1, device=DEV), torch.zeros(3 * B, c["h2"].shape[1], device=DEV),
           torch.zeros(3 * B, device=DEV)]
    dh2, dsig, cs = o.heads_sh_bwd(y, h2, wc, bc, dirs, raw, _dev(c["d_raw"]), *acc, rpg, deg)
    torch.cuda.synchronize()
    return dict(raw=raw, coef=coef, dh2=dh2, dsig=dsig, colsum=cs, d_ws=acc[0], d_bs=acc[1], d_wc=acc[2], d_bc=acc[3])


def _restate(c, deg, rpg, dtype):
    """fp64 on the inputs as the kernel sees them (activations rounded to the compute dtype)."""
    t = {k: (None if v is None else torch.from_numpy(v)) for k, v in c.items()}
    y, h2 = t["y"].to(dtype).double(), t["h2"].to(dtype).double()
    a = [t[k].double() for k in ("ws", "bs", "wc", "bc")]
    noise = None if t["noise"] is None else t["noise"].double()
    raw, lin = R.heads_fwd(y, h2, *a, noise, t["dirs"].double(), rpg, deg)
    b = R.heads_bwd(y, h2, *a, noise, t["dirs"].double(), rpg, deg, t["d_raw"].double())
    return dict(b, rgb=raw[:, :3], sigma=raw[:, 3], coef=lin)


def _check(case, dtype):
    deg, N, S, rpg, noise = case
    c = SW.head_case(*case)
    tol = _bounds(case)
    got = _run(c, deg, rpg, dtype)
    ref = _restate(c, deg, rpg, dtype)
    f = lambda t: t.detach().double().cpu()
    cmp = dict(rgb=f(got["raw"][:, :3]), sigma=f(got["raw"][:, 3]), coef=f(got["coef"]), dh2=f(got["dh2"]), dsig=f(got["dsig"]),
               d_ws=f(got["d_ws"]), d_bs=f(got["d_bs"])[0], d_wc=f(got["d_wc"]), d_bc=f(got["d_bc"]), colsum=f(got["colsum"]))
    half_ulp = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]
    extra = dict(dh2=half_ulp * float(ref["dh2"].abs().max()), colsum=half_ulp * rpg * float(ref["dh2"].abs().max()))
    for k in NAMES:
        err = float((cmp[k] - ref[k]).abs().max())
        bound = float(tol[k]) + extra.get(k, 0.0)
        print(f"{SW.case_key(*case)} {dtype} {k}: max |err| {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (k, err, bound)
    # d_raw is exactly zero on the last quarter of the rows: their dh2 is +0, bit for bit; the column sums see what was stored
    P = N * S
    z = got["dh2"][P - P // 4:]
    assert not z.view(torch.int32 if dtype == torch.float32 else torch.int16).any()
    # coef off: the same raw, bit for bit; a second run of both entry points: the same bits everywhere
    again = _run(c, deg, rpg, dtype, want_coef=False)
    assert again["coef"] is None
    for k in ("raw", "dh2", "dsig", "colsum", "d_ws", "d_bs", "d_wc", "d_bc"):
        assert torch.equal(again[k], got[k]), k
    third = _run(c, deg, rpg, dtype)
    assert torch.equal(third["coef"], got["coef"]) and torch.equal(third["raw"], got["raw"]) and torch.equal(third["d_wc"], got["d_wc"])


@pytest.mark.parametrize("case", SW.head_cases(), ids=lambda c: SW.case_key(*c))
def test_heads_sh_fp32_vs_fp64_restatement(case):
    """deg 0..4 (3 B = 3, 12, 27, 48, 75) on a single row, 65 rows, 192, 259 and 28800 rows, rows_per_group = S and 1, with and
    without sigma noise, non-unit directions, coef on and off, two runs."""
    _check(case, torch.float32)


HALF_CASES = [c for c in SW.head_cases() if (c[1], c[2]) in ((7, 37), (300, 96)) and c[3] != 1] + [(2, 5, 13, 1, True)]


@pytest.mark.parametrize("case", HALF_CASES, ids=lambda c: SW.case_key(*c))
def test_heads_sh_bf16(case):
    from switch_nerf_amd import _lib
    _lib.use_half("bf16")
    _check(case, torch.bfloat16)


@pytest.mark.parametrize("case", HALF_CASES, ids=lambda c: SW.case_key(*c))
def test_heads_sh_fp16(case):
    from switch_nerf_amd import _lib
    try:
        _lib.use_half("f16")
        _check(case, torch.float16)
    finally:
        _lib.use_half("bf16")


@pytest.mark.parametrize("deg", [1, 2, 4])
def test_rows_past_the_head_do_not_leak(deg):
    """The colour head handed over as the first 3 B rows of a larger buffer whose further rows hold 1e30 (and a large bias in the last
    real row): the same bits as with exactly-sized tensors - nothing past row 3 B - 1 is read into a result."""
    from switch_nerf_amd import ops as o
    case = (deg, 7, 37, 37, True)
    c = SW.head_case(*case)
    B = (deg + 1) ** 2
    c["bc"][-1] = 1000.0
    a = _run(c, deg, 37, torch.float32)
    y, h2 = _dev(c["y"]), _dev(c["h2"])
    wc_big = torch.full((3 * B + 8, c["h2"].shape[1]), 1e30, device=DEV)
    bc_big = torch.full((3 * B + 8,), 1e30, device=DEV)
    wc_big[: 3 * B], bc_big[: 3 * B] = _dev(c["wc"]), _dev(c["bc"])
    raw, coef = o.heads_sh_fwd(y, h2, _dev(c["ws"]), _dev(c["bs"]), wc_big[: 3 * B], bc_big[: 3 * B], _dev(c["noise"]), _dev(c["dirs"]), 37, deg,
                               want_coef=True)
    assert torch.equal(raw, a["raw"]) and torch.equal(coef, a["coef"]) and torch.isfinite(raw).all()
    acc = [torch.zeros(256, device=DEV), torch.zeros(1, device=DEV), torch.full((3 * B + 8, 128), 7.0, device=DEV), torch.full((3 * B + 8,), 7.0, device=DEV)]
    acc[2][: 3 * B], acc[3][: 3 * B] = 0, 0
    dh2, _, _ = o.heads_sh_bwd(y, h2, wc_big[: 3 * B], bc_big[: 3 * B], _dev(c["dirs"]), raw, _dev(c["d_raw"]), acc[0], acc[1], acc[2][: 3 * B],
                               acc[3][: 3 * B], 37, deg)
    assert torch.equal(dh2, a["dh2"]) and torch.equal(acc[2][: 3 * B], a["d_wc"]) and torch.equal(acc[3][: 3 * B], a["d_bc"])
    assert (acc[2][3 * B:] == 7.0).all() and (acc[3][3 * B:] == 7.0).all()          # the gradient rows behind the head are not written


def test_saturated_inputs():
    """|lin| ~ 40 and u > 20: finite, and within the forward error of an fp32 dot product of the contraction's |terms|
    (gamma_n = n 2^-24 with n = H2 + B + 2 operations per sum) pushed through the sigmoid's slope (<= 1 / 4) plus one rounding; where
    u > 20 the softplus returns u itself (models/nerf.py:68-69, threshold 20)."""
    deg, N, S = 3, 7, 37
    c = SW.head_case(deg, N, S, S, False)
    c["wc"] *= 60.0
    c["ws"] = np.abs(c["ws"]) * 8.0
    got = _run(c, deg, S, torch.float32)
    ref = _restate(c, deg, S, torch.float32)
    raw = got["raw"].double().cpu()
    assert torch.isfinite(raw).all() and float(ref["coef"].abs().max()) > 40 and int((ref["sigma"] > 20).sum()) > 10
    t = {k: torch.from_numpy(v).double() for k, v in c.items() if v is not None}
    B, H2, M = (deg + 1) ** 2, c["h2"].shape[1], c["y"].shape[1]
    Y = R.basis(deg, t["dirs"]).repeat_interleave(S, 0).abs()
    s_abs = ((t["h2"].abs() @ t["wc"].abs().t() + t["bc"].abs()).view(-1, 3, B) * Y[:, None, :]).sum(-1)
    bound_rgb = 0.25 * (H2 + B + 2) * 2.0 ** -24 * s_abs + 2.0 ** -23
    assert ((raw[:, :3] - ref["rgb"]).abs() <= bound_rgb).all()
    assert ((raw[:, :3] >= 0) & (raw[:, :3] <= 1)).all()
    u_abs = t["y"].abs() @ t["ws"].abs() + t["bs"].abs() + 1
    assert ((raw[:, 3] - ref["sigma"]).abs() <= (M + 3) * 2.0 ** -24 * u_abs + 2.0 ** -23 * ref["sigma"].abs()).all()
    for k in ("dh2", "d_wc", "d_ws", "colsum"):
        assert torch.isfinite(got[k].float()).all(), k


def test_entry_points_validate_before_launch():
    import ctypes as C
    from switch_nerf_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(0x1000)
    err = lambda: lib.swn_last_error().decode()
    assert lib.swn_heads_sh_fwd(p, p, _lib.F32, p, p, p, p, None, p, 7, 2, 100, 256, 128, p, None, None) != 0 and "rows_per_group" in err()
    assert lib.swn_heads_sh_fwd(p, p, _lib.F32, p, p, p, p, None, p, 10, 5, 100, 256, 128, p, None, None) != 0 and "deg" in err()
    assert lib.swn_heads_sh_fwd(p, p, _lib.F32, p, p, p, p, None, None, 10, 2, 100, 256, 128, p, None, None) != 0 and "null pointer" in err()
    assert lib.swn_heads_sh_fwd(p, p, _lib.F32, p, p, p, p, None, p, 10, 2, 100, 128, 64, p, None, None) != 0 and "model_dim" in err()
    nb = C.c_size_t(0)
    assert lib.swn_heads_sh_bwd_workspace_bytes(100, 256, 128, 10, 2, C.byref(nb)) == 0 and nb.value > 0
    args = [p, p, _lib.F32, p, p, p, p, p, 100, 256, 128, 10, 2, p, p, p, p, p, p, None, p]
    assert lib.swn_heads_sh_bwd(*args, nb.value - 4, None) != 0 and "workspace" in err()
