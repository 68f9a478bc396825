"""The kernels behind training Mega-NeRF cells with spherical-harmonics colour (csrc/sh.hip): swn_cells_blend_sh_bwd, swn_heads_coef_fwd,
swn_heads_coef_bwd, against a float64 torch evaluation of their formulas (include/swn.h):

    q_c[r] = w_r d_raw[p][c] raw[p][c] (1 - raw[p][c])   (deg 0: * s_c[r] (1 - s_c[r]))      q_3[r] = w_r d_raw[p][3]      p = rows[r]
    out[r] = (h2[r] Wc^T + bc, softplus(y[r] . ws + bs + noise[r] - 1))
    dh2[r] = (h2[r] > 0) sum_k g[r][k] Wc[k],  g[r][c B + b] = q_c[r] Y_b(dirs[r]);  d_Wc += g^T h2;  d_bc += sum_r g;  dsig = q_3 (1 - exp(-sigma))

The tolerance is the project's blend_sh_tol rule: 4 x the error of the SAME formula evaluated in float32 torch against float64 on the same
inputs (for a 16-bit output: both rounded to it).  None of it comes from the code under test."""
import ctypes as C

import numpy as np
import pytest
import torch

import mega_restate as R
import sh_restate as SR

pytestmark = pytest.mark.gpu
CANARY = -12345.5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _close(got, f32, f64, what):
    """|got - f64| <= 4 max|f32 - f64| elementwise."""
    got, f32, f64 = (t.detach().double().cpu() for t in (got, f32, f64))
    tol = 4 * float((f32 - f64).abs().max())
    err = float((got - f64).abs().max()) if got.numel() else 0.0
    print(f"{what}: err {err:.3e}, bound {tol:.3e}")
    assert got.shape == f64.shape and err <= tol, f"{what}: error {err:.3e} over 4 x the float32 formula's {tol / 4:.3e}"


# ------------------------------------------------------------------------------------------ swn_cells_blend_sh_bwd
def _blend_case(seed, P, K, margin, rpg, deg, far=()):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (P, 3)).astype(np.float32)
    cen = rng.uniform(-0.8, 0.8, (K, 3)).astype(np.float32)
    for i in far:
        cen[i] = (4e7, -4e7, 4e7)
    w = R.assign(x, cen, 0, margin)
    counts, begin, rows, slot = R.pack(w)
    total = int(begin[-1])
    f = lambda a: np.ascontiguousarray(a, np.float32)
    c = dict(w=w, begin=np.asarray(begin, np.int32), rows=np.asarray(rows, np.int32)[:total], total=total, counts=counts,
             raw=f(np.concatenate([rng.uniform(0.02, 0.98, (P, 3)), rng.uniform(0, 3, (P, 1))], 1)), d_raw=f(rng.standard_normal((P, 4))),
             dirs=f(rng.standard_normal((P // rpg, 3))), sub=f(rng.uniform(0.02, 0.98, (total, 4))) if deg == 0 else None)
    return c


def _blend_formula(c, rpg, deg, hard, dtype):
    """(q, dirs_packed) in torch at `dtype`, the products left to right."""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    rows = torch.from_numpy(c["rows"]).long()
    cell = torch.searchsorted(torch.from_numpy(c["begin"]).long()[1:], torch.arange(c["total"]), right=True)
    raw, d = t(c["raw"])[rows], t(c["d_raw"])[rows]
    q = d if hard else t(c["w"])[rows, cell][:, None] * d
    q = torch.cat([q[:, :3] * raw[:, :3] * (1 - raw[:, :3]), q[:, 3:]], 1)
    if deg == 0:
        s = t(c["sub"])[:, :3]
        q = torch.cat([q[:, :3] * s * (1 - s), q[:, 3:]], 1)
    return q, t(c["dirs"])[rows // rpg]


def _blend_run(c, rpg, deg, hard, total=None):
    from switch_nerf_amd import ops
    return ops.cells_blend_sh_bwd(c["w"].cuda().contiguous(), _dev(c["rows"]) if c["total"] else torch.zeros(1, dtype=torch.int32, device="cuda"),
                                  _dev(c["begin"]), _dev(c["raw"]), _dev(c["d_raw"]), _dev(c["dirs"]), rpg, deg,
                                  c["total"] if total is None else total, hard, None if c["sub"] is None else _dev(c["sub"]))


@pytest.mark.parametrize("margin", [1.0, 1.15])
@pytest.mark.parametrize("K", [1, 3, 17, 64])
@pytest.mark.parametrize("P", [1, 63, 65, 197])
def test_cells_blend_sh_bwd_vs_float64(P, K, margin):
    """Every degree, rows_per_group 1 and (where it divides P) 5 - rays that straddle the 64-point tiles; 17 cells cross the 16-cell lane
    group of the forward, 64 is the cap.  Two runs are bit-equal."""
    for deg in range(5):
        for rpg in (1, 5):
            if P % rpg:
                continue
            c = _blend_case(9000 + 1000 * deg + 10 * K + P + rpg, P, K, margin, rpg, deg)
            hard = margin == 1
            q, dp = _blend_run(c, rpg, deg, hard)
            (q32, dp32), (q64, dp64) = (_blend_formula(c, rpg, deg, hard, dt) for dt in (torch.float32, torch.float64))
            _close(q, q32, q64, f"q P{P} K{K} m{margin} d{deg} g{rpg}")
            assert torch.equal(dp.cpu(), dp32)          # (a copy)
            q2, dp2 = _blend_run(c, rpg, deg, hard)
            assert torch.equal(q, q2) and torch.equal(dp, dp2)


@pytest.mark.parametrize("margin", [1.0, 1.15])
@pytest.mark.parametrize("empty", [0, 2, 4])
def test_cells_blend_sh_bwd_cells_without_a_member(empty, margin):
    for deg in (0, 3):
        c = _blend_case(9100 + empty + deg, 195, 5, margin, 5, deg, far=(empty,))
        assert c["counts"][empty] == 0 and c["begin"][empty] == c["begin"][empty + 1]
        q, dp = _blend_run(c, 5, deg, margin == 1)
        (q32, dp32), (q64, _) = (_blend_formula(c, 5, deg, margin == 1, dt) for dt in (torch.float32, torch.float64))
        _close(q, q32, q64, f"q empty {empty} m{margin} d{deg}")
        assert torch.equal(dp.cpu(), dp32)


@pytest.mark.parametrize("deg", [0, 2])
def test_cells_blend_sh_bwd_writes_its_rows_only_and_returns_errors(deg):
    from switch_nerf_amd import _lib, ops
    P, K, rpg, extra = 195, 3, 5, 70
    c = _blend_case(9200 + deg, P, K, 1.15, rpg, deg)
    total = c["total"]
    qb, db = torch.full((total + extra, 4), CANARY, device="cuda"), torch.full((total + extra, 3), CANARY, device="cuda")
    good = [c["w"].cuda().contiguous(), _dev(c["rows"]), _dev(c["begin"]), _dev(c["raw"]), _dev(c["d_raw"]), _dev(c["dirs"]),
            None if c["sub"] is None else _dev(c["sub"])]
    lib = _lib.load()

    def run(ptrs, total_, rpg_, deg_, P_, K_, hard_, qp, dpp):
        return lib.swn_cells_blend_sh_bwd(*ptrs, total_, rpg_, deg_, P_, K_, hard_, qp, dpp, ops._stream())
    ptrs = [ops._p(t) for t in good]
    assert run(ptrs, total, rpg, deg, P, K, 0, ops._p(qb), ops._p(db)) == 0
    ref_q, ref_d = ops.cells_blend_sh_bwd(*good[:6], rpg, deg, total, False, good[6])
    assert torch.equal(qb[:total], ref_q) and torch.equal(db[:total], ref_d)
    assert (qb[total:] == CANARY).all() and (db[total:] == CANARY).all()
    qb.fill_(CANARY), db.fill_(CANARY)
    assert run(ptrs, 0, rpg, deg, P, K, 0, ops._p(qb), ops._p(db)) == 0          # total == 0: nothing is launched
    assert (qb == CANARY).all() and (db == CANARY).all()
    # errors: each returns non-zero and writes nothing
    for K_ in (0, 65):
        assert run(ptrs, total, rpg, deg, P, K_, 0, ops._p(qb), ops._p(db)) != 0
    for deg_ in (-1, 5):
        assert run(ptrs, total, rpg, deg_, P, K, 0, ops._p(qb), ops._p(db)) != 0
    for rpg_ in (0, -1, 2, 7):          # (< 1, or not dividing 195)
        assert run(ptrs, total, rpg_, deg, P, K, 0, ops._p(qb), ops._p(db)) != 0
    for hard_, missing in ((0, (0, 1, 2, 3, 4, 5)), (1, (1, 3, 4, 5))):      # (the hard form reads neither the weights nor begin)
        for k in missing:
            bad = list(ptrs)
            bad[k] = None
            assert run(bad, total, rpg, deg, P, K, hard_, ops._p(qb), ops._p(db)) != 0, k
    if deg == 0:
        assert run(ptrs[:6] + [None], total, rpg, deg, P, K, 0, ops._p(qb), ops._p(db)) != 0      # (sub_out is read at degree 0)
    else:
        assert ptrs[6] is None          # (... and may be NULL otherwise: the run above)
    assert run(ptrs, total, rpg, deg, P, K, 0, None, ops._p(db)) != 0 and run(ptrs, total, rpg, deg, P, K, 0, ops._p(qb), None) != 0
    torch.cuda.synchronize()
    assert (qb == CANARY).all() and (db == CANARY).all()


# ------------------------------------------------------------------------------------------ the head kernels
NS = (1, 15, 17, 255, 257, 1000)
PAIRS = ((256, 128), (512, 256))


def _head_case(seed, n, M, H2, deg, dtype):
    rng = np.random.default_rng(seed)
    B = (deg + 1) ** 2
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    d = rng.standard_normal((n, 3))
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (n, 1))
    c = dict(y=f(np.maximum(rng.standard_normal((n, M)), 0)).to(dtype), h2=f(np.maximum(rng.standard_normal((n, H2)), 0)).to(dtype),
             ws=f(rng.uniform(-1, 1, M) / 16), bs=f(rng.uniform(-1, 1, 1)), wc=f(rng.uniform(-1, 1, (3 * B, H2)) / 8),
             bc=f(rng.uniform(-1, 1, 3 * B)), noise=f(rng.standard_normal(n)), dirs=f(d), q=f(rng.standard_normal((n, 4))))
    c["q"][n - n // 4:] = 0          # (a zero suffix: +0 rows in dh2)
    return c


def _fwd_formula(c, deg, inner, dtype, noise=True):
    t = lambda a: a.to(dtype)
    lin = t(c["h2"]) @ t(c["wc"]).t() + t(c["bc"])
    if inner:
        lin = torch.sigmoid(lin)
    u = t(c["y"]) @ t(c["ws"]) + t(c["bs"]) + (t(c["noise"]) if noise else 0) - 1
    return torch.cat([lin, torch.nn.functional.softplus(u, threshold=20.0)[:, None]], 1)


def _bwd_formula(c, sig, deg, dtype, out_dtype, pre):
    """(dh2, dsig, colsum, d_ws, d_bs, d_wc, d_bc) at `dtype`; dh2 rounded to the output type, the gradients added to `pre`."""
    t = lambda a: a.to(dtype)
    B = (deg + 1) ** 2
    Y = SR.basis(deg, t(c["dirs"]))
    g = (t(c["q"])[:, :3, None] * Y[:, None, :]).reshape(-1, 3 * B)
    h2, y = t(c["h2"]), t(c["y"])
    dh2 = ((g @ t(c["wc"])) * (h2 > 0)).to(out_dtype)
    dsig = t(c["q"])[:, 3] * (1 - torch.exp(-t(sig)))
    return (dh2, dsig, dh2.to(dtype), t(pre[0]) + dsig @ y, t(pre[1]) + dsig.sum(0, keepdim=True), t(pre[2]) + g.t() @ h2,
            t(pre[3]) + g.sum(0))


@pytest.mark.parametrize("deg", [0, 2, 4])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,H2", PAIRS)
def test_heads_coef_fwd_vs_float64(M, H2, dtype, deg):
    """Every row count (one row, around the 16-lane group, around a block, several tiles with a ragged last one), with and without sigma
    noise, at degree 0 with and without the inner sigmoid; rows past n and the columns between 3 B + 1 and the row stride are untouched;
    two runs are bit-equal; the inner sigmoid agrees with torch.sigmoid on the existing forward's coef output."""
    from switch_nerf_amd import ops
    B = (deg + 1) ** 2
    for n in NS:
        c = _head_case(9300 + 10 * deg + n + M, n, M, H2, deg, dtype)
        d = {k: v.cuda() for k, v in c.items()}
        for inner in ((False, True) if deg == 0 else (False,)):
            for noise in (True, False):
                buf = torch.full((n + 3, 3 * B + 4), CANARY, device="cuda")      # a strided view: row stride 3 B + 4
                out = buf[:n, :3 * B + 1]
                ops.heads_coef_fwd(d["y"], d["h2"], d["ws"], d["bs"], d["wc"], d["bc"], d["noise"] if noise else None, deg, out, inner)
                f32, f64 = (_fwd_formula(c, deg, inner, dt, noise) for dt in (torch.float32, torch.float64))
                _close(out, f32, f64, f"coef fwd n{n} ({M},{H2}) {dtype} d{deg} inner{int(inner)} noise{int(noise)}")
                assert (buf[n:] == CANARY).all() and (buf[:, 3 * B + 1:] == CANARY).all()
                buf2 = torch.full((n + 3, 3 * B + 4), CANARY, device="cuda")
                ops.heads_coef_fwd(d["y"], d["h2"], d["ws"], d["bs"], d["wc"], d["bc"], d["noise"] if noise else None, deg, buf2[:n, :3 * B + 1], inner)
                assert torch.equal(buf, buf2)
        # against the existing forward's coef output (the folded kernel's per-point side output) and its sigma
        raw, coef = ops.heads_sh_fwd(d["y"], d["h2"], d["ws"], d["bs"], d["wc"], d["bc"], d["noise"], d["dirs"], 1, deg, want_coef=True)
        packed = torch.empty(n, 3 * B + 1, device="cuda")
        ops.heads_coef_fwd(d["y"], d["h2"], d["ws"], d["bs"], d["wc"], d["bc"], d["noise"], deg, packed, deg == 0)
        f32, f64 = (_fwd_formula(c, deg, deg == 0, dt) for dt in (torch.float32, torch.float64))
        old = torch.cat([torch.sigmoid(coef) if deg == 0 else coef, raw[:, 3:]], 1)
        assert float((packed - old).abs().max()) <= 4 * float((f32.double() - f64).abs().max())


@pytest.mark.parametrize("deg", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,H2", PAIRS)
def test_heads_coef_bwd_vs_float64(M, H2, dtype, deg):
    """dh2 (masked by h2 > 0), dsig, group_colsum and the four parameter gradients ACCUMULATED into buffers pre-filled with non-zero values;
    the sigma output is read through the row stride of a packed row.  Two runs are bit-equal."""
    from switch_nerf_amd import ops
    B = (deg + 1) ** 2
    for n in NS:
        c = _head_case(9500 + 10 * deg + n + M, n, M, H2, deg, dtype)
        d = {k: v.cuda() for k, v in c.items()}
        rng = np.random.default_rng(n + deg)
        rows_out = torch.from_numpy(rng.uniform(0, 3, (n, 3 * B + 1)).astype(np.float32))
        sig = rows_out[:, 3 * B].clone()
        pre = [torch.from_numpy(rng.standard_normal(s).astype(np.float32)) for s in ((M,), (1,), (3 * B, H2), (3 * B,))]
        runs = []
        for _ in range(2):
            g = [p.clone().cuda() for p in pre]
            res = ops.heads_coef_bwd(d["y"], d["h2"], d["wc"], d["q"], d["dirs"], rows_out.cuda(), g[0], g[1], g[2], g[3], deg)
            runs.append(list(res) + g)
        for a, b in zip(*runs):
            assert torch.equal(a, b)
        f32, f64 = (_bwd_formula(c, sig, deg, dt, dtype, pre) for dt in (torch.float32, torch.float64))
        for name, got, a, b in zip(("dh2", "dsig", "colsum", "d_w_sigma", "d_b_sigma", "d_w_color", "d_b_color"), runs[0], f32, f64):
            _close(got, a, b, f"coef bwd {name} n{n} ({M},{H2}) {dtype} d{deg}")
        dh2 = runs[0][0].float().cpu()
        assert not (dh2[c["h2"].float() <= 0] != 0).any()
        assert not torch.signbit(dh2[n - n // 4:]).any()          # (zero gradient rows leave +0)
        assert torch.equal(runs[0][2].cpu(), dh2)                  # (group_colsum at one row per group: the stored dh2 row)


def test_heads_coef_kernels_write_their_rows_only_and_return_errors():
    from switch_nerf_amd import _lib, ops
    lib = _lib.load()
    n, M, H2, deg, extra = 257, 256, 128, 2, 70
    B = (deg + 1) ** 2
    c = {k: v.cuda() for k, v in _head_case(9700, n, M, H2, deg, torch.float32).items()}
    rows_out = torch.rand(n, 3 * B + 1, device="cuda")
    g = [torch.zeros(s, device="cuda") for s in ((M,), (1,), (3 * B, H2), (3 * B,))]
    ref = ops.heads_coef_bwd(c["y"], c["h2"], c["wc"], c["q"], c["dirs"], rows_out, *g, deg)
    dh2, dsig, cs = (torch.full(s, CANARY, device="cuda") for s in ((n + extra, H2), (n + extra,), (n + extra, H2)))
    nb = C.c_size_t(0)
    assert lib.swn_heads_coef_bwd_workspace_bytes(n, M, H2, deg, C.byref(nb)) == 0
    ws = torch.empty(nb.value // 4, device="cuda")
    g2 = [torch.zeros_like(t) for t in g]

    def bwd(n_, deg_=deg, M_=M, H2_=H2, drop=None, wsb=None, dt=0):
        p = [ops._p(c["y"]), ops._p(c["h2"]), dt, ops._p(c["wc"]), ops._p(c["q"]), ops._p(c["dirs"]), ops._pv(rows_out[:, 3 * B]), 3 * B + 1, n_, M_,
             H2_, deg_, ops._p(dh2), ops._p(dsig)] + [ops._p(t) for t in g2] + [ops._p(cs), ops._p(ws), nb.value if wsb is None else wsb,
                                                                               ops._stream()]
        if drop is not None:
            p[drop] = None
        return lib.swn_heads_coef_bwd(*p)
    f32code = ops._dt(c["y"])
    assert bwd(n, dt=f32code) == 0
    assert torch.equal(dh2[:n], ref[0]) and torch.equal(dsig[:n], ref[1]) and torch.equal(cs[:n], ref[2])
    assert all(torch.equal(a, b) for a, b in zip(g, g2))
    assert (dh2[n:] == CANARY).all() and (dsig[n:] == CANARY).all() and (cs[n:] == CANARY).all()
    for t in (dh2, dsig, cs):
        t.fill_(CANARY)
    keep = [t.clone() for t in g2]
    assert bwd(0, dt=f32code) == 0                                  # n == 0: nothing is launched, nothing accumulated
    assert (dh2 == CANARY).all() and (dsig == CANARY).all() and (cs == CANARY).all() and all(torch.equal(a, b) for a, b in zip(keep, g2))
    assert bwd(n, deg_=5, dt=f32code) != 0 and bwd(n, deg_=-1, dt=f32code) != 0 and bwd(n, M_=128, dt=f32code) != 0 and bwd(n, H2_=64, dt=f32code) != 0
    assert bwd(n, dt=77) != 0 and bwd(n, wsb=16, dt=f32code) != 0 and bwd(-1, dt=f32code) != 0
    for k in (0, 1, 3, 4, 5, 6, 12, 13, 14, 15, 16, 17, 19):          # (group_colsum, 18, may be NULL)
        assert bwd(n, drop=k, dt=f32code) != 0, k
    assert bwd(n, drop=18, dt=f32code) == 0
    # forward
    out = torch.full((n + extra, 3 * B + 1), CANARY, device="cuda")

    def fwd(n_, deg_=deg, inner=0, drop=None, stride=3 * B + 1, M_=M, dt=f32code):
        p = [ops._p(c["y"]), ops._p(c["h2"]), dt, ops._p(c["ws"]), ops._p(c["bs"]), ops._p(c["wc"]), ops._p(c["bc"]), None, deg_, inner, n_, M_, H2,
             ops._p(out), stride, ops._stream()]
        if drop is not None:
            p[drop] = None
        return lib.swn_heads_coef_fwd(*p)
    assert fwd(n) == 0
    assert (out[n:] == CANARY).all() and not (out[:n] == CANARY).any()
    out.fill_(CANARY)
    assert fwd(0) == 0
    assert fwd(n, deg_=5) != 0 and fwd(n, inner=1) != 0 and fwd(n, stride=3 * B) != 0 and fwd(n, M_=384) != 0 and fwd(n, dt=77) != 0 and fwd(-1) != 0
    for k in (0, 1, 3, 4, 5, 6, 13):
        assert fwd(n, drop=k) != 0, k
    torch.cuda.synchronize()
    assert (out == CANARY).all()
