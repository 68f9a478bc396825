"""swn_wgrad_multi: the four copies of the stream kernel's piece (gathered / plain slab loop x with / without bias sums), which a
workgroup picks per (job, weight set) piece.  One launch mixes every kind of job; it is checked against the fp64 sum, against the same
jobs with materialised operands, against single-job launches, and across the two variant switches inside one workgroup's walk."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E = 8                                  # weight sets
COUNTS = [0, 1, 31, 32, 33, 65, 300]   # rows of a group: empty, 1, one slab of 32 rows -1 / exact / +1, two slabs + 1, odd slab count
CAP = 300
# (m, n, A gathered, B gathered, bias): the four gather kinds, and every (gathered / plain) x (with / without db) copy of the piece
MIXED = [(256, 256, True, False, True), (128, 256, False, True, True), (256, 32, True, True, False), (64, 64, False, False, False),
         (256, 256, False, False, True), (64, 64, False, False, True)]


@pytest.fixture(params=["bf16", "f16"])
def half(request):
    from switch_nerf_amd import _lib
    _lib.use_half(request.param)
    yield torch.bfloat16 if request.param == "bf16" else torch.float16
    _lib.use_half("bf16")


def _ops():
    from switch_nerf_amd import ops
    return ops


def _values(rng, shape, kind):
    """randn: the additions round, so the bits depend on their order.  grid: multiples of 1/8 in [-4, 4] - every product is a multiple of
    2^-6 below 16 and every partial sum of the <= 8192 rows used here fits 24 bits, so no fp32 addition rounds and the bits do NOT
    depend on the order (used where two launches cut the rows differently)."""
    if kind == "grid":
        return (rng.integers(-32, 33, size=shape) / 8.0).astype(np.float32)
    return rng.standard_normal(shape).astype(np.float32)


def _case(dtype, specs, counts, packed, kind, seed, cap=CAP):
    """specs: (m, n, gather A, gather B, bias) per job; counts: rows of group g (weight set g % E).  Returns the jobs as launched
    (gathered operands stored shuffled, read through the index), the same jobs with the operands in row order and no index, the fp64
    references with their |a| |b| sums, and the grouping arguments."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, dtype=np.int32)
    ng = len(counts)
    if packed:
        begin = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int32)
        rows = int(counts.sum())
    else:
        begin = np.arange(ng, dtype=np.int32) * cap
        rows = ng * cap
    dev = torch.device("cuda")
    perm = torch.from_numpy(rng.permutation(rows).astype(np.int32)).to(dev)
    jobs, mat, refs = [], [], []
    for (m, n, ga, gb, bias) in specs:
        a = torch.from_numpy(_values(rng, (rows, m), kind)).to(dtype)
        b = torch.from_numpy(_values(rng, (rows, n), kind)).to(dtype)
        fresh = lambda: (torch.full((E, m, n), 0.5, device=dev), torch.full((E, n), -1.0, device=dev) if bias else None)  # noqa: E731
        a_dev, b_dev = a.to(dev), b.to(dev)
        dw, db = fresh()
        mat.append((a_dev, b_dev, dw, db, None, None))

        def shuffled(x):
            src = torch.empty_like(x)
            src[perm.long()] = x
            return src
        dw, db = fresh()
        jobs.append((shuffled(a_dev) if ga else a_dev, shuffled(b_dev) if gb else b_dev, dw, db, perm if ga else None, perm if gb else None))
        ad, bd = a.double(), b.double()
        rw = torch.full((E, m, n), 0.5, dtype=torch.float64)
        rb = torch.full((E, n), -1.0, dtype=torch.float64)
        bw = torch.zeros(E, m, n, dtype=torch.float64)
        bb = torch.zeros(E, n, dtype=torch.float64)
        for g in range(ng):
            r0, r1 = int(begin[g]), int(begin[g]) + int(counts[g])
            rw[g % E] += ad[r0:r1].t() @ bd[r0:r1]
            rb[g % E] += bd[r0:r1].sum(0)
            bw[g % E] += ad[r0:r1].abs().t() @ bd[r0:r1].abs()
            bb[g % E] += bd[r0:r1].abs().sum(0)
        refs.append((rw, rb, bw, bb))
    kw = dict(n_groups=ng, n_wsets=E, group_stride=cap, group_rows=torch.from_numpy(counts).to(dev), group_rows_clamp=cap, tag=1)
    if packed:
        kw["group_begin"] = torch.from_numpy(begin).to(dev)
    return jobs, mat, refs, kw


def _check_fp64(jobs, refs, n_add, tag):
    # the bound of tests/test_wgrad_mfma16_gpu.py: the products are exact in fp32, only the order of the fp32 additions differs from the
    # fp64 sum: (additions) * 2^-24 * sum |a| |b| per element, with the rows of a weight set (+ 2) as the number of additions
    for ji, ((_a, _b, dw, db, _ag, _bg), (rw, rb, bw, bb)) in enumerate(zip(jobs, refs)):
        err = (dw.double().cpu() - rw).abs()
        tol = n_add * 2.0 ** -24 * (bw + 0.5) + 1e-6
        assert bool((err <= tol).all()), f"{tag} job {ji}: dW max err {err.max().item():.3e}, worst ratio {(err / tol).max().item():.2f}"
        if db is not None:
            errb = (db.double().cpu() - rb).abs()
            tolb = n_add * 2.0 ** -24 * (bb + 1.0) + 1e-6
            assert bool((errb <= tolb).all()), f"{tag} job {ji}: db max err {errb.max().item():.3e}"


def _same_bits(x, y, tag):
    for ji, (p, q) in enumerate(zip(x, y)):
        assert torch.equal(p[2], q[2]), f"{tag} job {ji}: dW differs"
        if p[3] is not None:
            assert torch.equal(p[3], q[3]), f"{tag} job {ji}: db differs"


def _mixed_counts():
    # 56 groups (7 per weight set): weight set e walks COUNTS from a start of its own, so every set holds every count, 462 rows in all
    return [COUNTS[(seg + g_e) % len(COUNTS)] for seg in range(len(COUNTS)) for g_e in range(E)]


@pytest.mark.parametrize("kind", ["randn", "grid"])
@pytest.mark.parametrize("packed", [False, True])
def test_wgrad_variants_mixed_launch(half, packed, kind):
    """One launch with gathered A / gathered B / both / neither, with and without db, widths 256/256, 128/256, 256/32, 64/64: against
    the fp64 sum, and bit for bit against the same launch with materialised operands (same cut of the rows, so the same additions in
    the same order).  Single-job launches cut the rows differently, so their additions come in another order: they are compared bit
    for bit on the grid operands, whose sums are exact in any order, and against the fp64 bound on the random ones."""
    jobs, mat, refs, kw = _case(half, MIXED, _mixed_counts(), packed, kind, seed=21)
    o = _ops()
    o.wgrad_multi(jobs, **kw)
    o.wgrad_multi(mat, **kw)
    single = [(a, b, torch.full_like(dw, 0.5), None if db is None else torch.full_like(db, -1.0), ag, bg) for (a, b, dw, db, ag, bg) in jobs]
    for j in single:
        o.wgrad_multi([j], **kw)
    torch.cuda.synchronize()
    n_add = sum(COUNTS) + 2
    tag = f"{half} packed={packed} {kind}"
    _check_fp64(jobs, refs, n_add, tag + " mixed")
    _same_bits(jobs, mat, tag + " gathered vs materialised")
    _check_fp64(single, refs, n_add, tag + " single")
    if kind == "grid":
        _same_bits(jobs, single, tag + " mixed vs single-job launches")


# ---- variant switches inside one workgroup's walk
SW_ROWS = 1024                      # rows of each of the 8 groups (one per weight set): 32 slabs each, 256 slabs per job
SW_GATHERED = (256, 256, True, False, True)     # weight 16 on the line of work
SW_PLAIN = (64, 64, False, False, False)        # weight 4


def _crossing_workgroups(weights, slabs, n_wg):
    """The kernel's cut (ws_cut / ws_first_slab in wgrad.hip): workgroups whose share holds slabs of both jobs."""
    total = sum(w * slabs for w in weights)

    def first(x, base, w):
        d = x - base
        return 0 if d <= 0 else min((d + w - 1) // w, slabs)
    out = []
    for k in range(n_wg):
        x0, x1 = k * total // n_wg, (k + 1) * total // n_wg
        base, have = 0, []
        for w in weights:
            have.append(first(x0, base, w) < first(x1, base, w))
            base += w * slabs
        if all(have):
            out.append(k)
    return out


@pytest.mark.parametrize("order", ["gathered_first", "plain_first"])
def test_wgrad_variants_switch_inside_workgroup(half, order):
    """Two jobs of 8 groups x 1024 rows (256 slabs each): a gathered 256/256 job with db and a plain 64/64 job without.  The line of
    work is 20 * 256 weighted slabs; with one workgroup per compute unit (256 on this device: 20 units each) the job boundary at 4096
    (gathered first) / 1024 (plain first) is no multiple of the share, so the workgroup that holds it ends one job's last slab and
    starts the other's first - a switch gathered+bias -> plain, and plain -> gathered+bias, inside its walk.  The test recomputes the
    cut for the device's workgroup count and requires such a workgroup."""
    specs = [SW_GATHERED, SW_PLAIN] if order == "gathered_first" else [SW_PLAIN, SW_GATHERED]
    n_wg = min(torch.cuda.get_device_properties(0).multi_processor_count, 1024)
    cross = _crossing_workgroups([(m + n) // 32 for (m, n, *_r) in specs], E * SW_ROWS // 32, n_wg)
    assert cross, f"no workgroup of {n_wg} crosses the job boundary: choose other row counts"
    jobs, mat, refs, kw = _case(half, specs, [SW_ROWS] * E, False, "randn", seed=33, cap=SW_ROWS)
    o = _ops()
    o.wgrad_multi(jobs, **kw)
    o.wgrad_multi(mat, **kw)
    torch.cuda.synchronize()
    _check_fp64(jobs, refs, SW_ROWS + 2, f"{half} {order}")
    _same_bits(jobs, mat, f"{half} {order} gathered vs materialised")
