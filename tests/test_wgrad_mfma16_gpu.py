"""swn_wgrad_multi, the balanced weight-gradient stream launch, on 16-bit operands (16x16x32 MFMAs on fragments read with the
transposing LDS read out of a swizzled slab image): dW and db against fp64 torch on the same rounded operands, over the job widths,
ragged groups, gathered and packed row layouts the step uses; gathered == dispatched and launch == launch bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (m, n, bias): every width class of the kernel - full 256 x 256 tiles, half-width tiles on either side (whole waves idle), and 32
# columns (most 16 x 16 sub-tiles of a wave past the width)
DIMS = [(256, 256, True), (128, 256, True), (256, 128, True), (32, 256, True), (256, 32, False), (96, 160, True), (64, 64, True)]
# rows of the (segment, expert) groups: empty, 1, one slab -1 / exact / +1, one row past two slabs, 300 (odd slab count), capacity
COUNTS = [0, 1, 31, 32, 33, 65, 300, 331]
CAP, E = 331, 4


@pytest.fixture(params=["bf16", "f16"])
def half(request):
    from switch_nerf_amd import _lib
    _lib.use_half(request.param)
    yield torch.bfloat16 if request.param == "bf16" else torch.float16
    _lib.use_half("bf16")


def _ops():
    from switch_nerf_amd import ops
    return ops


def _case(dtype, packed, seed=5):
    """7 jobs over one grouping; job 0 reads A through a permutation, job 6 reads B through one (the step's first / last expert
    layer).  packed: the groups sit back to back (group_begin) instead of at multiples of CAP."""
    rng = np.random.default_rng(seed)
    counts = np.array(COUNTS, dtype=np.int32)
    ng = len(counts)
    if packed:
        begin = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int32)
        rows = int(counts.sum())
    else:
        begin = np.arange(ng, dtype=np.int32) * CAP
        rows = ng * CAP
    perm = rng.permutation(rows).astype(np.int32)
    dev = torch.device("cuda")
    jobs, refs, plain = [], [], []
    for ji, (m, n, bias) in enumerate(DIMS):
        a = torch.from_numpy(rng.standard_normal((rows, m)).astype(np.float32)).to(dtype)
        b = torch.from_numpy(rng.standard_normal((rows, n)).astype(np.float32)).to(dtype)
        dw = torch.full((E, m, n), 0.5, device=dev)
        db = torch.full((E, n), -1.0, device=dev) if bias else None
        a_dev, b_dev, ag, bg = a.to(dev), b.to(dev), None, None
        plain.append((a_dev, b_dev))
        if ji == 0:             # A rows stored shuffled, read through the index
            src = torch.empty_like(a_dev)
            src[torch.from_numpy(perm).long().to(dev)] = a_dev
            a_dev, ag = src, torch.from_numpy(perm).to(dev)
        if ji == len(DIMS) - 1:
            src = torch.empty_like(b_dev)
            src[torch.from_numpy(perm).long().to(dev)] = b_dev
            b_dev, bg = src, torch.from_numpy(perm).to(dev)
        jobs.append((a_dev, b_dev, dw, db, ag, bg))
        ad, bd = a.double(), b.double()
        rw = torch.full((E, m, n), 0.5, dtype=torch.float64)
        rb = torch.full((E, n), -1.0, dtype=torch.float64)
        bound_w = torch.zeros(E, m, n, dtype=torch.float64)
        bound_b = torch.zeros(E, n, dtype=torch.float64)
        for g in range(ng):
            r0, r1 = int(begin[g]), int(begin[g]) + int(counts[g])
            rw[g % E] += ad[r0:r1].t() @ bd[r0:r1]
            rb[g % E] += bd[r0:r1].sum(0)
            bound_w[g % E] += ad[r0:r1].abs().t() @ bd[r0:r1].abs()
            bound_b[g % E] += bd[r0:r1].abs().sum(0)
        refs.append((rw, rb, bound_w, bound_b))
    kw = dict(n_groups=ng, n_wsets=E, group_stride=CAP, group_rows=torch.from_numpy(counts).to(dev), group_rows_clamp=CAP, tag=1)
    if packed:
        kw["group_begin"] = torch.from_numpy(begin).to(dev)
    return jobs, refs, plain, kw


def _check(jobs, refs, tag):
    # the products are exact in fp32; only the order of the fp32 additions differs from the fp64 sum: bound each element by
    # (additions) * 2^-24 * sum |a| |b|, with the row count of a weight set as the number of additions
    n_add = sum(COUNTS) + 2
    for ji, ((_a, _b, dw, db, _ag, _bg), (rw, rb, bw, bb)) in enumerate(zip(jobs, refs)):
        err = (dw.double().cpu() - rw).abs()
        tol = n_add * 2.0 ** -24 * (bw + 0.5) + 1e-6
        assert bool((err <= tol).all()), f"{tag} job {ji} {DIMS[ji]}: dW max err {err.max().item():.3e}, worst ratio {(err / tol).max().item():.2f}"
        if db is not None:
            errb = (db.double().cpu() - rb).abs()
            tolb = n_add * 2.0 ** -24 * (bb + 1.0) + 1e-6
            assert bool((errb <= tolb).all()), f"{tag} job {ji}: db max err {errb.max().item():.3e}"


@pytest.mark.parametrize("packed", [False, True])
def test_wgrad_multi_16bit_vs_fp64(half, packed):
    """7 jobs of different widths in one launch against the fp64 sum, plain and packed group layouts."""
    jobs, refs, _plain, kw = _case(half, packed)
    _ops().wgrad_multi(jobs, **kw)
    torch.cuda.synchronize()
    _check(jobs, refs, f"{half} packed={packed}")


@pytest.mark.parametrize("packed", [False, True])
def test_wgrad_multi_16bit_gathered_and_deterministic(half, packed):
    """A read through the permutation (first layer) and B read through it (last layer) give the bits of the dispatched operands;
    two launches give the same bits."""
    jobs, _refs, plain, kw = _case(half, packed, seed=9)
    o = _ops()
    o.wgrad_multi(jobs, **kw)
    disp = []
    for (a, b), (_a, _b, dw, db, _ag, _bg) in zip(plain, jobs):
        disp.append((a, b, torch.full_like(dw, 0.5), None if db is None else torch.full_like(db, -1.0), None, None))
    o.wgrad_multi(disp, **kw)
    again = [(a, b, torch.full_like(dw, 0.5), None if db is None else torch.full_like(db, -1.0), ag, bg)
             for (a, b, dw, db, ag, bg) in jobs]
    o.wgrad_multi(again, **kw)
    torch.cuda.synchronize()
    for ji, (j, d, r) in enumerate(zip(jobs, disp, again)):
        assert torch.equal(j[2], d[2]) and torch.equal(j[2], r[2]), f"job {ji}: dW differs"
        if j[3] is not None:
            assert torch.equal(j[3], d[3]) and torch.equal(j[3], r[3]), f"job {ji}: db differs"


def test_wgrad_multi_16bit_single_jobs_match_fp64(half):
    """Each width alone in its own launch (the cut of the work differs from the 7-job launch): same bound."""
    jobs, refs, _plain, kw = _case(half, False, seed=13)
    o = _ops()
    for ji in range(len(jobs)):
        o.wgrad_multi([jobs[ji]], **kw)
    torch.cuda.synchronize()
    _check(jobs, refs, f"{half} single")
