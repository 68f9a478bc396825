"""GPU: the image metrics (switch_nerf_amd/metrics.py over csrc/ssim.hip) against the fp64 restatement (tests/metrics_restate.py) and
the reference's own floats (tests/golden/metrics.npz), at the smallest shapes at which the kernel can go wrong: images smaller than
the window, one tile exactly, one-pixel tail tiles, a batch, 1 and 4 channels, windows of 1 / 3 / 15 taps, identical / constant /
negated pairs, masks, uint8 and bf16 inputs.  Bounds: metrics_restate.BOUND_SCALAR / BOUND_MAP (profiles/r23_metrics.md).

Measured on the MI355X (profiles/r23_metrics.md): see the kernel-error table there."""
import math

import numpy as np
import pytest
import torch

import metrics_restate as restate
from metrics_restate import BOUND_MAP, BOUND_SCALAR

pytestmark = pytest.mark.gpu

IMAGE_CASES = ["s1x1", "s5x7", "s11x11", "tile", "tails", "big0", "big1", "c1", "c4", "fs1", "fs3", "fs15", "ident", "const", "neg",
               "u8", "bf16"]
MASK_CASES = ["mask_all", "mask_one", "mask_checker", "mask_tail", "mask_none"]
_cache = {}


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(f"{golden_dir}/metrics.npz")
    assert sorted(map(str, g["cases"])) == sorted(IMAGE_CASES + MASK_CASES)
    return g


def case(g, name):
    """-> (pred, target, mask, filter_size) as numpy, the restatement's result: computed once per case, shared, never modified."""
    if name not in _cache:
        base = str(g[f"{name}_of"]) if f"{name}_of" in g.files else name
        x, y = g[f"{base}_pred"], g[f"{base}_target"]
        mask = g[f"{name}_mask"] if base != name else None
        fs = int(g[f"{name}_fs"])
        _cache[name] = (x, y, mask, fs, restate.metrics(x, y, g[f"taps_{fs}"], mask=mask))
    return _cache[name]


def device_inputs(name, x, y, mask):
    """The case's tensors as a user holds them: "u8" the target as uint8 (the golden target is k / 255 in fp32), "bf16" the prediction
    as bf16 (the golden prediction is bf16-representable)."""
    p, t = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    if name == "u8":
        t8 = torch.round(torch.from_numpy(y) * 255).to(torch.uint8)
        assert torch.equal(t8.float() / 255, torch.from_numpy(y))             # on the host, as the reference converted it
        t = t8.cuda()
    if name == "bf16":
        assert torch.equal(p.to(torch.bfloat16).float(), p)
        p = p.to(torch.bfloat16)
    m = None if mask is None else torch.from_numpy(mask).cuda()
    return p, t, m


def second_input(p, t):
    """Another pair of the same shapes and dtypes for the captured buffers."""
    return (1 - p.float()).to(p.dtype), (255 - t) if t.dtype == torch.uint8 else (1 - t).flip(0)


def psnr_bound(mse, psnr):
    """The mse bound through d psnr / d mse = 10 / (ln 10 mse), plus two fp32 ulps of the value (log10 and the product, in fp32)."""
    return 10 / math.log(10) * BOUND_SCALAR / mse + 2 * float(np.spacing(np.float32(abs(psnr))))


def close_scalar(got, want, bound, what):
    print(f"    {what}: got {got!r} want {want!r} |diff| {abs(got - want) if math.isfinite(want) else 0.0:.3e} bound {bound:.3e}")
    if math.isnan(want):
        assert math.isnan(got), what
    elif math.isinf(want):
        assert got == want, what
    else:
        assert abs(got - want) <= bound, (what, got, want, bound)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), k


def check_case(g, name):
    from switch_nerf_amd import metrics
    x, y, mask, fs, want = case(g, name)
    p, t, m = device_inputs(name, x, y, mask)
    kw = dict(valid_mask=m, want_map=True, filter_size=fs)
    res = metrics.image_metrics(p, t, **kw)
    again = metrics.image_metrics(p, t, **kw)
    # the captured pair of launches, replayed on a second input written into the captured buffers
    p2, t2 = second_input(p, t)
    eager2 = metrics.image_metrics(p2, t2, **kw)
    sp, st, out = p.clone(), t.clone(), torch.zeros(1, 4, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        metrics.image_metrics(sp, st, out=out, **kw)               # the side stream's workspace exists before the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        held = metrics.image_metrics(sp, st, out=out, **kw)
    sp.copy_(p2)
    st.copy_(t2)
    graph.replay()
    torch.cuda.synchronize()                                       # nothing below reads an output before the replay has ended
    same_bits(res, again)
    same_bits(held, eager2)
    assert held["ssim"].data_ptr() == out.data_ptr()

    print(f"\n{name}: {tuple(x.shape)} filter {fs}")
    A, B, Cc = x.shape
    assert res["ssim_map"].shape == (1, A, B, Cc) and res["ssim"].shape == res["psnr"].shape == res["mse"].shape == (1,)
    map_err = float(np.abs(res["ssim_map"][0].cpu().numpy().astype(np.float64) - want["map"]).max())
    print(f"    map: max |diff| {map_err:.3e} bound {BOUND_MAP:.3e}")
    assert map_err <= BOUND_MAP
    close_scalar(res["ssim"].item(), want["ssim"], BOUND_SCALAR, "ssim")
    close_scalar(res["mse"].item(), want["mse"], BOUND_SCALAR, "mse")
    close_scalar(res["psnr"].item(), want["psnr"], psnr_bound(want["mse"], want["psnr"]) if want["mse"] > 0 else 0.0, "psnr")
    if mask is None:
        assert "ssim_mask" not in res and "psnr_mask" not in res
        # the float wrappers against the reference's own floats
        close_scalar(metrics.ssim(p, t, 1.0, filter_size=fs), float(g[f"{name}_ssim"]), BOUND_SCALAR, "ssim() vs reference")
        ref_psnr = float(g[f"{name}_psnr"])
        close_scalar(metrics.psnr(p[None], t[None]), ref_psnr, psnr_bound(want["mse"], ref_psnr) if want["mse"] > 0 else 0.0,
                     "psnr() vs reference")
    else:
        close_scalar(res["ssim_mask"].item(), want["ssim_mask"], BOUND_SCALAR, "ssim_mask")
        bound_m = psnr_bound(want["mse_mask"], want["psnr_mask"]) if want["mse_mask"] > 0 else 0.0
        close_scalar(res["psnr_mask"].item(), want["psnr_mask"], bound_m, "psnr_mask")
        close_scalar(metrics.ssim_mask(p, t, 1.0, m), float(g[f"{name}_ssim_mask"]), BOUND_SCALAR, "ssim_mask() vs reference")
        close_scalar(metrics.psnr_mask(p, t, m), float(g[f"{name}_psnr_mask"]), bound_m, "psnr_mask() vs reference")
        # the raw row: mse over the masked pixels
        raw = torch.empty(1, 4, device="cuda")
        metrics.image_metrics(p, t, valid_mask=m.to(torch.uint8), out=raw, filter_size=fs)
        close_scalar(raw[0, 3].item(), want["mse_mask"], BOUND_SCALAR, "mse_mask")
        assert torch.equal(bits(raw[0, :2]), bits(torch.stack([res["ssim"][0], res["mse"][0]])))


@pytest.mark.parametrize("name", IMAGE_CASES)
def test_image_case(golden, name):
    check_case(golden, name)


@pytest.mark.parametrize("name", MASK_CASES)
def test_mask_case(golden, name):
    check_case(golden, name)


def test_shapes_are_the_kernels_edge_cases(golden):
    from switch_nerf_amd import metrics
    T = metrics.TILE
    shape = lambda n: golden[f"{n}_pred"].shape
    assert shape("tile") == (T, T, 3) and shape("tails") == (T + 1, 2 * T + 1, 3) and shape("big0") == shape("big1") == (40, 70, 3)
    assert shape("s1x1") == (1, 1, 3) and shape("s5x7") == (5, 7, 3) and shape("s11x11") == (11, 11, 3)
    assert shape("c1") == (17, 33, 1) and shape("c4") == (17, 33, 4) and shape("fs15") == (17, 33, 3)
    tail = golden["mask_tail_mask"]
    assert tail[:, 2 * T:].all() and not tail[:, :2 * T].any()                 # only the tail tiles along the last axis
    assert golden["mask_one_mask"].sum() == 1 and not golden["mask_none_mask"].any() and golden["mask_all_mask"].all()


def test_identical_and_empty_mask(golden):
    """Identical images: ssim 1 within rounding, mse exactly 0, psnr +inf; an all-false mask: nan in both masked means."""
    from switch_nerf_amd import metrics
    x, y, _, fs, _ = case(golden, "ident")
    p = torch.from_numpy(x).cuda()
    res = metrics.image_metrics(p, p.clone(), want_map=True)
    assert res["mse"].item() == 0.0 and res["psnr"].item() == math.inf and metrics.psnr(p, p.clone()) == math.inf
    assert abs(res["ssim"].item() - 1.0) <= restate.ULP_ONE and float((res["ssim_map"] - 1).abs().max()) <= restate.ULP_ONE
    none = torch.zeros(x.shape[:2], dtype=torch.bool, device="cuda")
    assert math.isnan(metrics.ssim_mask(p, p.clone(), 1.0, none)) and math.isnan(metrics.psnr_mask(p, p.clone(), none))


def test_batch_keeps_images_apart(golden):
    """Two different 40 x 70 images in one call: each row is, bit for bit, the image's own single-image result (per-image partial
    slots do not mix), also with a leading batch shape [2, 1, ...], a per-image mask and a caller's `out`."""
    from switch_nerf_amd import metrics
    pairs = [case(golden, n) for n in ("big0", "big1")]
    p = torch.stack([torch.from_numpy(c[0]) for c in pairs]).cuda()
    t = torch.stack([torch.from_numpy(c[1]) for c in pairs]).cuda()
    mask = torch.zeros(2, 40, 70, dtype=torch.bool, device="cuda")
    mask[0, :, 64:] = True
    mask[1, 3:35, 1:9] = True
    out = torch.empty(2, 4, device="cuda")
    both = metrics.image_metrics(p[:, None], t[:, None], valid_mask=mask[:, None], out=out, want_map=True)
    torch.cuda.synchronize()
    assert both["ssim"].shape == (2,) and both["ssim_map"].shape == (2, 40, 70, 3) and both["ssim"].data_ptr() == out.data_ptr()
    for i, c in enumerate(pairs):
        one = metrics.image_metrics(p[i], t[i], valid_mask=mask[i], want_map=True)
        for k in one:
            assert torch.equal(bits(one[k][0]), bits(both[k][i])), (i, k)
        want = restate.metrics(c[0], c[1], golden["taps_11"], mask=mask[i].cpu().numpy())
        for k in ("ssim", "mse", "ssim_mask"):
            close_scalar(both[k][i].item(), want[k], BOUND_SCALAR, f"image {i} {k}")
        assert float(np.abs(both["ssim_map"][i].cpu().numpy().astype(np.float64) - want["map"]).max()) <= BOUND_MAP
    assert both["ssim"][0].item() != both["ssim"][1].item()
