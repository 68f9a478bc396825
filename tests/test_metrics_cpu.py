"""CPU-only: the image metrics' host side (switch_nerf_amd/metrics.py) and the fp64 restatement the GPU tests measure against
(tests/metrics_restate.py), pinned on the reference's own floats (tests/golden/metrics.npz, scripts/gen_golden_metrics.py)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import metrics_restate as restate
from switch_nerf_amd import metrics

from metrics_restate import REF_ERR_MAP, REF_ERR_SCALAR      # the measured maxima this file re-measures (profiles/r23_metrics.md)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(f"{golden_dir}/metrics.npz")


def case_inputs(g, name):
    """-> pred, target, mask or None, filter_size of a golden case."""
    if f"{name}_of" in g.files:
        base = str(g[f"{name}_of"])
        return g[f"{base}_pred"], g[f"{base}_target"], g[f"{name}_mask"], int(g[f"{name}_fs"])
    return g[f"{name}_pred"], g[f"{name}_target"], None, int(g[f"{name}_fs"])


def test_restatement_matches_the_reference(golden):
    g = golden
    assert len(g["cases"]) == 22
    worst_scalar = worst_map = 0.0
    for name in map(str, g["cases"]):
        x, y, mask, fs = case_inputs(g, name)
        r = restate.metrics(x, y, g[f"taps_{fs}"], mask=mask)
        if mask is None:
            pairs = [(float(g[f"{name}_ssim"]), r["ssim"]), (float(g[f"{name}_mse"]), r["mse"])]
            worst_map = max(worst_map, float(np.abs(g[f"{name}_map"].astype(np.float64) - r["map"]).max()))
            psnr_ref, psnr, mse = float(g[f"{name}_psnr"]), r["psnr"], r["mse"]
        else:
            pairs = [(float(g[f"{name}_ssim_mask"]), r["ssim_mask"]), (float(g[f"{name}_mse_mask"]), r["mse_mask"])]
            psnr_ref, psnr, mse = float(g[f"{name}_psnr_mask"]), r["psnr_mask"], r["mse_mask"]
        for ref, mine in pairs:
            if math.isnan(ref):
                assert math.isnan(mine), name
            else:
                assert abs(ref - mine) <= REF_ERR_SCALAR, (name, ref, mine)
                worst_scalar = max(worst_scalar, abs(ref - mine))
        # psnr: the mse bound through d psnr / d mse = 10 / (ln 10 mse), plus two fp32 ulps of the value for log10 and the product
        if math.isnan(psnr_ref) or math.isinf(psnr_ref):
            assert (math.isnan(psnr) and math.isnan(psnr_ref)) or psnr == psnr_ref, name
        else:
            assert abs(psnr_ref - psnr) <= 10 / math.log(10) * REF_ERR_SCALAR / mse + 2 * np.spacing(np.float32(abs(psnr_ref))), name
    print(f"reference vs fp64 restatement: scalar {worst_scalar:.3e}, map {worst_map:.3e}")
    assert worst_map <= REF_ERR_MAP
    # the constants are the measured maxima, not a loose cap over them
    assert worst_scalar >= 0.9 * REF_ERR_SCALAR and worst_map >= 0.9 * REF_ERR_MAP


def test_special_cases_of_the_restatement(golden):
    g = golden
    x, y, _, fs = case_inputs(g, "ident")
    r = restate.metrics(x, y, g[f"taps_{fs}"])
    assert r["ssim"] == 1.0 and r["mse"] == 0.0 and r["psnr"] == math.inf and float(g["ident_psnr"]) == math.inf
    x, y, mask, fs = case_inputs(g, "mask_none")
    r = restate.metrics(x, y, g[f"taps_{fs}"], mask=mask)
    assert math.isnan(r["ssim_mask"]) and math.isnan(r["psnr_mask"])
    assert math.isnan(float(g["mask_none_ssim_mask"])) and math.isnan(float(g["mask_none_psnr_mask"]))
    x, y, _, fs = case_inputs(g, "neg")
    assert restate.metrics(x, y, g[f"taps_{fs}"])["ssim"] < 0            # the negative-covariance branch is what this case runs


@pytest.mark.parametrize("size", [1, 3, 11, 15])
def test_taps_are_the_references_bits(golden, size):
    t = metrics._taps(size, 1.5)
    assert t.dtype == torch.float32 and t.device.type == "cpu" and t.shape == (size,)
    assert np.array_equal(t.numpy().view(np.uint32), golden[f"taps_{size}"].view(np.uint32))
    assert metrics._taps(size, 1.5) is t                                 # cached: the same host memory on every call


def test_argument_checking():
    img = torch.rand(6, 9, 3)
    with pytest.raises(ValueError, match="differ in shape"):
        metrics.image_metrics(img, torch.rand(6, 8, 3))
    with pytest.raises(ValueError, match="1 to 4 channels"):
        metrics.image_metrics(torch.rand(6, 9, 5), torch.rand(6, 9, 5))
    for fs in (0, 2, 10, 17, -3):
        with pytest.raises(ValueError, match="filter_size must be odd"):
            metrics.image_metrics(img, img, filter_size=fs)
        with pytest.raises(ValueError, match="filter_size must be odd"):
            metrics.ssim(img, img, 1.0, filter_size=fs)
    with pytest.raises(ValueError, match="valid_mask must be bool or uint8"):
        metrics.image_metrics(img, img, valid_mask=torch.ones(6, 8, dtype=torch.bool))
    with pytest.raises(ValueError, match="pred must be fp32, bf16 or fp16"):
        metrics.image_metrics(img.double(), img.double())
    # well-formed arguments on the host: there is no CPU path
    for fn in (lambda: metrics.image_metrics(img, img), lambda: metrics.psnr(img, img), lambda: metrics.ssim(img, img, 1.0),
               lambda: metrics.psnr_mask(img, img, torch.ones(6, 9, dtype=torch.bool)),
               lambda: metrics.ssim_mask(img, img, 1.0, torch.ones(6, 9, dtype=torch.bool))):
        with pytest.raises(ValueError, match="GPU only"):
            fn()
    with pytest.raises(ValueError, match=r"one image \[A, B, C\] or \[1, A, B, C\]"):
        metrics.ssim(torch.rand(2, 6, 9, 3), torch.rand(2, 6, 9, 3), 1.0)


def test_entry_point_validates_before_launch():
    """swn_ssim_fwd rejects an even or oversized window with a NEGATIVE code, every other bad argument with a message; the workspace is
    20 bytes per image and tile of metrics.TILE^2 pixels (fake non-null pointers are never dereferenced on the host)."""
    from switch_nerf_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(0x1000)
    taps = (C.c_float * 15)(*([1.0 / 15] * 15))
    tp = C.cast(taps, C.c_void_p)
    err = lambda: lib.swn_last_error().decode()
    need = C.c_size_t(0)
    T = metrics.TILE
    assert lib.swn_ssim_workspace_bytes(2, T + 1, 2 * T + 1, C.byref(need)) == 0 and need.value == 2 * 2 * 3 * 20
    assert lib.swn_ssim_workspace_bytes(1, T, T, C.byref(need)) == 0 and need.value == 20
    assert lib.swn_ssim_workspace_bytes(0, T, T, C.byref(need)) != 0
    for fs in (0, 2, 10, 16, 17, -1):
        assert lib.swn_ssim_fwd(p, p, None, 1, 8, 8, 3, tp, fs, 1e-4, 9e-4, None, p, 1 << 20, p, None) < 0 and "filter_size" in err()
    assert lib.swn_ssim_fwd(p, p, None, 1, 8, 8, 5, tp, 11, 1e-4, 9e-4, None, p, 1 << 20, p, None) > 0 and "channels" in err()
    assert lib.swn_ssim_fwd(p, p, None, 1, 8, 8, 0, tp, 11, 1e-4, 9e-4, None, p, 1 << 20, p, None) > 0 and "channels" in err()
    assert lib.swn_ssim_fwd(p, None, None, 1, 8, 8, 3, tp, 11, 1e-4, 9e-4, None, p, 1 << 20, p, None) > 0 and "null pointer" in err()
    assert lib.swn_ssim_fwd(p, p, None, 1, 0, 8, 3, tp, 11, 1e-4, 9e-4, None, p, 1 << 20, p, None) > 0 and "bad sizes" in err()
    assert lib.swn_ssim_fwd(p, p, None, 1, 8, 8, 3, tp, 11, 1e-4, 9e-4, None, p, 19, p, None) > 0 and "workspace" in err()
    assert lib.swn_ssim_fwd(p, p, None, 1, 8, 8, 3, tp, 11, 1e-4, 9e-4, None, C.c_void_p(0x1004), 1 << 20, p, None) > 0 \
        and "misaligned" in err()
