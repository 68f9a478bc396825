"""Image metrics of the validation loop on the device: the reference's metrics.py (psnr :8-10, ssim :51-121, psnr_mask / ssim_mask
:124-208) over one fused HIP pass (csrc/ssim.hip, ops.ssim_fwd).

image_metrics() is the form a validation loop calls and a hipGraph can hold: device tensors in, device tensors out, no host read and
no synchronise.  psnr / ssim / psnr_mask / ssim_mask take the reference's signatures and return Python floats - the one host read.
There is no CPU path (the CPU statement of the formula lives in tests/metrics_restate.py); LPIPS is not provided.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import ops

TILE = 32            # SWN_SSIM_TILE (include/swn.h): the edge of the square of output pixels one workgroup owns
MAX_FILTER_SIZE = 15

_taps_cache = {}


def _check_filter(filter_size) -> int:
    if int(filter_size) != filter_size or not 1 <= filter_size <= MAX_FILTER_SIZE or filter_size % 2 == 0:
        raise ValueError(f"filter_size must be odd and in 1..{MAX_FILTER_SIZE}, got {filter_size} (even windows are not supported: "
                         "the reference's two passes then change the image size)")
    return int(filter_size)


def _taps(filter_size: int, filter_sigma: float) -> torch.Tensor:
    """The normalised Gaussian window as the reference's torch ops round it on the host: fp32 tap positions, fp32 exp, fp32 sum, divide
    (metrics.py:81-85; an odd size is centred on its middle tap)."""
    filter_size = _check_filter(filter_size)
    key = (filter_size, float(filter_sigma))
    t = _taps_cache.get(key)
    if t is None:
        pos = torch.arange(filter_size, dtype=torch.float32) - float(filter_size // 2)
        w = torch.exp(-0.5 * (pos / filter_sigma) ** 2)
        t = _taps_cache[key] = (w / torch.sum(w)).contiguous()
    return t


_u8_tables = {}


def _u8_to_unit(t: torch.Tensor) -> torch.Tensor:
    """uint8 -> fp32 k / 255 with the quotient rounded as the host's division rounds it (the runner's `/ 255.` on its CPU ground truth):
    a 256-entry table made on the host, one per device (a host-to-device copy on first use, so before any capture), gathered on the
    device - a device-side `t / 255.0` multiplies by a rounded reciprocal instead and is off by an ulp for some k."""
    tab = _u8_tables.get(t.device)
    if tab is None:
        tab = _u8_tables[t.device] = (torch.arange(256, dtype=torch.float32) / 255.0).to(t.device)
    return tab[t.long()]


def _as_batch(name: str, t: torch.Tensor) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dim() < 3:
        raise ValueError(f"{name} must be a tensor [..., A, B, C], got {type(t).__name__ if not isinstance(t, torch.Tensor) else tuple(t.shape)}")
    return t.reshape(-1, *t.shape[-3:])


def image_metrics(pred: torch.Tensor, target: torch.Tensor, max_val: float = 1.0, valid_mask: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None, want_map: bool = False, filter_size: int = 11, filter_sigma: float = 1.5,
                  k1: float = 0.01, k2: float = 0.03) -> Dict[str, torch.Tensor]:
    """PSNR and SSIM of rendered images against their ground truth, on the device.

    pred [..., A, B, C] fp32 / bf16 / fp16 (upcast to fp32), target the same shape in a float type or uint8 (converted to k / 255, the
    runner's ground truth), C <= 4, any leading batch (n images).  valid_mask [..., A, B] bool or uint8: the Mega-NeRF cell's cluster
    mask.  Returns DEVICE tensors `psnr`, `ssim`, `mse` [n]; with a mask also `psnr_mask`, `ssim_mask` (nan where the mask selects
    nothing, as the reference's mean of an empty tensor); with want_map also `ssim_map` [n, A, B, C].  out: a caller's fp32 [n, 4]
    buffer for the raw (ssim, mse, ssim_mask, mse_mask) rows, e.g. one a captured graph keeps writing.  mse == 0 gives psnr = +inf.
    No host read, no synchronise: the pair of launches and the few elementwise ops around it follow the caller's stream."""
    p, t = _as_batch("pred", pred), _as_batch("target", target)
    if p.shape != t.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and target {tuple(target.shape)} differ in shape")
    n, A, B, Cc = p.shape
    if not 1 <= Cc <= 4:
        raise ValueError(f"1 to 4 channels (the last axis), got C = {Cc}")
    if n < 1 or A < 1 or B < 1:
        raise ValueError(f"empty image batch {tuple(pred.shape)}")
    taps = _taps(filter_size, filter_sigma)
    if p.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise ValueError(f"pred must be fp32, bf16 or fp16, got {p.dtype}")
    if not (t.dtype == torch.uint8 or t.dtype.is_floating_point):
        raise ValueError(f"target must be a float type or uint8, got {t.dtype}")
    m = None
    if valid_mask is not None:
        if valid_mask.dtype not in (torch.bool, torch.uint8) or valid_mask.numel() != n * A * B or tuple(valid_mask.shape[-2:]) != (A, B):
            raise ValueError(f"valid_mask must be bool or uint8 [..., {A}, {B}] over the {n} image(s), got {valid_mask.dtype} "
                             f"{tuple(valid_mask.shape)}")
        m = valid_mask.reshape(n, A, B).contiguous()
        m = m.view(torch.uint8) if m.dtype == torch.bool else m
    if not (p.is_cuda and t.is_cuda and (m is None or m.is_cuda)):
        raise ValueError("image_metrics runs on the GPU only: pred, target and valid_mask must be device tensors (there is no CPU path)")
    if not (p.device == t.device and (m is None or m.device == p.device)):
        raise ValueError("pred, target and valid_mask must live on one device")
    if out is not None and (out.dtype != torch.float32 or tuple(out.shape) != (n, 4) or not out.is_contiguous() or out.device != p.device):
        raise ValueError(f"out must be a contiguous fp32 [{n}, 4] tensor on {p.device}")
    p = p.to(torch.float32).contiguous()
    t = (_u8_to_unit(t) if t.dtype == torch.uint8 else t.to(torch.float32)).contiguous()
    ssim_map = torch.empty_like(p) if want_map else None
    with torch.cuda.device(p.device):
        raw = ops.ssim_fwd(p, t, taps, (k1 * max_val) ** 2, (k2 * max_val) ** 2, mask=m, map_out=ssim_map, out=out)
    log = -10.0 * torch.log10(raw[:, 1::2])                    # [n, 2]: psnr, psnr_mask
    res = {"psnr": log[:, 0], "ssim": raw[:, 0], "mse": raw[:, 1]}
    if m is not None:
        res["psnr_mask"], res["ssim_mask"] = log[:, 1], raw[:, 2]
    if want_map:
        res["ssim_map"] = ssim_map
    return res


def _one(name: str, rgbs: torch.Tensor) -> None:
    if not isinstance(rgbs, torch.Tensor) or not (rgbs.dim() == 3 or (rgbs.dim() == 4 and rgbs.shape[0] == 1)):
        raise ValueError(f"{name}: one image [A, B, C] or [1, A, B, C] (a batch goes through image_metrics)")


def psnr(rgbs: torch.Tensor, target_rgbs: torch.Tensor) -> float:
    _one("psnr", rgbs)
    return image_metrics(rgbs, target_rgbs)["psnr"].item()


def ssim(rgbs: torch.Tensor, target_rgbs: torch.Tensor, max_val: float, filter_size: int = 11, filter_sigma: float = 1.5,
         k1: float = 0.01, k2: float = 0.03) -> float:
    _one("ssim", rgbs)
    return image_metrics(rgbs, target_rgbs, max_val, filter_size=filter_size, filter_sigma=filter_sigma, k1=k1, k2=k2)["ssim"].item()


def psnr_mask(rgbs: torch.Tensor, target_rgbs: torch.Tensor, valid_mask: torch.Tensor) -> float:
    _one("psnr_mask", rgbs)
    return image_metrics(rgbs, target_rgbs, valid_mask=valid_mask)["psnr_mask"].item()


def ssim_mask(rgbs: torch.Tensor, target_rgbs: torch.Tensor, max_val: float, valid_mask: torch.Tensor, filter_size: int = 11,
              filter_sigma: float = 1.5, k1: float = 0.01, k2: float = 0.03) -> float:
    _one("ssim_mask", rgbs)
    return image_metrics(rgbs, target_rgbs, max_val, valid_mask=valid_mask, filter_size=filter_size, filter_sigma=filter_sigma,
                         k1=k1, k2=k2)["ssim_mask"].item()
