"""Fixture of the image metrics (switch_nerf_amd/metrics.py) from the REFERENCE's own metrics.psnr / ssim / psnr_mask / ssim_mask, on
the CPU in fp32.

Usage (build container only, like oracle/gen_golden.py: the reference is not on the GPU box):
    python scripts/gen_golden_metrics.py

The reference's metrics module imports `lpips` at its top, which is not installed and not used by the four functions: an empty module
object stands in for it in sys.modules for the import.

Writes tests/golden/metrics.npz, data only:
    cases                      the case names
    taps_<size>                the reference's window (fp32) for sigma 1.5, sizes 1, 3, 11, 15
    <case>_pred / _target      the image pair, fp32 [A, B, C] (a mask case names its image case in <case>_of instead)
    <case>_mask                bool [A, B] (mask cases)
    <case>_fs                  filter_size (max_val is 1, sigma 1.5, k1 / k2 the defaults everywhere)
    <case>_ssim / _psnr        the floats the reference returned;  _ssim_mask / _psnr_mask for mask cases
    <case>_mse / _mse_mask     the fp32 mean squared error under the reference's psnr (checked: -10 log10 of it IS the returned float)
    <case>_map                 the reference's ssim_map [A, B, C], recomputed here with the same torch ops (checked: its mean IS the
                               returned float)
Images are seeded torch.rand, smoothed with a 3 x 3 box so that the local variances are not pure noise; the target is the prediction
plus smoothed noise.  Special pairs: identical, both constant, y = 1 - x, a uint8-representable target (k / 255 in fp32), a
bf16-representable prediction.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("SWN_REFERENCE", "/root/reference")
sys.modules.setdefault("lpips", types.ModuleType("lpips"))
sys.path.insert(0, REF)
from switch_nerf import metrics as ref  # noqa: E402

SIGMA = 1.5
TILE = 32


def smooth(z):
    return F.avg_pool2d(z.permute(2, 0, 1)[None], 3, stride=1, padding=1, count_include_pad=False)[0].permute(1, 2, 0).contiguous()


def pair(seed, A, B, C):
    g = torch.Generator().manual_seed(seed)
    x = smooth(torch.rand(A, B, C, generator=g))
    y = (x + 0.25 * (smooth(torch.rand(A, B, C, generator=g)) - 0.5)).clamp(0.0, 1.0)
    return x, y


def window(fs):
    pos = torch.arange(fs) - fs // 2 + 0.0
    w = torch.exp(-0.5 * (pos / SIGMA) ** 2)
    return w / torch.sum(w)


def ref_map(x, y, fs):
    """The map under the reference's ssim, [A, B, C]: torch fp32, the same grouped convolutions in the same order."""
    C = x.shape[-1]
    w, hw = window(fs), fs // 2
    wb = w.view(1, 1, 1, -1).repeat(C, 1, 1, 1)
    wa = w.view(1, 1, -1, 1).repeat(C, 1, 1, 1)
    blur = lambda z: F.conv2d(F.conv2d(z, wb, padding=[0, hw], groups=C), wa, padding=[hw, 0], groups=C)
    x, y = x.permute(2, 0, 1)[None], y.permute(2, 0, 1)[None]
    mu0, mu1 = blur(x), blur(y)
    mu00, mu11, mu01 = mu0 * mu0, mu1 * mu1, mu0 * mu1
    s00 = torch.clamp(blur(x ** 2) - mu00, min=0.0)
    s11 = torch.clamp(blur(y ** 2) - mu11, min=0.0)
    s01 = blur(x * y) - mu01
    s01 = torch.sign(s01) * torch.min(torch.sqrt(s00 * s11), torch.abs(s01))
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    m = (2 * mu01 + c1) * (2 * s01 + c2) / ((mu00 + mu11 + c1) * (s00 + s11 + c2))
    return m, m[0].permute(1, 2, 0).contiguous()


def same(a, b):
    return a == b or (a != a and b != b)


def main():
    torch.set_num_threads(1)
    out, names = {}, []

    def image_case(name, x, y, fs=11):
        names.append(name)
        ssim, psnr = ref.ssim(x, y, 1.0, filter_size=fs, filter_sigma=SIGMA), ref.psnr(x, y)
        m_bchw, m = ref_map(x, y, fs)
        assert same(torch.mean(m_bchw.reshape([-1, m.numel()]), dim=-1).item(), ssim), name
        mse = torch.mean((x - y) ** 2)
        assert same(-10 * torch.log10(mse).item(), psnr), name
        out.update({f"{name}_pred": x.numpy(), f"{name}_target": y.numpy(), f"{name}_fs": np.int32(fs), f"{name}_ssim": np.float64(ssim),
                    f"{name}_psnr": np.float64(psnr), f"{name}_mse": np.float32(mse.item()), f"{name}_map": m.numpy()})
        return m

    def mask_case(name, of, x, y, m, mask):
        names.append(name)
        ssim, psnr = ref.ssim_mask(x, y, 1.0, mask, filter_sigma=SIGMA), ref.psnr_mask(x, y, mask)
        assert same(torch.mean(m[mask]).item(), ssim), name
        mse = torch.mean((x[mask] - y[mask]) ** 2)
        assert same(-10 * torch.log10(mse).item(), psnr), name
        out.update({f"{name}_of": np.str_(of), f"{name}_mask": mask.numpy(), f"{name}_fs": np.int32(11),
                    f"{name}_ssim_mask": np.float64(ssim), f"{name}_psnr_mask": np.float64(psnr), f"{name}_mse_mask": np.float32(mse.item())})

    for fs in (1, 3, 11, 15):
        out[f"taps_{fs}"] = window(fs).numpy()
    # sizes around the window and the tile
    for i, (name, (A, B, C)) in enumerate((("s1x1", (1, 1, 3)), ("s5x7", (5, 7, 3)), ("s11x11", (11, 11, 3)), ("tile", (TILE, TILE, 3)),
                                           ("big0", (40, 70, 3)), ("big1", (40, 70, 3)), ("c1", (17, 33, 1)), ("c4", (17, 33, 4)))):
        image_case(name, *pair(100 + i, A, B, C))
    xt, yt = pair(120, TILE + 1, 2 * TILE + 1, 3)
    mt = image_case("tails", xt, yt)
    x, y = pair(130, 17, 33, 3)
    for fs in (1, 3, 15):
        image_case(f"fs{fs}", x, y, fs)
    image_case("ident", x, x.clone())
    image_case("const", torch.full((17, 33, 3), 0.3), torch.full((17, 33, 3), 0.6))
    image_case("neg", x, 1.0 - x)
    image_case("u8", x, torch.round(y * 255).to(torch.uint8).float() / 255)
    image_case("bf16", x.to(torch.bfloat16).float(), y)
    # masks over the image with tail tiles
    A, B = xt.shape[:2]
    masks = {"mask_all": torch.ones(A, B, dtype=torch.bool), "mask_none": torch.zeros(A, B, dtype=torch.bool),
             "mask_one": torch.zeros(A, B, dtype=torch.bool), "mask_tail": torch.zeros(A, B, dtype=torch.bool),
             "mask_checker": (torch.arange(A)[:, None] + torch.arange(B)[None, :]) % 2 == 0}
    masks["mask_one"][7, 40] = True
    masks["mask_tail"][:, 2 * TILE:] = True                   # the one-pixel-wide tail tiles along the last axis only
    for name, mask in masks.items():
        mask_case(name, "tails", xt, yt, mt, mask)
    out["cases"] = np.array(names)
    path = os.path.join(ROOT, "tests", "golden", "metrics.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(names)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
