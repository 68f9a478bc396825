"""The image metrics restated in fp64 numpy: the yardstick of tests/test_metrics_cpu.py (pinned there on the reference's own floats,
tests/golden/metrics.npz) and of tests/test_metrics_gpu.py.

Written from the formula, not from the reference's text.  An image pair x, y [A, B, C] (channels last); a normalised window w of odd
length 2 h + 1 (the reference's fp32 taps, cast up); both images padded with h zeros on every side of the two spatial axes.
    blur(z)[a, b, c] = sum_i sum_j w[i] w[j] z_pad[a + i, b + j, c]                (the pass along B, then the pass along A)
    mu0 = blur(x), mu1 = blur(y), s00 = max(blur(x^2) - mu0^2, 0), s11 = max(blur(y^2) - mu1^2, 0), r = blur(x y) - mu0 mu1
    s01 = sign(r) min(sqrt(s00 s11), |r|)
    map = (2 mu0 mu1 + c1) (2 s01 + c2) / ((mu0^2 + mu1^2 + c1) (s00 + s11 + c2)),  c1 = (k1 max_val)^2, c2 = (k2 max_val)^2
ssim = mean(map); mse = mean((x - y)^2); psnr = -10 log10(mse); the masked forms: the same means over the pixels a boolean mask
[A, B] selects, all channels of those pixels (nan for a mask that selects nothing).
"""
import numpy as np

# profiles/r23_metrics.md, "The reference's own error": the largest |reference fp32 on the CPU - this restatement| over every case of
# tests/golden/metrics.npz, for the scalars (ssim, mse and their masked forms) and for the ssim map, rounded up in the last digit
# (test_metrics_cpu.py re-measures both).  The kernel is allowed 4 x that - its summation order is neither conv2d's nor torch.mean's -
# plus one fp32 ulp of 1.0 for the cases where the reference's error is exactly 0.
REF_ERR_SCALAR = 2.68e-6
REF_ERR_MAP = 2.97e-5
ULP_ONE = 2.0 ** -23
BOUND_SCALAR = 4 * REF_ERR_SCALAR + ULP_ONE
BOUND_MAP = 4 * REF_ERR_MAP + ULP_ONE


def blur(z, w):
    """z [A, B, C] fp64, w [2 h + 1] -> the zero-padded separable blur, same shape."""
    w = np.asarray(w, dtype=np.float64)
    h = w.size // 2
    assert w.size % 2 == 1
    A, B, _ = z.shape
    pad = np.pad(z, ((0, 0), (h, h), (0, 0)))
    along_b = sum(w[j] * pad[:, j:j + B] for j in range(w.size))
    pad = np.pad(along_b, ((h, h), (0, 0), (0, 0)))
    return sum(w[i] * pad[i:i + A] for i in range(w.size))


def ssim_map(x, y, w, max_val=1.0, k1=0.01, k2=0.03):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    assert x.shape == y.shape and x.ndim == 3
    c1, c2 = (k1 * max_val) ** 2, (k2 * max_val) ** 2
    mu0, mu1 = blur(x, w), blur(y, w)
    s00 = np.maximum(blur(x * x, w) - mu0 * mu0, 0.0)
    s11 = np.maximum(blur(y * y, w) - mu1 * mu1, 0.0)
    r = blur(x * y, w) - mu0 * mu1
    s01 = np.sign(r) * np.minimum(np.sqrt(s00 * s11), np.abs(r))
    return (2 * mu0 * mu1 + c1) * (2 * s01 + c2) / ((mu0 * mu0 + mu1 * mu1 + c1) * (s00 + s11 + c2))


def _psnr(mse):
    with np.errstate(divide="ignore"):
        return float(-10.0 * np.log10(mse))


def metrics(x, y, w, mask=None, max_val=1.0, k1=0.01, k2=0.03):
    """-> dict: map [A, B, C], ssim, mse, psnr and, with a mask, ssim_mask, mse_mask, psnr_mask (Python floats, fp64)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    m = ssim_map(x, y, w, max_val, k1, k2)
    se = (x - y) ** 2
    res = {"map": m, "ssim": float(m.mean()), "mse": float(se.mean())}
    res["psnr"] = _psnr(res["mse"])
    if mask is not None:
        mask = np.asarray(mask).astype(bool)
        assert mask.shape == x.shape[:2]
        if mask.any():
            res["ssim_mask"], res["mse_mask"] = float(m[mask].mean()), float(se[mask].mean())
            res["psnr_mask"] = _psnr(res["mse_mask"])
        else:
            res["ssim_mask"] = res["mse_mask"] = res["psnr_mask"] = float("nan")
    return res
