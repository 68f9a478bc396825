"""fp64 (or any torch dtype) restatement of the spherical-harmonics colour path: the basis, the heads (swn_heads_sh_fwd / _bwd's
contract), and the dense NeRF module with rgb_dim = 3 (d + 1)^2 (models/nerf.py:143-191 with pos_dir_dim = 0).  Written from the
formulas, independent of the kernels; tests/test_sh_cpu.py pins it on the reference's own outputs (tests/golden/sh_*.npz)."""
from __future__ import annotations

import torch

# real spherical harmonics, degree l -> the constants of its 2 l + 1 polynomials (sign included)
K0 = 0.28209479177387814
K1 = 0.4886025119029199
K2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
K3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
      -0.5900435899266435)
K4 = (2.5033429417967046, -1.7701307697799304, 0.9461746957575601, -0.6690465435572892, 0.10578554691520431, -0.6690465435572892,
      0.47308734787878004, -1.7701307697799304, 0.6258357354491761)


def basis(deg: int, dirs: torch.Tensor) -> torch.Tensor:
    """Y [N, (deg + 1)^2] at dirs [N, 3], taken as given (not normalised)."""
    assert 0 <= deg <= 4
    x, y, z = dirs[:, 0], dirs[:, 1], dirs[:, 2]
    out = [torch.full_like(x, K0)]
    if deg > 0:
        out += [-K1 * y, K1 * z, -K1 * x]
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        out += [K2[0] * xy, K2[1] * yz, K2[2] * (2 * zz - xx - yy), K2[3] * xz, K2[4] * (xx - yy)]
    if deg > 2:
        out += [K3[0] * y * (3 * xx - yy), K3[1] * xy * z, K3[2] * y * (4 * zz - xx - yy), K3[3] * z * (2 * zz - 3 * xx - 3 * yy),
                K3[4] * x * (4 * zz - xx - yy), K3[5] * z * (xx - yy), K3[6] * x * (xx - 3 * yy)]
    if deg > 3:
        out += [K4[0] * xy * (xx - yy), K4[1] * yz * (3 * xx - yy), K4[2] * xy * (7 * zz - 1), K4[3] * yz * (7 * zz - 3),
                K4[4] * (zz * (35 * zz - 30) + 3), K4[5] * xz * (7 * zz - 3), K4[6] * (xx - yy) * (7 * zz - 1),
                K4[7] * xz * (xx - 3 * yy), K4[8] * (xx * (xx - 3 * yy) - yy * (3 * xx - yy))]
    return torch.stack(out, 1)


def eval_sh(deg: int, coef: torch.Tensor, dirs: torch.Tensor) -> torch.Tensor:
    """coef [N, 3, B], dirs [N, 3] -> [N, 3]."""
    return (coef * basis(deg, dirs)[:, None, :]).sum(-1)


def softplus_shifted(u):
    """F.softplus(u - 1, threshold 20) (models/nerf.py:68-69)."""
    v = u - 1
    return torch.where(v > 20, v, torch.log1p(torch.exp(torch.clamp(v, max=20))))


def heads_fwd(y, h2, ws, bs, wc, bc, noise, dirs, rows_per_group: int, deg: int):
    """-> (raw [P, 4], lin [P, 3 B]) in the dtype of the (already widened) inputs; rows i belongs to ray i // rows_per_group."""
    P, B = y.shape[0], (deg + 1) ** 2
    lin = h2 @ wc.t() + bc
    Y = basis(deg, dirs).repeat_interleave(rows_per_group, 0)              # [P, B]
    rgb = torch.sigmoid((lin.view(P, 3, B) * Y[:, None, :]).sum(-1))
    u = y @ ws + bs + (noise if noise is not None else 0)
    return torch.cat([rgb, softplus_shifted(u)[:, None]], 1), lin


def heads_bwd(y, h2, ws, bs, wc, bc, noise, dirs, rows_per_group: int, deg: int, d_raw):
    """The kernel's outputs from the formulas: dh2 = (d_lin Wc) masked by h2 > 0 (h2 is a ReLU's output: the gradient reaches its
    pre-activation), dsig = d_raw_sigma softplus'(u), the four parameter gradients, and the per-ray column sums of dh2."""
    P, B = y.shape[0], (deg + 1) ** 2
    raw, _ = heads_fwd(y, h2, ws, bs, wc, bc, noise, dirs, rows_per_group, deg)
    rgb = raw[:, :3]
    p = d_raw[:, :3] * rgb * (1 - rgb)
    Y = basis(deg, dirs).repeat_interleave(rows_per_group, 0)
    d_lin = (p[:, :, None] * Y[:, None, :]).reshape(P, 3 * B)
    u = y @ ws + bs + (noise if noise is not None else 0) - 1
    dsig = d_raw[:, 3] * torch.sigmoid(u)
    dh2 = (d_lin @ wc) * (h2 > 0)
    return dict(dh2=dh2, dsig=dsig, d_ws=dsig @ y, d_bs=dsig.sum(), d_wc=d_lin.t() @ h2, d_bc=d_lin.sum(0),
                colsum=dh2.view(P // rows_per_group, rows_per_group, -1).sum(1))


def embed(x, n_freqs: int):
    """models/nerf.py:21-26: (x, sin(2^k x), cos(2^k x), ...)."""
    out = [x]
    for k in range(n_freqs):
        out += [torch.sin((2.0 ** k) * x), torch.cos((2.0 ** k) * x)]
    return torch.cat(out, -1)


def module_forward(sd, cfg, x, sigma_noise=None, dtype=torch.float64):
    """The dense NeRF with rgb_dim = 3 B on x [P, 3 + 1] = position, image index -> [P, 3 B + 1] (raw coefficients, sigma).
    sd: {reference key: array}."""
    t = {k: torch.as_tensor(v).to(dtype) for k, v in sd.items()}
    enc = embed(torch.as_tensor(x[:, :3]).to(dtype), cfg["pos_xyz_dim"])
    h = enc
    for i in range(cfg["layers"]):
        if i in cfg["skip_layers"]:
            h = torch.cat([enc, h], -1)
        h = torch.relu(h @ t[f"xyz_encodings.{i}.0.weight"].t() + t[f"xyz_encodings.{i}.0.bias"])
    u = h @ t["sigma.weight"].t() + t["sigma.bias"]
    if sigma_noise is not None:
        u = u + torch.as_tensor(sigma_noise).to(dtype).view(-1, 1)
    sigma = softplus_shifted(u)
    final = h @ t["xyz_encoding_final.weight"].t() + t["xyz_encoding_final.bias"]
    emb = t["embedding_a.weight"][torch.as_tensor(x[:, 3]).long()]
    h2 = torch.relu(torch.cat([final, emb], -1) @ t["dir_a_encoding.0.weight"].t() + t["dir_a_encoding.0.bias"])
    return torch.cat([h2 @ t["rgb.weight"].t() + t["rgb.bias"], sigma], -1)
