"""Kernel-level checks of the two-network cascade's launches against the existing entry points in the same process:
swn_cascade_resample (draws = swn_sample_pdf, union = torch.sort(cat), bit for bit) and swn_cascade_loss
(a float64 restatement; the degenerate case against swn_step_loss bit for bit)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(3, 2), (5, 3), (64, 96), (128, 192), (512, 512), (1021, 3)]


def dev():
    return torch.device("cuda:0")


def ops():
    from switch_nerf_amd import ops as _ops
    return _ops


def make_inputs(rng, N, S, F, weights, u):
    o = rng.uniform(-0.1, 0.1, (N, 3))
    d = rng.standard_normal((N, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d, np.full((N, 1), 0.05), np.full((N, 1), 1.0)], 1).astype(np.float32)
    z = np.sort(rng.uniform(0.05, 1.0, (N, S)).astype(np.float32), axis=1)
    if weights == "random":
        w = rng.uniform(0.0, 1.0, (N, S)).astype(np.float32) ** 4
    elif weights == "one_bin":                      # all the mass in one inner bin per ray
        w = np.zeros((N, S), np.float32)
        w[np.arange(N), rng.integers(1, S - 1, N)] = 0.9
    else:                                           # "zero": the 1e-8 floor alone shapes the pdf
        w = np.zeros((N, S), np.float32)
    if u == "none":
        uu = None
    elif u == "random":
        uu = rng.uniform(0.0, 1.0, (N, F)).astype(np.float32)
    elif u == "equal":
        uu = np.full((N, F), 0.37, np.float32)
    else:                                           # "runs": long runs of repeated draws (duplicate fine depths)
        uu = np.repeat(rng.uniform(0.0, 1.0, (N, (F + 6) // 7)).astype(np.float32), 7, axis=1)[:, :F].copy()
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev())
    return t(rays), t(z), t(w), t(uu)


@pytest.mark.parametrize("N", [1, 67])
@pytest.mark.parametrize("S,F", SHAPES)
def test_cascade_resample_bits(S, F, N):
    o = ops()
    rng = np.random.default_rng(1000 * S + F + N)
    for weights, u in (("random", "random"), ("random", "none"), ("one_bin", "runs"), ("zero", "equal"), ("one_bin", "random"),
                       ("zero", "random"), ("random", "runs")):
        rays, z, w, uu = make_inputs(rng, N, S, F, weights, u)
        zf_ref = o.sample_pdf(z, w, uu, F)
        zu_ref = torch.sort(torch.cat([z, zf_ref], -1), -1)[0].contiguous()
        zu, zf = o.cascade_resample(z, w, uu, F, want_z_fine=True)
        assert torch.equal(zf, zf_ref), (weights, u, "z_fine")
        assert torch.equal(zu, zu_ref), (weights, u, "z_union")
        zu2, zf2 = o.cascade_resample(z, w, uu, F)                       # without the optional output: the same union
        assert zf2 is None and torch.equal(zu2, zu_ref)


@pytest.mark.parametrize("S,F", [(513, 512), (2, 8), (8, 1)])
def test_cascade_resample_refuses(S, F):
    """Out-of-range sample counts are refused with the entry point's message and nothing is launched: the output keeps its sentinel."""
    from switch_nerf_amd import _lib
    o = ops()
    N = 4
    z = torch.linspace(0.1, 1.0, S, device=dev()).expand(N, S).contiguous()
    w = torch.ones(N, S, device=dev())
    with pytest.raises(RuntimeError, match="swn_cascade_resample: coarse samples >= 3, fine >= 2, coarse \\+ fine <= 1024"):
        o.cascade_resample(z, w, None, F)
    out = torch.full((N, S + F), -7.0, device=dev())
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = _lib.load().swn_cascade_resample(p(z), p(w), None, N, S, F, p(out), None, None)
    torch.cuda.synchronize()
    assert rc != 0 and bool((out == -7.0).all())


@pytest.mark.parametrize("coarse_photo", [True, False])
@pytest.mark.parametrize("gates", ["both", "none", "fine", "coarse"])
def test_cascade_loss_vs_float64(coarse_photo, gates):
    """out5 and the four gradient seeds against a float64 restatement of runner.py:1195-1211, at swn_step_loss's tolerances."""
    o = ops()
    g = torch.Generator(device="cpu").manual_seed(5)
    N, wt = 1000, 5e-4
    rf, rc, tgt = (torch.rand(N, 3, generator=g).to(dev()) for _ in range(3))
    lf = torch.rand(5, generator=g).to(dev()) if gates in ("both", "fine") else None
    lc = torch.rand(3, generator=g).to(dev()) if gates in ("both", "coarse") else None
    scale = torch.tensor([1024.0], device=dev())
    for sc in (None, scale):
        out5, d_f, d_c, d_lf, d_lc = o.cascade_loss(rf, rc, tgt, lf, lc, wt, coarse_photo, sc)
        s_ = 1.0 if sc is None else 1024.0
        photo = ((rf.double() - tgt.double()) ** 2).mean()
        coarse = ((rc.double() - tgt.double()) ** 2).mean()
        gate = ((lf.double().mean() if lf is not None else 0.0) + (lc.double().mean() if lc is not None else 0.0)) / 2
        loss = ((photo + coarse) / 2 if coarse_photo else photo) + wt * gate
        want = torch.stack([photo, coarse, torch.as_tensor(gate, dtype=torch.float64, device=dev()), loss, -10 * torch.log10(photo)]).float()
        assert (out5 - want).abs().max().item() <= 2e-6 * max(1.0, want.abs().max().item())
        share = 0.5 if coarse_photo else 1.0
        assert (d_f - (rf - tgt) * (2.0 * share * s_ / (3 * N))).abs().max().item() <= 1e-9 * s_ + 1e-7 * d_f.abs().max().item()
        if coarse_photo:
            assert (d_c - (rc - tgt) * (2.0 * 0.5 * s_ / (3 * N))).abs().max().item() <= 1e-9 * s_ + 1e-7 * d_c.abs().max().item()
        else:
            assert not d_c.any()                     # exact zeros
        assert (d_lf is None) == (lf is None) and (d_lc is None) == (lc is None)
        if lf is not None:
            assert torch.allclose(d_lf, torch.full_like(lf, wt * 0.5 / 5 * s_), rtol=1e-6)
        if lc is not None:
            assert torch.allclose(d_lc, torch.full_like(lc, wt * 0.5 / 3 * s_), rtol=1e-6)


def test_cascade_loss_degenerate_equals_step_loss():
    """rgb_coarse = rgb_fine with coarse_photo on: photo and psnr carry swn_step_loss's bits (the same summation order), and the two
    launches repeat their own bits."""
    o = ops()
    g = torch.Generator(device="cpu").manual_seed(6)
    for N in (1, 341, 4099):
        rgb, tgt = torch.rand(N, 3, generator=g).to(dev()), torch.rand(N, 3, generator=g).to(dev())
        la = torch.rand(4, generator=g).to(dev())
        out4 = o.step_loss(rgb, tgt, la, None, 5e-4)[0]
        out5 = o.cascade_loss(rgb, rgb.clone(), tgt, la, la.clone(), 5e-4, True)[0]
        assert torch.equal(out5[0], out4[0]) and torch.equal(out5[4], out4[3])
        assert torch.equal(out5[1], out5[0])
        assert torch.equal(o.cascade_loss(rgb, rgb.clone(), tgt, la, la.clone(), 5e-4, True)[0], out5)
