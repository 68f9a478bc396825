"""Fixture of the two-network cascade (switch_nerf_amd/cascade.py) from the REFERENCE's own Cascade (models/cascade.py, built by
models/model_utils.py:97-117 with use_cascade = True), its rendering.render_rays, its autograd and torch.optim.Adam, on the CPU.

Usage (build container only, like oracle/gen_golden.py whose helpers it uses):
    python scripts/gen_golden_cascade.py

Writes tests/golden/cascade_dense.npz, data only.  Weights are never stored: the coarse half is synth.make_dense_weights(seed), the fine
half synth.make_dense_weights(seed + 1); the file holds their checksums.  The dense cfg of dense_nerf_train.npz (synth.DENSE), 64 rays,
S = 32, F = 16, one model chunk; for perturb 0 (p0_*) and 1 (p1_*, the draws replayed from the seed and stored: p1_perturb_rand [N, S],
p1_fine_u [N, F]):
    rgb_coarse, rgb_fine, depth_fine, depth_variance_fine, keys (the result's key set)
    z_union [N, S + F]   what the fine half was called on (a forward pre-hook on it records the points; their depths are (x - o) . d in
                         float64, d being unit vectors)
    w_inner [N, S - 2]   the coarse weights _sample_pdf received (weights_coarse[:, 1:-1], recorded around the reference's own call)
    loss                 (mse(rgb_fine) + mse(rgb_coarse)) / 2, the form of Runner._training_step_nerf (runner.py:1195-1204)
    gsum__ / gslice__    per parameter of both halves (the format of dense_nerf_train.npz, keys coarse.<k> / fine.<k>), the slice
                         thinned to every `every_p0` / `every_p1`-th position (stored) for the file's size
eval_*: the evaluation-mode render (no gradients), and eval0_keys: the key set with fine_samples = 0 on a Cascade(coarse, None).
adam_p{1,2}_sums / _slices / adam_offsets: every parameter after one and two steps of torch.optim.Adam(lr 5e-4) on the perturb-0 case
(its step-1 gradient IS p0_gslice__), at every `every_adam`-th position of the gradient slices, packed in the order of param_names.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden as gg  # noqa: E402
import synth  # noqa: E402      (on the path through gen_golden)
from switch_nerf.models import model_utils  # noqa: E402
from switch_nerf.models.cascade import Cascade  # noqa: E402
from switch_nerf import rendering  # noqa: E402

N, S, FINE = 64, 32, 16
SEED, RAY_SEED, DRAW_SEED, LR, N_SLICE = 171, 172, 77, 5e-4, 499
EVERY_P0, EVERY_P1, EVERY_ADAM = 1, 16, 16


def sl(a):
    a = np.asarray(a).reshape(-1)
    return a[:: max(1, a.size // N_SLICE)][:N_SLICE].copy()


def build(perturb, fine=FINE):
    """The reference's Cascade of two dense NeRFs with the synth weights loaded -> (nerf, hparams, the halves' state dicts)."""
    cfg = synth.DENSE
    h = gg.make_hparams(synth.BUILDING, coarse=S, chunk=65536, perturb=perturb, fine=fine)
    h.use_moe, h.use_cascade, h.return_sigma, h.moe_return_gates = False, True, False, False
    h.layers, h.skip_layers, h.layer_dim = cfg["layers"], list(cfg["skip_layers"]), cfg["layer_dim"]
    torch.manual_seed(0)
    nerf = model_utils.get_nerf(h, cfg["appearance_count"])
    assert isinstance(nerf, Cascade) and (nerf.fine is None) == (fine == 0)
    sds = [synth.make_dense_weights(SEED + i, cfg) for i in range(2 if fine else 1)]
    sd = {f"{half}.{k}": torch.from_numpy(v.copy()) for half, part in zip(("coarse", "fine"), sds) for k, v in part.items()}
    assert set(sd) == set(nerf.state_dict()), sorted(set(sd) ^ set(nerf.state_dict()))
    nerf.load_state_dict(sd)
    return nerf, h, sds


def render(nerf, h, rays, img):
    """The reference's render_rays -> (results, z_union, the coarse weights _sample_pdf received)."""
    seen, w_in = [], []
    hook = nerf.fine.register_forward_pre_hook(lambda mod, args: seen.append(args[0].detach().numpy().copy())) if nerf.fine is not None else None
    orig = rendering._sample_pdf

    def recording_sample_pdf(bins, weights, *a, **k):
        w_in.append(weights.detach().numpy().copy())
        return orig(bins, weights, *a, **k)
    rendering._sample_pdf = recording_sample_pdf
    try:
        res, _ = rendering.render_rays(nerf, None, torch.from_numpy(rays), torch.from_numpy(img), h, None, None, get_depth=True,
                                       get_depth_variance=True, get_bg_fg_rgb=False)
    finally:
        rendering._sample_pdf = orig
        if hook is not None:
            hook.remove()
    zu = None
    if seen:
        x = np.concatenate(seen)[:, :3].astype(np.float64).reshape(len(rays), -1, 3)
        zu = ((x - rays[:, None, :3].astype(np.float64)) * rays[:, None, 3:6].astype(np.float64)).sum(-1).astype(np.float32)
    return res, zu, (w_in[0] if w_in else None)


def record(prefix, res, out):
    for k in ("rgb_coarse", "rgb_fine", "depth_fine", "depth_variance_fine"):
        out[prefix + k] = res[k].detach().numpy()
    out[prefix + "keys"] = np.array(sorted(res))


def step_loss(res, rgbs):
    t = torch.from_numpy(rgbs)
    return (torch.nn.functional.mse_loss(res["rgb_fine"], t) + torch.nn.functional.mse_loss(res["rgb_coarse"], t)) / 2


def gen_dense():
    out = dict(seed=SEED, ray_seed=RAY_SEED, draw_seed=DRAW_SEED, N=N, S=S, F=FINE, lr=LR, every_p0=EVERY_P0, every_p1=EVERY_P1,
               every_adam=EVERY_ADAM)
    rays, img, rgbs = synth.make_rays(RAY_SEED, N, synth.DENSE["appearance_count"])
    out.update(rays=rays, image_indices=img, rgbs=rgbs)
    for tag, perturb in (("p0_", 0.0), ("p1_", 1.0)):
        nerf, h, sds = build(perturb)
        nerf.train()
        if perturb > 0:      # the reference draws rand_like(z_vals) (rendering.py:583), then torch.rand(N, fine) (:608): replay the stream
            torch.manual_seed(DRAW_SEED)
            out[tag + "perturb_rand"], out[tag + "fine_u"] = torch.rand(N, S).numpy(), torch.rand(N, FINE).numpy()
            torch.manual_seed(DRAW_SEED)
        res, zu, w_in = render(nerf, h, rays, img)
        assert zu.shape == (N, S + FINE) and (np.diff(zu, axis=1) >= -1e-6).all() and w_in.shape == (N, S - 2)
        loss = step_loss(res, rgbs)
        loss.backward()
        record(tag, res, out)
        out[tag + "z_union"], out[tag + "w_inner"], out[tag + "loss"] = zu, w_in, loss.detach().numpy()
        every = EVERY_P0 if perturb == 0 else EVERY_P1
        for n, p in nerf.named_parameters():
            out[tag + "gsum__" + n] = synth.checksum(p.grad.numpy())
            out[tag + "gslice__" + n] = sl(p.grad.numpy())[::every]
        print(f"  ({tag[:2]}) loss {loss.item():.6f}, keys {sorted(res)}")
    out["param_names"] = np.array([n for n, _ in nerf.named_parameters()])
    out["sd_checksums"] = np.stack([synth.checksum(v) for part in sds for v in part.values()])
    # evaluation mode (perturb is 0 there: the depths of p0)
    nerf, h, _ = build(1.0)
    nerf.eval()
    with torch.no_grad():
        res, _, _ = render(nerf, h, rays, img)
    record("eval_", res, out)
    nerf0, h0, _ = build(0.0, fine=0)
    nerf0.eval()
    with torch.no_grad():
        res0, _, _ = render(nerf0, h0, rays, img)
    out["eval0_keys"], out["eval0_rgb_coarse"] = np.array(sorted(res0)), res0["rgb_coarse"].numpy()
    # two Adam steps on the perturb-0 case
    nerf, h, _ = build(0.0)
    nerf.train()
    opt = torch.optim.Adam(nerf.parameters(), lr=LR)
    for step in (1, 2):
        opt.zero_grad()
        res, _, _ = render(nerf, h, rays, img)
        loss = step_loss(res, rgbs)
        loss.backward()
        if step == 1:
            for n, p in nerf.named_parameters():
                assert np.array_equal(sl(p.grad.numpy())[::EVERY_P0], out["p0_gslice__" + n]), n
        opt.step()
        named = [(n, p.detach().numpy()) for n, p in nerf.named_parameters()]
        parts = [sl(a)[::EVERY_ADAM] for _, a in named]
        out[f"adam_p{step}_sums"] = np.stack([synth.checksum(a) for _, a in named])
        out[f"adam_p{step}_slices"] = np.concatenate(parts)
        out["adam_offsets"] = np.cumsum([0] + [len(q) for q in parts]).astype(np.int64)
        out[f"adam_loss{step}"] = loss.detach().numpy()
        print(f"  (adam) step {step}: loss {loss.item():.6f}")
    gg.save("cascade_dense", **out)


if __name__ == "__main__":
    os.makedirs(gg.OUT, exist_ok=True)
    torch.set_num_threads(8)
    print(f"[cascade] dense: {N} rays x ({S} coarse + {FINE} fine), perturb 0 / 1, eval, two Adam steps")
    gen_dense()
