"""CPU-only: the pure-torch restatement of the Mega-NeRF cell router (tests/mega_restate.py, direct distances) pinned on the
reference's own results (tests/golden/mega_*.npz, scripts/gen_golden_mega.py), and the construction of switch_nerf_amd.mega.MegaNeRF
from state dicts and from a container.

The reference measures its distances with torch.cdist, which above 25 rows uses the |x|^2 + |c|^2 - 2 x.c form: its distances carry a
cancellation error (stored as dist_err, measured against float64), so a point within 4 x dist_err of a membership decision may fall on
either side.  Such points are left out of the membership and weight comparisons; the fixtures are chosen so that they are at most 1 %
(asserted here; the committed fixtures have none)."""
import os

import numpy as np
import pytest
import torch

import mega_restate as R
import synth

G = os.path.join(os.path.dirname(__file__), "golden")
CASES = [("mega_fg", "m100", 1.0), ("mega_fg", "m115", 1.15), ("mega_bg", "m115", 1.15)]


@pytest.mark.parametrize("name,tag,margin", CASES)
def test_restatement_vs_reference_golden(name, tag, margin):
    g = np.load(os.path.join(G, name + ".npz"))
    x, cen, ds = g["x"], g["centroids"], int(g["cluster_2d"])
    excluded = (R.boundary_gap(x, cen, ds, margin) <= 4 * float(g["dist_err"])).numpy()
    np.testing.assert_array_equal(excluded, g["excluded_" + tag])
    print(f"{name} {tag}: dist_err {float(g['dist_err']):.3e}, excluded {excluded.sum()} of {len(x)}")
    assert excluded.mean() <= 0.01
    keep = ~excluded
    w_ref = g["weights_" + tag]
    w = R.assign(x, cen, ds, margin).numpy()
    np.testing.assert_array_equal((w > 0)[keep], (w_ref > 0)[keep])
    err = np.abs(w - w_ref)[keep].max()
    print(f"  weights: max error {err:.3e}, bound {float(g['weights_tol']):.3e}")
    assert err <= float(g["weights_tol"])
    np.testing.assert_allclose(w.sum(1), 1.0, rtol=0, atol=1e-6)
    # the outputs, given the reference's per-cell outputs: its own weights reproduce its result exactly (same loop, same order) ...
    hard = margin == 1
    counts, begin, rows, slot = R.pack(w_ref)
    assert begin[-1] == len(g["sub_" + tag]) and (counts > 0).all()
    out = R.blend(w_ref, slot, begin, g["sub_" + tag], hard).numpy()
    np.testing.assert_array_equal(out, g["out_" + tag])
    # ... and the restated weights give it within the measured bound (where the membership is the same, the packing is too)
    same = ((w > 0) == (w_ref > 0)).all(1)
    w_mix = np.where(same[:, None], w, w_ref)
    out2 = R.blend(w_mix, slot, begin, g["sub_" + tag], hard).numpy()
    assert np.abs(out2 - g["out_" + tag])[keep].max() <= float(g["blend_tol"])
    # rows / slot are each other's inverse, rows ascend inside a cell
    for i in range(len(cen)):
        r = rows[begin[i]:begin[i + 1]]
        assert (np.diff(r) > 0).all() and (slot[r, i] == np.arange(len(r))).all()
    # the gathered rows are x[cluster_mask] of the reference (its column cut for xyz_real, its sigma-noise rows)
    col0 = 3 if int(g["xyz_real"]) else 0
    xin, nin = R.gather(x, rows, col0, g["sigma_noise"])
    m0 = w_ref[:, 0] > 0
    np.testing.assert_array_equal(xin[: counts[0]].numpy(), x[m0][:, col0:])
    np.testing.assert_array_equal(nin[: counts[0]].numpy(), g["sigma_noise"].reshape(-1)[m0])


def test_restatement_ties_and_cluster_2d():
    """Two identical centroids: the first index wins the hard assignment, both are members (equal weights) with a margin; cluster_2d
    ignores the first coordinate."""
    cen = np.array([[0.5, 0.0, 0.0], [0.5, 0.0, 0.0], [-0.5, 0.0, 0.0]], np.float32)
    x = np.array([[0.4, 0.1, 0.0], [-0.4, 0.0, 0.2]], np.float32)
    np.testing.assert_array_equal(R.assign(x, cen, 0, 1.0).numpy(), [[1, 0, 0], [0, 0, 1]])
    w = R.assign(x, cen, 0, 1.15).numpy()
    assert w[0, 0] == w[0, 1] == 0.5 and w[0, 2] == 0 and w[1, 2] == 1
    d2 = R.distances(x, cen, 1).numpy()
    np.testing.assert_allclose(d2[:, 0], d2[:, 2], rtol=0, atol=0)


class _StandInNeRF(torch.nn.Module):
    """The parameter layout of the reference's NeRF sub-models (key names and shapes only; it computes nothing)."""

    def __init__(self, cfg):
        super().__init__()
        W, xd = cfg["layer_dim"], cfg["xyz_dim"]
        in_xyz = xd + xd * 2 * cfg["pos_xyz_dim"]
        in_dir = 3 + 6 * cfg["pos_dir_dim"]
        lin = torch.nn.Linear
        self.xyz_encodings = torch.nn.ModuleList([
            torch.nn.Sequential(lin(in_xyz if i == 0 else (W + in_xyz if i in cfg["skip_layers"] else W), W), torch.nn.ReLU(True))
            for i in range(cfg["layers"])])
        self.embedding_a = torch.nn.Embedding(cfg["appearance_count"], cfg["appearance_dim"])
        self.xyz_encoding_final = lin(W, W)
        self.dir_a_encoding = torch.nn.Sequential(lin(W + in_dir + cfg["appearance_dim"], W // 2), torch.nn.ReLU(True))
        self.sigma = lin(W, 1)
        self.rgb = lin(W // 2, 3)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return x


class _StandInContainer(torch.nn.Module):
    """The attribute names of a merged Mega-NeRF container (model_utils.py:90-96)."""

    def __init__(self, fg, bg, centroids, cluster_2d):
        super().__init__()
        for i, m in enumerate(fg):
            setattr(self, f"sub_module_{i}", m)
        for i, m in enumerate(bg):
            setattr(self, f"bg_sub_module_{i}", m)
        self.register_buffer("centroids", centroids)
        self.cluster_2d = cluster_2d

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return x


CFG = dict(layer_dim=256, layers=2, skip_layers=(1,), pos_xyz_dim=3, pos_dir_dim=2, appearance_dim=8, appearance_count=4, xyz_dim=3)


def _stand_ins(seed, cfg, n):
    sds = [synth.make_dense_weights(seed + i, cfg) for i in range(n)]
    mods = []
    for sd in sds:
        m = _StandInNeRF(cfg)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
        mods.append(m)
    return sds, mods


def test_from_container_and_state_dicts_round_trip(tmp_path):
    from switch_nerf_amd.mega import MegaNeRF, dense_cfg_from_state_dict
    cfg_bg = dict(CFG, xyz_dim=4)
    cen = torch.tensor([[-0.5, -0.4, 0.1], [0.5, -0.3, -0.2], [0.0, 0.5, 0.3]])
    sds, fg = _stand_ins(401, CFG, 3)
    sds_bg, bg = _stand_ins(411, cfg_bg, 3)
    path = str(tmp_path / "container.pt")
    torch.jit.save(torch.jit.script(_StandInContainer(fg, bg, cen, True)), path)
    for background, want_sd, want_cfg in ((False, sds, CFG), (True, sds_bg, cfg_bg)):
        m = MegaNeRF.from_container(path, 1.15, background=background, device="cpu")
        assert m.xyz_real == background and m.cluster_dim_start == 1 and m.boundary_margin == 1.15 and len(m.sub_modules) == 3
        assert torch.equal(m.centroids, cen) and not m.training
        assert dense_cfg_from_state_dict(want_sd[0], want_cfg["xyz_dim"]) == want_cfg
        for sub, sd in zip(m.sub_modules, want_sd):
            assert {k: sub.cfg[k] for k in want_cfg} == want_cfg and not sub.training
            out = sub.state_dict()
            assert set(out) == set(sd)
            for k in sd:
                np.testing.assert_array_equal(out[k].numpy(), sd[k])
    m = MegaNeRF.from_state_dicts(sds, cen.numpy(), CFG, boundary_margin=1.0, device="cpu")
    assert m.cluster_dim_start == 0 and not m.xyz_real and m.boundary_margin == 1.0
    for got, sd in zip(m.state_dicts(), sds):
        for k in sd:
            np.testing.assert_array_equal(got[k].numpy(), sd[k])
    with pytest.raises(AssertionError):
        MegaNeRF(m.sub_modules, cen, 0.9, False, False)
    with pytest.raises(NotImplementedError, match="inference only"):
        m.train()
    with pytest.raises(TypeError, match="xyz_dim 4"):
        MegaNeRF(m.sub_modules, cen, 1.15, True, False)
