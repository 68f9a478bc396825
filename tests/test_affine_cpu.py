"""affine_appearance (models/nerf_moe.py:153-161, 436-438) without a GPU: the parameter / checkpoint layout against the reference model's
own named_parameters() list (recorded in the fixtures), the combinations that are not built, and the exported entry points."""
import ctypes
import os

import numpy as np
import pytest
import torch

import affine_weights as aw
import synth

G = os.path.join(os.path.dirname(__file__), "golden")
NEW_SYMBOLS = ("swn_affine_ray_fwd", "swn_affine_ray_bwd", "swn_affine_ray_bwd_workspace_bytes", "swn_heads_affine_fwd",
               "swn_heads_affine_bwd", "swn_heads_affine_bwd_workspace_bytes")


def _host_model(cfg=None, **kw):
    from switch_nerf_amd.model import SwitchNeRF
    return SwitchNeRF(aw.affine_cfg() if cfg is None else cfg, dtype=torch.float32, device="cpu", **kw)


@pytest.mark.parametrize("fixture", ["model_fwd_affine", "render_train_affine", "render_train_affine_mip"])
def test_state_dict_keys_and_shapes_equal_the_reference_models(fixture):
    g = np.load(os.path.join(G, fixture + ".npz"))
    sd = _host_model().state_dict()
    names = [str(n) for n in g["names"]]
    assert list(sd.keys()) == names                       # the same keys in the order the reference registers them
    for n in names:
        assert tuple(sd[n].shape) == tuple(int(v) for v in g["pshape__" + n]), n
    M = synth.BUILDING["model_dim"]
    assert sd["layers.2.fcs.0.weight"].shape == (128, M + 27) and sd["affine.weight"].shape == (12, 48) and sd["affine.bias"].shape == (12,)
    assert [n for n, _ in _host_model().named_parameters()] == names


def test_switch_off_layout_is_untouched_and_affine_parameters_sit_in_the_dense_prefix():
    from switch_nerf_amd.model import SwitchNeRF
    off = SwitchNeRF(synth.BUILDING, dtype=torch.float32, device="cpu")
    assert not off.affine and "affine.w" not in off.spec and "affine.weight" not in off.state_dict()
    assert off.spec["l2r.w"][1] == (27 + 48, 128)
    off2 = SwitchNeRF(dict(synth.BUILDING, affine_appearance=False), dtype=torch.float32, device="cpu")
    assert off2.spec == off.spec and off2.n_dense == off.n_dense and off2.n_flat == off.n_flat
    on = _host_model()
    assert on.affine and on.n_ray_feat == 27 and on.spec["l2r.w"][1] == (27, 128)
    for k in ("affine.w", "affine.b"):
        o, shape = on.spec[k]
        assert o + int(np.prod(shape)) <= on.n_dense, "all-reduced with the dense prefix under expert parallelism, never sharded"
    assert on.spec["exp0.w"][0] >= on.n_dense
    assert not (on.sw["fused_heads"] or on.sw["fused_tail"] or on.sw["fused_tail_bwd"])      # the heads run as their own launches
    with pytest.raises(ValueError, match="affine_appearance"):
        on.set_kernel_switches(fused_heads=True)


def test_load_state_dict_and_checkpoint_file_round_trip_keep_the_affine_parameters(tmp_path):
    from switch_nerf_amd import checkpoint
    sd = aw.make_affine_weights(7)
    a = _host_model()
    a.load_state_dict(sd)
    got = a.state_dict()
    for k, v in sd.items():
        assert np.array_equal(got[k].numpy(), v), k
    a.m.normal_(generator=torch.Generator().manual_seed(1)); a.v.uniform_(generator=torch.Generator().manual_seed(2)); a.step_count = 5
    path = str(tmp_path / "affine.pt")
    checkpoint.save_checkpoint(path, a, iteration=5)
    keys = [k[len("module."):] if k.startswith("module.") else k for k in torch.load(path, weights_only=False)["model_state_dict"]]
    assert "affine.weight" in keys and "affine.bias" in keys
    b = _host_model(seed=3)
    assert not torch.equal(b.p["affine.w"], a.p["affine.w"])
    checkpoint.load_checkpoint(path, b)
    assert torch.equal(b.flat, a.flat) and b.step_count == 5
    for buf in ("m", "v"):                                 # (per tensor: the padding between tensors is not part of a checkpoint)
        ma, mb = a._to_ref_layout(a._views(getattr(a, buf))), b._to_ref_layout(b._views(getattr(b, buf)))
        assert all(torch.equal(ma[k], mb[k]) for k in ma) and ma["affine.weight"].abs().sum() > 0
    # the seqexperts layout (what the reference's evaluation loads) carries them through unchanged
    c = _host_model(seed=4)
    c.load_state_dict(a.state_dict(layout="seqexperts"))
    assert torch.equal(c.flat, a.flat)


def test_unsupported_combinations_raise_naming_affine_appearance():
    from argparse import Namespace
    from switch_nerf_amd.background import BackgroundScene
    from switch_nerf_amd.dense import DenseNeRF
    from switch_nerf_amd.parallel import ExpertParallel
    from switch_nerf_amd.rendering import render_rays, render_rays_mip
    with pytest.raises(NotImplementedError, match="affine_appearance"):
        DenseNeRF(dict(synth.DENSE, affine_appearance=True), dtype=torch.float32, device="cpu")
    on, off = _host_model(), _host_model(synth.BUILDING)
    bg = DenseNeRF(synth.DENSE_BG, dtype=torch.float32, device="cpu")
    with pytest.raises(NotImplementedError, match="affine_appearance"):
        BackgroundScene(on, bg)
    BackgroundScene(off, bg)                               # (the switch off: as before)
    for kw in (dict(owner_tail=True), dict(), dict(padded=True)):
        with pytest.raises(NotImplementedError, match="affine_appearance"):
            on.set_expert_parallel(ExpertParallel(0, 1, 8, **kw))
    assert on.ep is None
    rays, img = torch.zeros(4, 8), torch.zeros(4, dtype=torch.long)
    hp = dict(coarse_samples=8, fine_samples=0, model_chunk_size=32, perturb=0.0)
    for model, flag in ((on, False), (off, True)):
        with pytest.raises(NotImplementedError, match="affine_appearance"):
            render_rays(model, None, rays, img, Namespace(affine_appearance=flag, **hp))
        with pytest.raises(NotImplementedError, match="affine_appearance"):
            render_rays_mip(model, rays, torch.zeros(4, 1), img, Namespace(affine_appearance=flag, **hp))
    with pytest.raises(NotImplementedError, match="affine_appearance"):          # an hparams without the key says "off"
        render_rays(on, None, rays, img, Namespace(**hp))


def test_affine_without_an_appearance_embedding_is_refused_at_construction():
    with pytest.raises(ValueError, match="appearance_dim"):
        _host_model(dict(synth.BUILDING, affine_appearance=True, appearance_dim=0))


def test_new_entry_points_are_declared_bound_and_exported_by_both_builds():
    from switch_nerf_amd import _lib
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.LIB_PATH_F16)):
        import __graft_entry__
        __graft_entry__.build()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "swn.h")).read()
    for path in (_lib.LIB_PATH, _lib.LIB_PATH_F16):
        lib = ctypes.CDLL(path)
        for s in NEW_SYMBOLS:
            assert hasattr(lib, s), f"{s} not exported by {os.path.basename(path)}"
            assert s in _lib.SIGNATURES and (s + "(") in header


def test_argument_validation_of_the_new_entry_points_without_a_gpu():
    from switch_nerf_amd import _lib
    lib = _lib.load()
    err = lambda: lib.swn_last_error().decode()
    p = ctypes.c_void_p(64)
    nb = ctypes.c_size_t(0)
    assert lib.swn_heads_affine_bwd_workspace_bytes(65, 256, 128, 13, ctypes.byref(nb)) == 0 and nb.value == 5 * (256 + 384 + 4) * 4
    assert lib.swn_heads_affine_fwd(p, p, _lib.F32, p, p, p, p, None, p, 7, 65, 256, 128, p, None) != 0 and "rows_per_group" in err()
    assert lib.swn_heads_affine_fwd(p, p, _lib.F32, p, p, p, p, None, None, 13, 65, 256, 128, p, None) != 0 and "null pointer" in err()
    assert lib.swn_heads_affine_fwd(p, p, _lib.F32, p, p, p, p, None, p, 13, 65, 64, 128, p, None) != 0 and "model_dim" in err()
    args = (None, p, _lib.F32, p, p, p, p, p, 65, 256, 128)
    assert lib.swn_heads_affine_bwd(*args, 0, p, p, p, p, p, p, None, p, p, nb.value, None) != 0 and "rows_per_group" in err()
    assert lib.swn_heads_affine_bwd(*args, 13, p, p, p, p, p, p, None, p, p, nb.value - 4, None) != 0 and "workspace" in err()
    assert lib.swn_heads_affine_bwd(*args, 13, p, p, p, p, p, p, None, None, p, nb.value, None) != 0 and "null pointer" in err()
    assert lib.swn_affine_ray_fwd(p, 0, p, 1, p, p, 5, p, None) != 0 and "bad sizes" in err()
    assert lib.swn_affine_ray_fwd(p, 48, p, 1, p, p, 0, p, None) == 0              # no rays: nothing launched
    assert lib.swn_affine_ray_bwd_workspace_bytes(65, 48, ctypes.byref(nb)) == 0 and nb.value == 2 * (12 * 48 + 12) * 4
    assert lib.swn_affine_ray_bwd(p, p, 48, p, 1, p, 65, p, p, p, p, nb.value - 4, None) != 0 and "workspace" in err()
