"""CPU-only: the host side of the padded form of Mega-NeRF joint training (switch_nerf_amd.mega.MegaNeRF cell_capacity,
switch_nerf_amd.graph.GraphedMegaStep) - the keyword's validation, what the padded form refuses, and that the compact form still refuses
graph capture.  Nothing here touches a device: every check fires before the first launch."""
import inspect

import numpy as np
import pytest
import torch

import synth

CFG = dict(layer_dim=256, layers=2, skip_layers=(1,), pos_xyz_dim=3, pos_dir_dim=2, appearance_dim=8, appearance_count=4, xyz_dim=3)
CEN = np.array([[-0.5, -0.4, 0.1], [0.5, -0.3, -0.2], [0.0, 0.5, 0.3]], np.float32)


def _subs(cfg=CFG, dtype=torch.float32):
    from switch_nerf_amd.dense import DenseNeRF
    subs = []
    for i in range(3):
        m = DenseNeRF(cfg, dtype=dtype, device="cpu")
        if cfg.get("sh_deg") is None:
            m.load_state_dict(synth.make_dense_weights(501 + i, cfg))
        subs.append(m)
    return subs


def _model(**kw):
    from switch_nerf_amd.mega import MegaNeRF
    return MegaNeRF(_subs(), CEN, 1.0, False, False, joint_training=True, **kw)


def test_cell_capacity_keyword_and_its_validation():
    from switch_nerf_amd.mega import MegaNeRF
    for f in (MegaNeRF.forward_points, MegaNeRF.grad_step, MegaNeRF.train_step):
        assert inspect.signature(f).parameters["cell_capacity"].default is None
    assert inspect.signature(MegaNeRF.apply_step).parameters["res"].default is None
    m = _model()
    assert m._capacity(None) is None and m._capacity(5) == (5, 5) and m._capacity((7, 3)) == (7, 3) and m._capacity([1, 2]) == (1, 2)
    x, rays, img = torch.zeros(4, 7), torch.zeros(4, 8), torch.zeros(4, dtype=torch.long)
    for bad in (0, -3, 1.5, "8", True, (4,), (4, 4, 4), (4, 0), (4, 2.0), ()):
        with pytest.raises(ValueError, match="cell_capacity"):
            m.forward_points(x, cell_capacity=bad)
        with pytest.raises(ValueError, match="cell_capacity"):
            m.grad_step(x[:, :3], rays, img, 2, cell_capacity=bad)
        with pytest.raises(ValueError, match="cell_capacity"):
            m.train_step(x[:, :3], rays, img, 2, cell_capacity=bad)


def test_what_the_padded_form_refuses():
    from switch_nerf_amd import graph
    from switch_nerf_amd.mega import MegaNeRF
    x, rays, img = torch.zeros(4, 4), torch.zeros(4, 8), torch.zeros(4, dtype=torch.long)
    sh = MegaNeRF(_subs(dict(CFG, pos_dir_dim=0, sh_deg=1)), CEN, 1.0, False, False, joint_training=True, sh_training=True)
    with pytest.raises(NotImplementedError, match="cell_capacity.*spherical-harmonics"):
        sh.forward_points(x, dirs=torch.zeros(4, 3), cell_capacity=8)
    with pytest.raises(NotImplementedError, match="cell_capacity.*spherical-harmonics"):
        sh.train_step(x[:, :3], rays, img, 2, cell_capacity=(8, 4))
    with pytest.raises(NotImplementedError, match="cell_capacity.*spherical-harmonics"):
        graph.GraphedMegaStep(sh, x[:, :3], rays, img, 2, 8)
    # what joint training refuses stays refused, whatever the form: at construction ...
    with pytest.raises(NotImplementedError, match="xyz_real"):
        MegaNeRF(_subs(dict(CFG, xyz_dim=4)), CEN, 1.0, True, False, joint_training=True)
    with pytest.raises(NotImplementedError, match="fp16"):
        MegaNeRF(_subs(dtype=torch.float16), CEN, 1.0, False, False, joint_training=True)
    m = _model()
    with pytest.raises(NotImplementedError, match="device noise"):
        m.set_device_noise(7)
    with pytest.raises(NotImplementedError, match="accumulation"):
        m.set_accumulation(2)
    with pytest.raises(NotImplementedError, match="finite guard"):
        m.set_check_finite(True)
    # ... and in the tail a padded step ends with
    res = dict(cell_overflow=None)
    with pytest.raises(NotImplementedError, match="data parallelism"):
        m.apply_step(lambda flat: 1.0, True, res)
    m.sub_modules[1].accum_steps = 2
    with pytest.raises(NotImplementedError, match="accumulation"):
        m.apply_step(None, True, res)
    m.sub_modules[1].accum_steps = 1
    m.sub_modules[2].check_finite = True
    with pytest.raises(NotImplementedError, match="finite guard"):
        m.apply_step(None, True, res)
    # the graphed step: joint training only, and a capacity is required
    with pytest.raises(NotImplementedError, match="inference only"):
        graph.GraphedMegaStep(MegaNeRF(_subs(), CEN, 1.0, False, False), x[:, :3], rays, img, 2, 8)
    with pytest.raises(ValueError, match="cell_capacity is required"):
        graph.GraphedMegaStep(_model(), x[:, :3], rays, img, 2, None)
    with pytest.raises(ValueError, match="cell_capacity"):
        graph.GraphedMegaStep(_model(), x[:, :3], rays, img, 2, 0)


def test_overflow_is_refused_before_anything_is_touched():
    """apply_step(res=...) with a non-zero overflow pair raises, naming the capacity and the true counts, with the step count and every
    parameter as they were; a zero pair with optimizer_step=False returns having touched nothing."""
    m = _model()
    before = {k: v.clone() for k, v in m.named_parameters()}
    ctx = dict(C=768, counts=torch.tensor([2048, 0, 0], dtype=torch.int32))
    res = dict(cell_overflow=torch.tensor([1280, 0], dtype=torch.int32), ctx=ctx)
    with pytest.raises(RuntimeError, match=r"1280 .*cell capacity 768.*\[2048, 0, 0\]"):
        m.apply_step(None, True, res)
    fine = dict(C=384, counts=torch.tensor([380, 390, 254], dtype=torch.int32))
    res = dict(cell_overflow=torch.tensor([0, 6], dtype=torch.int32), ctx=dict(ctx, counts=torch.tensor([700, 700, 648])), ctx_fine=fine)
    with pytest.raises(RuntimeError, match=r"fine: cell capacity 384.*\[380, 390, 254\]"):
        m.apply_step(None, False, res)
    assert m.step_count == 0 and all(s.step_count == 0 for s in m.sub_modules)
    for k, v in m.named_parameters():
        assert torch.equal(v, before[k]), k
    m.apply_step(None, False, dict(cell_overflow=torch.zeros(2, dtype=torch.int32), ctx=ctx))
    assert m.step_count == 0


def test_compact_form_still_refuses_capture_and_the_padded_form_does_not(monkeypatch):
    m = _model()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(NotImplementedError, match="graph capture is not built - counts.tolist\\(\\) sizes the ragged per-cell calls on the host"):
        m.forward_points(torch.zeros(4, 7))
    with pytest.raises(NotImplementedError, match="graph capture is not built"):
        m.forward_points(torch.zeros(4, 7), cell_capacity=None)
    # the padded form passes that line: it gets as far as the shape check behind it
    with pytest.raises(Exception, match="Unexpected input shape"):
        m.forward_points(torch.zeros(4, 6), cell_capacity=8)


def test_documents_say_what_is_out_of_scope():
    from switch_nerf_amd import graph, mega
    doc = " ".join(mega.__doc__.split())
    assert "graph capture of the COMPACT form" in doc and "GraphedMegaStep" in doc
    gdoc = " ".join(graph.GraphedMegaStep.__doc__.split())
    for word in ("spherical-harmonics", "seeded device noise", "data parallelism", "xyz_real", "grouped launch"):
        assert word in gdoc and word in doc, word
