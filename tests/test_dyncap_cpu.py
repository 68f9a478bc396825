"""CPU-only: the capacity rule of the dynamic MoE capacity (capacity_factor <= 0, tutel_fast_dispatch.py:210-216) in the layer mirror and
in SwitchNeRF, and the message of the expert-parallel refusal."""
import pytest


def test_layer_capacity_rule():
    from switch_nerf_amd.moe import layer_capacity
    # cf > 0: k * int(cf * ceil(P / E)), max_rows ignored
    assert layer_capacity(1.25, 1000, 8) == int(1.25 * 125)
    assert layer_capacity(1.0, 1001, 8, top_k=2, max_rows=7) == 2 * 126
    # cf = 0: max(loc) + 1 as given
    assert layer_capacity(0.0, 1000, 8, max_rows=190) == 190
    assert layer_capacity(0.0, 768, 8, top_k=2, max_rows=300) == 300
    # cf < 0: clamped at k * int(-cf * ceil(P / E))
    assert layer_capacity(-0.5, 1000, 8, max_rows=190) == 62
    assert layer_capacity(-0.5, 1000, 8, max_rows=40) == 40
    assert layer_capacity(-1.0, 768, 8, top_k=2, max_rows=500) == 192
    with pytest.raises(ValueError):
        layer_capacity(0.0, 1000, 8)


def test_model_capacity_rule():
    from switch_nerf_amd.model import SwitchNeRF
    m = SwitchNeRF.__new__(SwitchNeRF)       # (the rule only: no device state)
    m.E = 8
    for cf, seg, want in ((1.0, 65536, 8192), (1.25, 1000, 156), (0.0, 65536, 65536), (0.0, 1000, 1000), (-0.5, 65536, 4096),
                          (-1.25, 1000, 156)):
        m.cf = cf
        assert m.capacity(seg) == want, (cf, seg)


def test_expert_parallel_refusal_names_the_restriction():
    from switch_nerf_amd.model import DYNCAP_EP_ERROR, SwitchNeRF
    assert "capacity_factor = 0" in DYNCAP_EP_ERROR and "expert parallelism" in DYNCAP_EP_ERROR
    m = SwitchNeRF.__new__(SwitchNeRF)
    m.E, m.cf, m.ep = 8, 0.0, None

    class _EP:
        E = 8
    with pytest.raises(ValueError, match="not supported with expert parallelism"):
        m.set_expert_parallel(_EP())
    assert m.ep is None
    m.cf = -0.5                              # cf < 0 works through the static bound
    m.set_expert_parallel(_EP())
    assert m.ep is not None
