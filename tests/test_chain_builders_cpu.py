"""The expert chain's rules, each defined once in ops.py (expert_fwd_layers, expert_bwd_layers, expert_wgrad_items, expert_geometry and
the two Layer copies): what every layer of the forward, backward and weight-gradient lists carries, for L = 1 (a boundary no caller
exercises), 2 and 7 layers, with and without the skip, saving and not.  Layer only stores attributes: placeholder CPU tensors do."""
import pytest
import torch

from switch_nerf_amd import ops


def _t():
    return torch.zeros(1)


def _chain(L, saving):
    w, b, wb = [_t() for _ in range(L)], [_t() for _ in range(L)], [_t() for _ in range(L)]
    saves = [_t() if saving else None for _ in range(L - 1)]
    masks = [_t() if saving else None for _ in range(L - 1)]
    return w, b, wb, saves, masks


@pytest.mark.parametrize("saving", [True, False])
@pytest.mark.parametrize("skips", [(), (3,)])
@pytest.mark.parametrize("L", [1, 2, 7])
def test_forward_layer_list(L, skips, saving):
    w, b, _wb, saves, masks = _chain(L, saving)
    layers = ops.expert_fwd_layers(w, b, set(skips), saves, masks)
    assert len(layers) == L
    for l, ly in enumerate(layers):
        last = l == L - 1
        assert ly.w is w[l] and ly.b is b[l]
        assert ly.relu == (0 if last else 1)
        assert ly.skip == (1 if l in skips else 0)
        assert ly.save is (None if last else saves[l]) and ly.mask is (None if last else masks[l])
        assert (ly.save is not None) == (saving and not last) and (ly.mask is not None) == (saving and not last)
        assert ly.rowbias is None and ly.rows_per_bias == 0
    if L == 1:
        assert layers[0].save is None and layers[0].mask is None and layers[0].relu == 0


@pytest.mark.parametrize("L", [1, 2, 7])
def test_backward_layer_list(L):
    _w, _b, wb, _saves, masks = _chain(L, True)
    dz = [_t() for _ in range(L - 1)]
    bl = ops.expert_bwd_layers(wb, masks, dz)
    assert len(bl) == L
    for i, ly in enumerate(bl):
        l = L - 1 - i                                   # launch order: the last layer first
        assert ly.w is wb[l] and ly.b is None and ly.skip == 0
        if l > 0:
            assert ly.relu == 2 and ly.mask is masks[l - 1] and ly.save is dz[l - 1]
        else:
            assert ly.relu == 0 and ly.mask is None and ly.save is None
    if L == 1:                                          # one plain layer: no mask, no save, no ReLU backward
        assert (bl[0].relu, bl[0].mask, bl[0].save) == (0, None, None)


@pytest.mark.parametrize("gathers", ["none", "a", "both"])
@pytest.mark.parametrize("L", [1, 2, 7])
def test_wgrad_items(L, gathers):
    _w, _b, _wb, saves, _masks = _chain(L, True)
    dz, x_first, dz_last = [_t() for _ in range(L - 1)], _t(), _t()
    dw, db = [_t() for _ in range(L)], [_t() for _ in range(L)]
    ag = _t() if gathers in ("a", "both") else None
    bg = _t() if gathers == "both" else None
    items = ops.expert_wgrad_items(x_first, saves, dz, dz_last, dw, db, a_gather=ag, b_gather=bg)
    assert len(items) == L
    for l, (a, bz, w_, b_, a_g, b_g) in enumerate(items):
        assert a is (x_first if l == 0 else saves[l - 1])          # layer 0 reads the chain's input rows
        assert bz is (dz_last if l == L - 1 else dz[l])             # layer L - 1 reads the last dZ
        assert w_ is dw[l] and b_ is db[l]
        assert a_g is (ag if l == 0 else None)                      # each gather on the side that owns it
        assert b_g is (bg if l == L - 1 else None)
    assert ops.expert_wgrad_items(x_first, saves, dz, dz_last, dw, db)[0][4:] == (None, None)


def test_expert_geometry_both_sides_of_each_condition():
    bf16, f16, f32 = torch.bfloat16, torch.float16, torch.float32
    for rows, want in ((255, 1), (256, 7)):
        assert ops.expert_geometry(256, bf16, rows) == want
        assert ops.expert_geometry(256, f16, rows) == want
        assert ops.expert_geometry(256, bf16, rows, preferred=4) == (4 if want == 7 else 1)
        assert ops.expert_geometry(256, f32, rows) == 1             # fp32: the 64-row kernels
        assert ops.expert_geometry(128, bf16, rows) == 1            # another width
        assert ops.expert_geometry(512, bf16, rows) == 1
    assert ops.expert_geometry(256, bf16, 1 << 20) == 7


def test_layer_copies():
    m = torch.arange(12, dtype=torch.int32)
    ly = ops.Layer(_t(), _t(), relu=1, skip=True, save=_t(), mask=m, rowbias=_t(), rows_per_bias=64)
    a = ly.without_saves()
    assert a.save is None and a.mask is None
    assert (a.w, a.b, a.relu, a.skip, a.rowbias, a.rows_per_bias) == (ly.w, ly.b, 1, 1, ly.rowbias, 64)
    s = ly.with_mask_words(4, 8)
    assert torch.equal(s.mask, m[4:8]) and s.mask.data_ptr() == m[4:].data_ptr() and s.save is ly.save
    assert (s.w, s.b, s.relu, s.skip, s.rowbias, s.rows_per_bias) == (ly.w, ly.b, 1, 1, ly.rowbias, 64)
    assert ly.mask is m and ly.save is not None                     # the original is untouched
    assert ops.Layer(_t()).with_mask_words(0, 4).mask is None
