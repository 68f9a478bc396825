"""swn_chain_desc.x_k: the first layer of a persistent chain (geometry 7) run over its REAL K only, instead of all 256 columns of its
zero-padded weights.  The products left out are finite x 0 and the order of the others per accumulator is unchanged, so every output
of the launch must have the same BITS with and without the field - checked on the front forward chain (tag 3), the fused backward
(tag 8) and the separate tail backward (tag 5), bf16 and fp16 - and swn_mlp_chain must refuse the field where it means nothing."""
import pytest
import torch

pytestmark = pytest.mark.gpu

M, H2 = 256, 128


@pytest.fixture(params=["bf16", "f16"])
def half(request):
    from switch_nerf_amd import _lib
    _lib.use_half(request.param)
    yield torch.bfloat16 if request.param == "bf16" else torch.float16
    _lib.use_half("bf16")


def _ops():
    from switch_nerf_amd import ops
    return ops


def _dev():
    return torch.device("cuda")


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    va, vb = (a.view(torch.int16), b.view(torch.int16)) if a.element_size() == 2 else (a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(va, vb), f"{what}: {(va != vb).float().mean().item():.3g} of the elements differ"


@pytest.mark.parametrize("x_k", [80, 128])
@pytest.mark.parametrize("P", [256, 300, 64])
def test_front_forward_chain_same_bits(half, P, x_k):
    """Tag 3 on the model's front geometry (7): one full tile, a ragged second tile, less than one row group.  Encoding rows of 128
    columns with 75 real ones; the chain output, both saved activations and the ReLU mask words."""
    o, dt = _ops(), half
    g = torch.Generator().manual_seed(1000 + P)
    pe = torch.zeros(P, 128)
    pe[:, :75] = torch.randn(P, 75, generator=g)
    pe = pe.to(_dev()).to(dt)
    W0 = torch.zeros(1, 128, M)
    W0[:, :75] = torch.randn(1, 75, M, generator=g) / 9
    w0p = o.pack_weights_padded(W0.to(_dev()), dt, True, 256)
    w1 = o.pack_weights((torch.randn(1, M, M, generator=g) / 16).to(_dev()), dt, True)
    w2 = o.pack_weights((torch.randn(1, M, M, generator=g) / 16).to(_dev()), dt, True)
    b = [(torch.randn(1, M, generator=g) * 0.1).to(_dev()) for _ in range(3)]

    def run(xk):
        h0, a1, gg = (torch.full((P + 40, M), 3.0, dtype=dt, device=_dev()) for _ in range(3))
        mask = torch.zeros(o.chain_mask_words(dt, 1, P, M), dtype=torch.int32, device=_dev())
        o.mlp_chain(pe, [o.Layer(w0p, b[0], save=h0), o.Layer(w1, b[1], relu=1, mask=mask, save=a1), o.Layer(w2, b[2])], gg[:P],
                    tag=3, geometry=7, x_features=128, x_k=xk)
        torch.cuda.synchronize()
        return dict(g=gg, h0=h0, a1=a1, mask=mask)

    ref, got = run(0), run(x_k)
    assert not torch.equal(ref["h0"][:P], torch.full_like(ref["h0"][:P], 3.0))          # (the launch ran)
    for k in ref:
        _same_bits(ref[k], got[k], f"{k} (P = {P}, x_k = {x_k})")
    assert torch.equal(got["g"][P:], torch.full_like(got["g"][P:], 3.0)) and torch.equal(got["h0"][P:], torch.full_like(got["h0"][P:], 3.0))


def _routing(o):
    """2 segments x 2 experts, capacity 300 (no multiple of the 256-row tile): groups with 400 (full, 100 dropped), 112 (partly
    filled), 512 (full, 212 dropped) and 0 tokens."""
    seg_tokens, E, cap = 512, 2, 300
    idx = torch.zeros(2 * seg_tokens, dtype=torch.int32)
    idx[400:512] = 1
    g = torch.Generator().manual_seed(7)
    sh = torch.cat([torch.randperm(seg_tokens, generator=g), seg_tokens + torch.randperm(seg_tokens, generator=g)])
    idx = idx[sh].contiguous().to(_dev())
    P = idx.numel()
    gmax = (torch.rand(P, generator=g) * 0.8 + 0.2).to(_dev())
    gates = torch.rand(P, E, generator=g).to(_dev())
    loc, counts, perm, tok2row, _ = o.route_top1(idx, gmax, gates, seg_tokens, E, cap, True)
    drop_begin, dropped = o.route_dropped(idx, loc, counts, seg_tokens, E, cap)
    assert int(drop_begin[-1].item()) == 312
    return dict(P=P, E=E, cap=cap, ng=2 * E, gmax=gmax, counts=counts, perm=perm, tok2row=tok2row, drop_begin=drop_begin, dropped=dropped)


def test_fused_backward_same_bits(half):
    """Tag 8: the tail's two backward layers (dh2's 128 features under the K-padded backward-data copy), the combine backward, three
    expert backward layers with stored masks and a skip's y_add.  dx, dh1, dz_last, every dz, dgmax and the sigma head's weight gradient."""
    o, dt = _ops(), half
    r = _routing(o)
    P, E, cap, ng, L = r["P"], r["E"], r["cap"], r["ng"], 3
    rows = ng * cap
    g = torch.Generator().manual_seed(8)
    Wb = [o.pack_weights((torch.randn(E, M, M, generator=g) / 16).to(_dev()), dt, False) for _ in range(L)]
    w1b = o.pack_weights((torch.randn(1, M, M, generator=g) / 16).to(_dev()), dt, False)
    w2bpad = o.pack_weights_padded((torch.randn(1, M, H2, generator=g) / 16).to(_dev()), dt, False, 0, 256)
    wsig = (torch.randn(M, generator=g) * 0.1).to(_dev())
    dsig = torch.randn(P, generator=g).to(_dev())
    dh2 = torch.randn(P, H2, generator=g).to(_dev()).to(dt)
    y = torch.randn(P, M, generator=g).relu().to(_dev()).to(dt)
    y[r["tok2row"].view(-1) < 0] = 0
    masks = [torch.randint(-2 ** 31, 2 ** 31 - 1, (o.chain_mask_words(dt, ng, cap, M),), generator=g, dtype=torch.int64).int().to(_dev())
             for _ in range(L - 1)]
    kw = dict(n_groups=ng, n_wsets=E, group_stride=cap, group_rows=r["counts"].view(-1), group_rows_clamp=cap, x_gather=r["perm"].view(-1))

    def run(xk):
        dh1 = torch.full((P, M), 7.0, dtype=dt, device=_dev())
        dzl, dx = (torch.full((rows, M), 5.0, dtype=dt, device=_dev()) for _ in range(2))
        dz = [torch.full((rows, M), 5.0, dtype=dt, device=_dev()) for _ in range(L - 1)]
        dgm, dws = torch.full((P,), 7.0, device=_dev()), torch.ones(M, device=_dev())
        bl = [o.Layer(Wb[l], None, relu=2 if l > 0 else 0, mask=masks[l - 1] if l > 0 else None, save=dz[l - 1] if l > 0 else None)
              for l in range(L - 1, -1, -1)]
        o.mlp_chain(dh2, [o.Layer(w2bpad, None, save=dh1), o.Layer(w1b, None, save=dzl)] + bl, dx, y_add=dz[1], tag=8, geometry=7,
                    x_features=H2, x_k=xk, combine=(y, dsig, wsig, r["gmax"], dgm, dws), head=(2, r["drop_begin"], r["dropped"]), **kw)
        torch.cuda.synchronize()
        return dict(dx=dx, dh1=dh1, dz_last=dzl, dz0=dz[0], dz1=dz[1], dgmax=dgm, dwsig=dws)

    ref, got = run(0), run(128)
    assert not torch.equal(ref["dh1"], torch.full_like(ref["dh1"], 7.0)) and not torch.equal(ref["dwsig"], torch.ones_like(ref["dwsig"]))
    for k in ref:
        _same_bits(ref[k], got[k], k)


def test_tail_backward_chain_same_bits(half):
    """Tag 5 on geometry 7 (the separate tail backward with the combine backward in its write-out), 700 rows: two tiles and a ragged one."""
    o, dt = _ops(), half
    g = torch.Generator().manual_seed(9)
    P = 700
    dh2 = (torch.randn(P, H2, generator=g) * 0.1).to(_dev()).to(dt)
    w2p = o.pack_weights_padded((torch.randn(1, M, H2, generator=g) / 16).to(_dev()), dt, False, 0, 256)
    w1 = o.pack_weights((torch.randn(1, M, M, generator=g) / 16).to(_dev()), dt, False)
    y = torch.randn(P, M, generator=g).to(_dev()).to(dt)
    dsig, wsig = torch.randn(P, generator=g).to(_dev()), torch.randn(M, generator=g).to(_dev())
    gate = (torch.rand(P, generator=g) * 0.8 + 0.1).to(_dev())

    def run(xk):
        dh1, dout = (torch.full((P + 40, M), 3.0, dtype=dt, device=_dev()) for _ in range(2))
        dg = torch.full((P,), 7.0, device=_dev())
        o.mlp_chain(dh2, [o.Layer(w2p, None, save=dh1), o.Layer(w1, None)], dout[:P], tag=5, combine=(y, dsig, wsig, gate, dg), geometry=7,
                    x_features=H2, x_k=xk)
        torch.cuda.synchronize()
        return dict(dh1=dh1, dout=dout, dgate=dg)

    ref, got = run(0), run(128)
    assert not torch.equal(ref["dout"][:P], torch.full_like(ref["dout"][:P], 3.0))
    for k in ref:
        _same_bits(ref[k], got[k], k)


@pytest.mark.parametrize("case", ["not_a_multiple", "above_256", "geometry_below_6", "x_features_not_128", "no_kernel_of_that_length"])
def test_x_k_is_refused_where_it_means_nothing(case):
    o, dt = _ops(), torch.bfloat16
    P = 256
    pe = torch.zeros(P, 128, dtype=dt, device=_dev())
    x256 = torch.zeros(P, M, dtype=dt, device=_dev())
    W0 = torch.zeros(1, 128, M, device=_dev())
    w0p, w0 = o.pack_weights_padded(W0, dt, True, 256), o.pack_weights(W0, dt, True)
    w1 = o.pack_weights(torch.zeros(1, M, M, device=_dev()), dt, True)
    out = torch.zeros(P, M, dtype=dt, device=_dev())
    args = dict(not_a_multiple=(pe, w0p, dict(geometry=7, x_features=128, x_k=72)),
                above_256=(pe, w0p, dict(geometry=7, x_features=128, x_k=272)),
                geometry_below_6=(pe, w0, dict(geometry=0, x_features=0, x_k=128)),
                x_features_not_128=(x256, w1, dict(geometry=7, x_features=0, x_k=128)),
                no_kernel_of_that_length=(pe, w0p, dict(geometry=7, x_features=128, x_k=48)))[case]
    x, w, kw = args
    with pytest.raises(RuntimeError, match="x_k"):
        o.mlp_chain(x, [o.Layer(w, None), o.Layer(w1, None)], out, tag=3, **kw)
    torch.cuda.synchronize()
    assert out.abs().sum().item() == 0          # (nothing was launched)
