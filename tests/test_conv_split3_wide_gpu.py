"""Split3 tiles whose waves own full-width column strips (conv_dma2.hip: ids 41, 42 and 46 with one wave column) against id 43, bit
for bit, at the shapes of the stage-1 eval step's heavy layers: a dilated 3x3 256->256 conv with zero padding and with a padding
value, a 1x1 256->1024 conv with a residual, and both as grouped launches.  Every unsplit S3 id feeds each accumulator the same
MFMA sequence, so the wave layout must not change a single bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

WIDE = (41, 42, 46)
OTHERS = (44,)


def _params(ops, w, shift, pad, dil):
    packed, kpad = ops.pack_conv_weight(w)
    co, ci, kh, kw = w.shape
    packed = packed.contiguous()
    return ops.ConvParams(packed, None, shift, ci, co, kh, kw, 1, pad, dil, kpad, False, True, ops.pack_split3(packed))


def _problem(dev, seed, N, HW, cin, cout, k, dil, residual):
    g = torch.Generator().manual_seed(seed)
    M = N * HW * HW
    buf = torch.empty(M + 4, cin, device=dev)              # the padding vector sits right behind the activations
    buf[:M] = torch.randn(M, cin, generator=g).to(dev)
    buf[M:] = torch.randn(cin, generator=g).to(dev)
    w = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).to(dev)
    shift = torch.randn(cout, generator=g).to(dev)
    res = torch.randn(N, HW, HW, cout, generator=g).to(dev) if residual else None
    return buf[:M].view(N, HW, HW, cin), buf[M], w, shift, res


@pytest.mark.parametrize("N,HW,cin,cout,k,dil,residual,padv", [
    (2, 51, 256, 256, 3, 2, False, False),
    (2, 51, 256, 256, 3, 2, False, True),
    (3, 51, 256, 1024, 1, 1, True, False),
], ids=["3x3-d2-256-256", "3x3-d2-256-256-padding-value", "1x1-256-1024-residual"])
def test_full_width_wave_strips_match_id_43_bit_for_bit(hip_lib, dev, N, HW, cin, cout, k, dil, residual, padv):
    from pemp_amd import ops
    x, pv, w, shift, res = _problem(dev, 23, N, HW, cin, cout, k, dil, residual)
    p = _params(ops, w, shift, dil if k == 3 else 0, dil)
    pad_value = pv if padv else None
    want = ops.conv2d(x, p, pad_value=pad_value, residual=res, tile=43)
    assert bool(want.abs().sum() > 0)
    for tile in WIDE + OTHERS:
        got = ops.conv2d(x, p, pad_value=pad_value, residual=res, tile=tile)
        bad = got != want
        assert not bool(bad.any()), (tile, int(bad.sum()))


@pytest.mark.parametrize("padv", [False, True], ids=["zero-padding", "padding-value"])
def test_full_width_wave_strips_in_a_grouped_launch_match_id_43(hip_lib, dev, padv):
    from pemp_amd import ops
    x, pv, w, shift, _ = _problem(dev, 29, 2, 51, 256, 256, 3, 1, False)
    g = torch.Generator().manual_seed(31)
    ps = [_params(ops, w, shift, 1, 1)]
    ps += [_params(ops, (torch.randn(256, 256, 3, 3, generator=g) / 48).to(dev), shift, d, d) for d in (2, 6)]
    ps += [_params(ops, (torch.randn(256, 256, 1, 1, generator=g) / 16).to(dev), shift, 0, 1)]
    pvs = [pv if (padv and p.kh > 1) else None for p in ps]
    want = [ops.conv2d(x, p, pad_value=v, tile=43) for p, v in zip(ps, pvs)]
    for tile in WIDE + OTHERS:
        outs = [torch.empty_like(f) for f in want]
        # grouped launches take padding vectors for all members or none: the 1x1 member reads none (no tap leaves the image)
        ops.conv2d_group([x] * 4, ps, outs, pad_values=[pv] * 4 if padv else None, tile=tile)
        for i, (o, f) in enumerate(zip(outs, want)):
            assert torch.equal(o, f), (tile, i, padv)
