"""The fused stem (ops.stem_pool: PEMP_CONV_POOL3S2, csrc/conv_stem_pool.hip) against float64 conv2d + max_pool2d of torch on the
CPU: exact on integer data and on piece probes that reach each of the six split3 products; out-of-image conv pixels never win a
maximum; random-data error against torch's CPU fp32 path; independent of batch, of the output's channel stride and of graph
replay; and ResNetEngine.stem_forward fused against its two-launch fp32-chain form.

Shapes (N x H x W; the conv and pool sizes below come from the layers' formulas): 9 x 9 is smaller than one 8 x 8 patch of pool
outputs; 23 x 37 gives conv 12 x 19 and pool 7 x 10 (even and odd, a partial patch); 64 x 50 and 97 x 97 span several patches;
70 x 131 spans several patches in both directions with partial last ones."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import test_conv_split3_fuzz_cpu as A

pytestmark = pytest.mark.gpu

SHAPES = [(1, 9, 9), (3, 23, 37), (1, 64, 50), (3, 97, 97), (1, 70, 131)]
COUT = 64


def conv_hw(h, w):
    return (h + 2 * 3 - 7) // 2 + 1, (w + 2 * 3 - 7) // 2 + 1


def pool_hw(ho, wo):
    def one(i):                      # ATen: ceil((i + 2 p - k) / s) + 1, minus one when the last window starts in the right padding
        o = -(-(i + 2 - 3) // 2) + 1
        return o - 1 if (o - 1) * 2 >= i + 1 else o
    return one(ho), one(wo)


def reference(x, w, scale, shift, relu, dtype=torch.float64):
    """x NHWC4, w [Cout, 4, 7, 7] -> pooled NHWC in ``dtype`` on the CPU."""
    y = F.conv2d(x.to(dtype).permute(0, 3, 1, 2), w.to(dtype), None, 2, 3)
    assert tuple(y.shape[2:]) == conv_hw(x.shape[1], x.shape[2])
    if scale is not None:
        y = y * scale.to(dtype).view(1, -1, 1, 1)
    if shift is not None:
        y = y + shift.to(dtype).view(1, -1, 1, 1)
    if relu:
        y = y.clamp_min(0)
    p = F.max_pool2d(y, 3, 2, 1, ceil_mode=True)
    assert tuple(p.shape[2:]) == pool_hw(*y.shape[2:])
    return p.permute(0, 2, 3, 1).contiguous()


def params(ops, dev, w, scale=None, shift=None, relu=False):
    packed, kpad = ops.pack_conv_weight(w.to(dev), stem4=True)
    t = lambda v: None if v is None else v.float().contiguous().to(dev)
    return ops.ConvParams(packed.contiguous(), t(scale), t(shift), 4, w.shape[0], 7, 7, 2, 3, 1, kpad, True, relu,
                          w3pool=ops.pack_split3(packed.contiguous()))


def fused(ops, dev, x, prm):
    n, h, w, _ = x.shape
    hp, wp = pool_hw(*conv_hw(h, w))
    out = torch.full((n, hp, wp, prm.cout), float("nan"), device=dev)
    ops.stem_pool(x.to(dev), prm, out=out)
    return out


# ---- 1. exact probes ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def integer_problem(shape):
    """Integer operands of mixed sign: |x| <= 8, |w| <= 3, 196 terms -- every sum stays below 2^13, far under 2^24."""
    n, h, w = shape
    g = torch.Generator().manual_seed(h * 1000 + w)
    x = torch.randint(-8, 9, (n, h, w, 4), generator=g).float()
    wt = torch.randint(-3, 4, (COUT, 4, 7, 7), generator=g).float()
    return x, wt


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "no-relu"])
def test_integer_data_is_exact(hip_lib, dev, shape, relu):
    from pemp_amd import ops
    x, w = integer_problem(shape)
    scale = torch.tensor([0.5, -2.0, 1.0, 4.0] * (COUT // 4))            # powers of two: the affine stays exact
    shift = torch.tensor([4.0, -8.0, 0.0, 16.0, -1.0, 2.0, 0.5, -0.25] * (COUT // 8))
    ref = reference(x, w, scale, shift, relu)
    want = ref.float()
    assert torch.equal(want.double(), ref)
    prm = params(ops, dev, w, scale, shift, relu)
    for launch in range(2):
        y = fused(ops, dev, x, prm).cpu()
        bad = y != want
        assert not bool(bad.any()), (shape, relu, launch, int(bad.sum()), bad.nonzero()[:4].tolist(), (y - want)[bad][:4].tolist())
    if not relu:
        assert bool((want < 0).any()) and bool((want > 0).any())


def piece_problem(pq, shape):
    """Operands in the style of tests/test_conv_split3_fuzz_cpu.probe_problem: dense activations and PROBE_TERMS weights per output
    channel from the tables of the named product, so that each operand carries its pieces down to the named one and every sum of
    at most four terms per product is exact in fp32."""
    n, h, w = shape
    (xt, _, _), (wt, _, _) = A._KINDS[A.PROBE_KINDS[pq][0]], A._KINDS[A.PROBE_KINDS[pq][1]]
    xt, wt = torch.tensor(xt, dtype=torch.float64), torch.tensor(wt, dtype=torch.float64)
    m, c = torch.arange(n * h * w), torch.arange(4)
    x = xt[(m[:, None] * 7 + c[None, :] * 13 + 3) % len(xt)].view(n, h, w, 4) * A.X_SCALE
    wgt = torch.zeros(COUT, 4, 7, 7, dtype=torch.float64)
    co = torch.arange(COUT)
    for i in range(A.PROBE_TERMS):
        tap = (co * 3 + 13 * i) % 49                       # taps of every K step, 48 (the last real one) included
        wgt[co, (co + i) % 4, tap // 7, tap % 7] = wt[(co + 3 * i) % len(wt)] * A.W_SCALE
    assert int((wgt != 0).sum()) == COUT * A.PROBE_TERMS and bool((wgt[:, :, 6, 6] != 0).any())
    assert torch.equal(x.float().double(), x) and torch.equal(wgt.float().double(), wgt)
    return x.float(), wgt.float()


@pytest.mark.parametrize("pq", A.PRODUCTS)
@pytest.mark.parametrize("shape", [(3, 23, 37), (1, 70, 131)], ids=lambda s: "x".join(map(str, s)))
def test_piece_probes_are_exact_and_see_their_product(hip_lib, dev, pq, shape):
    from pemp_amd import ops
    x, w = piece_problem(pq, shape)
    ref = reference(x, w, None, None, False)
    want = ref.float()
    assert torch.equal(want.double(), ref)                               # the float64 result is an fp32 value
    # the named product matters: without it the (exactly summed) convolution changes somewhere
    full = A.split3_conv_emulated(x, w, 2, 3, 1)
    assert torch.equal(full, A.conv_f64(x, w, 2, 3, 1))
    assert not torch.equal(A.split3_conv_emulated(x, w, 2, 3, 1, drop=pq), full)
    prm = params(ops, dev, w)
    for launch in range(2):
        y = fused(ops, dev, x, prm).cpu()
        bad = y != want
        assert not bool(bad.any()), (pq, shape, launch, int(bad.sum()), bad.nonzero()[:4].tolist(), (y - want)[bad][:4].tolist())


# ---- 2. halo and padding ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_out_of_image_conv_pixels_never_win(hip_lib, dev, shape):
    """Negative data, positive weights, no ReLU: every conv output is negative, and a conv pixel outside Ho x Wo -- fewer in-image
    taps, or a zero from a halo row that was never computed -- would be LARGER than its in-image neighbours and win the window."""
    from pemp_amd import ops
    n, h, w = shape
    g = torch.Generator().manual_seed(7)
    x = -torch.randint(1, 9, (n, h, w, 4), generator=g).float()
    wt = torch.randint(1, 4, (COUT, 4, 7, 7), generator=g).float()
    ref = reference(x, wt, None, None, False)
    assert bool((ref < 0).all())
    y = fused(ops, dev, x, params(ops, dev, wt)).cpu()
    assert torch.equal(y.double(), ref), (shape, int((y.double() != ref).sum()))


# ---- 3. random data -------------------------------------------------------------------------------------------------------------
def test_random_data_error_is_within_the_split3_bound(hip_lib, dev):
    """Error against float64 relative to the magnitude |scale| conv(|x|, |w|) + |shift| taken through the same pool (the maximum
    is 1-Lipschitz: a pooled error is at most the largest error in its window, and the pooled magnitude is the largest magnitude
    there), with torch's CPU fp32 conv2d + max_pool2d as the yardstick, held to the bound the split3 family has for K <= 576
    (tests/test_conv_split3_fuzz_cpu.ratio_bound; K = 196 here)."""
    from pemp_amd import ops
    g = torch.Generator().manual_seed(31)
    x = torch.randn(3, 97, 97, 4, generator=g)
    w = torch.randn(COUT, 4, 7, 7, generator=g) / 14.0
    scale = torch.randn(COUT, generator=g)
    shift = torch.randn(COUT, generator=g)
    ref = reference(x, w, scale, shift, True)
    mag = reference(x.abs(), w.abs(), scale.abs(), shift.abs(), False)
    yard = reference(x, w, scale, shift, True, dtype=torch.float32)
    y = fused(ops, dev, x, params(ops, dev, w, scale, shift, True)).cpu()
    (m3, r3), (mc, rc) = A.errors(y, ref, mag), A.errors(yard, ref, mag)
    bound = A.ratio_bound(196)
    print(f"fused stem vs CPU fp32 | K 196 | max {m3:.2e} = x{m3 / mc:.2f} | rms {r3:.2e} = x{r3 / rc:.2f} | yardstick max {mc:.2e} "
          f"rms {rc:.2e} | bound x{bound}")
    assert bound == 4.1
    assert m3 <= bound * mc and r3 <= bound * rc, (bound, m3, mc, r3, rc)


# ---- 4. invariance --------------------------------------------------------------------------------------------------------------
def _random_problem(shape, seed=5):
    n, h, w = shape
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, h, w, 4, generator=g), torch.randn(COUT, 4, 7, 7, generator=g) / 14.0, torch.randn(COUT, generator=g),
            torch.randn(COUT, generator=g))


def test_a_batch_of_one_equals_its_slice_of_the_batch(hip_lib, dev):
    from pemp_amd import ops
    x, w, scale, shift = _random_problem((3, 70, 131))
    prm = params(ops, dev, w, scale, shift, True)
    all3 = fused(ops, dev, x, prm)
    for i in range(3):
        assert torch.equal(fused(ops, dev, x[i:i + 1].contiguous(), prm), all3[i:i + 1]), i


def test_a_channel_window_is_written_and_nothing_else(hip_lib, dev):
    from pemp_amd import ops
    x, w, scale, shift = _random_problem((3, 23, 37))
    prm = params(ops, dev, w, scale, shift, True)
    dense = fused(ops, dev, x, prm)
    wide = torch.full(tuple(dense.shape[:3]) + (96,), float("nan"), device=dev)
    ops.stem_pool(x.to(dev), prm, out=wide[..., 16:80])
    assert torch.equal(wide[..., 16:80], dense)
    assert bool(torch.isnan(wide[..., :16]).all()) and bool(torch.isnan(wide[..., 80:]).all())


def test_graph_replay_equals_eager(hip_lib, dev):
    from pemp_amd import ops
    x, w, scale, shift = _random_problem((3, 64, 50))
    prm = params(ops, dev, w, scale, shift, True)
    xd = x.to(dev)
    eager = fused(ops, dev, x, prm)
    out = torch.empty_like(eager)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        ops.stem_pool(xd, prm, out=out)                 # warm-up on the capture stream
    torch.cuda.current_stream(dev).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.stem_pool(xd, prm, out=out)
    for _ in range(2):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(out, eager)


# ---- 5. engine --------------------------------------------------------------------------------------------------------------------
def test_stem_forward_fused_agrees_with_the_fp32_chain(hip_lib, dev, monkeypatch):
    """ResNetEngine.stem_forward on the fused launch against its two-launch fp32-chain form, at the tolerance
    tests/test_conv_split3_gpu.py holds split3 to against the fp32 chain on one layer: at most 1.5 x the chain's own error
    against float64, in maximum and in rms."""
    from pemp_amd import engine, ops
    g = torch.Generator().manual_seed(3)
    conv = torch.nn.Conv2d(3, 64, 7, 2, 3, bias=False)
    bn = torch.nn.BatchNorm2d(64)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(64, 3, 7, 7, generator=g) / 12.0)
        bn.weight.copy_(torch.rand(64, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(64, generator=g) * 0.3)
        bn.running_mean.copy_(torch.randn(64, generator=g) * 0.2)
        bn.running_var.copy_(torch.rand(64, generator=g) + 0.5)
    conv, bn = conv.to(dev), bn.to(dev).eval()
    img = torch.randn(3, 3, 97, 97, generator=g)
    x4 = ops.pack_input(img.to(dev).contiguous())

    def run(split3):
        monkeypatch.setattr(engine, "SPLIT3", split3)
        eng = object.__new__(engine.ResNetEngine)
        eng.arena = engine.Arena(dev)
        eng.stem = engine.conv_params(conv, bn, relu=True, stem4=True)
        assert eng.stem.w3 is None and (eng.stem.w3pool is not None) == split3
        y = eng.stem_forward(x4).clone()
        names = {k[0] for k in eng.arena.bufs}
        return y, names

    yf, names_f = run(True)
    yc, names_c = run(False)
    assert "stem" not in names_f and "pool" in names_f and {"stem", "pool"} <= names_c
    scale, shift = engine.bn_affine(bn)
    x4c = x4.cpu()
    w4 = torch.zeros(64, 4, 7, 7)
    w4[:, :3] = conv.weight.detach().cpu()
    ref = reference(x4c, w4, scale.cpu(), shift.cpu(), True)
    ef, ec = (yf.double().cpu() - ref).abs(), (yc.double().cpu() - ref).abs()
    rms = lambda e: e.pow(2).mean().sqrt().item()
    print(f"stem_forward: fused max {ef.max().item():.2e} rms {rms(ef):.2e} | fp32 chain max {ec.max().item():.2e} rms {rms(ec):.2e}")
    assert yf.shape == yc.shape and ec.max().item() > 0
    assert ef.max().item() <= 1.5 * ec.max().item(), (ef.max().item(), ec.max().item())
    assert rms(ef) <= 1.5 * rms(ec), (rms(ef), rms(ec))
