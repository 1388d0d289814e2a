"""The adjoint kernels of csrc/pfenet_bwd.hip (PFENet head training) against torch autograd on the CPU: the float64 result is
the reference, the bound is the one tests/test_canet_train_gpu.py holds its adjoints to,
|got - f64| <= 3 x |torch float32 on the CPU - f64| + 1e-6 max|f64|.  Also the loss path of the auxiliary ``inner_cls`` heads
(60 x 60 logits against a label that is larger or smaller than the map) on the existing ``eval_tail`` + ``upsample_ce_bwd``."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BINS = (60, 30, 15, 8)


def _bound(got, ref64, ref32, what):
    e_hip = float((got.double().cpu() - ref64).abs().max())
    e_ref = float((ref32.double() - ref64).abs().max())
    scale = float(ref64.abs().max())
    print(f"  {what}: |hip - f64| {e_hip:.2e}, |torch f32 - f64| {e_ref:.2e}, scale {scale:.2e}")
    assert bool(torch.isfinite(got).all()), what
    assert e_hip <= 3 * e_ref + 1e-6 * scale, (what, e_hip, e_ref, scale)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


# ---------------------------------------------------------------------------------------------------------------------------
# adaptive average pooling
# ---------------------------------------------------------------------------------------------------------------------------
def _pool_reference(gs, hw, dtype):
    n, c = gs[0].shape[0], gs[0].shape[3]
    x = torch.zeros((n, c, hw, hw), dtype=dtype, requires_grad=True)
    ys = [F.adaptive_avg_pool2d(x, g.shape[1]) for g in gs]
    return torch.autograd.grad(ys, x, [_nchw(g).to(dtype) for g in gs])[0].permute(0, 2, 3, 1)


@pytest.mark.parametrize("hw,bins,C", [(13, BINS, 256), (51, BINS, 256), (5, (8, 3), 64), (13, (60,), 256), (13, (8,), 256),
                                       (51, (30,), 256)])
def test_adaptive_avgpool_adjoint(hip_lib, dev, hw, bins, C):
    """All bins of a call in one launch, into a channel slice of a wider buffer that starts as NaN: every element of the slice is
    written (none accumulated into), nothing outside it is touched.  The g_k are channel slices of wider buffers too."""
    from pemp_amd import train_ops as T
    B = 2
    gen = torch.Generator().manual_seed(100 * hw + len(bins) + bins[0])
    gs = [torch.randn((B, b, b, C), generator=gen) for b in bins]
    r64, r32 = _pool_reference(gs, hw, torch.float64), _pool_reference(gs, hw, torch.float32)
    wide_g = [torch.full((B, b, b, C + 32), float("nan"), device=dev) for b in bins]
    for wg, g in zip(wide_g, gs):
        wg[..., 32:] = g.to(dev)
    wide = torch.full((B, hw, hw, C + 64), float("nan"), device=dev)
    out = T.adaptive_avgpool_bwd_multi([wg[..., 32:] for wg in wide_g], wide[..., 32:32 + C])
    torch.cuda.synchronize()
    _bound(out, r64, r32, f"pool adjoint {hw} <- {bins}")
    assert bool(torch.isnan(wide[..., :32]).all()) and bool(torch.isnan(wide[..., 32 + C:]).all())


def test_adaptive_avgpool_adjoint_is_exact_on_power_of_two_windows(hip_lib, dev):
    """16 -> 8 and 16 -> 4: every window is 2 x 2 or 4 x 4, each pixel lies in one window per bin, the divisions are exact and the
    sum has two terms: the result must EQUAL float64 autograd on integer gradients."""
    from pemp_amd import train_ops as T
    gen = torch.Generator().manual_seed(9)
    gs = [torch.randint(-8, 9, (2, b, b, 64), generator=gen).float() for b in (8, 4)]
    out = T.adaptive_avgpool_bwd_multi([g.to(dev) for g in gs], torch.full((2, 16, 16, 64), float("nan"), device=dev))
    assert torch.equal(out.double().cpu(), _pool_reference(gs, 16, torch.float64))


# ---------------------------------------------------------------------------------------------------------------------------
# bilinear (align_corners) resize
# ---------------------------------------------------------------------------------------------------------------------------
def _resize_reference(dy, in_hw, add, dtype):
    n, c = dy.shape[0], dy.shape[3]
    x = torch.zeros((n, c, *in_hw), dtype=dtype, requires_grad=True)
    y = F.interpolate(x, tuple(dy.shape[1:3]), mode="bilinear", align_corners=True)
    dx = torch.autograd.grad(y, x, _nchw(dy).to(dtype))[0].permute(0, 2, 3, 1)
    return dx if add is None else dx + add.to(dtype)


RESIZES = [((60, 60), (13, 13)), ((8, 8), (13, 13)), ((13, 13), (30, 30)), ((13, 13), (8, 8)), ((13, 13), (13, 13)), ((1, 1), (5, 5)),
           ((9, 11), (7, 20))]


@pytest.mark.parametrize("in_hw,out_hw", RESIZES)
@pytest.mark.parametrize("C", [256, 2])
@pytest.mark.parametrize("add_mode", ["none", "add", "alias"])
def test_resize_adjoint(hip_lib, dev, in_hw, out_hw, C, add_mode):
    """The forward maps in_hw -> out_hw; dy has out_hw, dx in_hw.  dy and dx are channel slices of wider rows (C = 256: the float4
    path) or NCHW tensors seen as [N,H,W,C] (C = 2: channel stride H W, the scalar path); ``add`` is a third buffer or dx itself."""
    from pemp_amd import train_ops as T
    N = 2
    gen = torch.Generator().manual_seed(in_hw[0] * 1000 + out_hw[1] * 10 + C)
    dy = torch.randn((N, *out_hw, C), generator=gen)
    add = None if add_mode == "none" else torch.randn((N, *in_hw, C), generator=gen)
    r64, r32 = _resize_reference(dy, in_hw, add, torch.float64), _resize_reference(dy, in_hw, add, torch.float32)
    if C == 2:
        ddy = dy.permute(0, 3, 1, 2).contiguous().to(dev).permute(0, 2, 3, 1)
        buf = torch.full((N, C, *in_hw), float("nan"), device=dev)
        out = buf.permute(0, 2, 3, 1)
    else:
        wide_y = torch.full((N, *out_hw, C + 64), float("nan"), device=dev)
        wide_y[..., 64:] = dy.to(dev)
        ddy = wide_y[..., 64:]
        buf = torch.full((N, *in_hw, C + 32), float("nan"), device=dev)
        out = buf[..., :C]
    if add_mode == "alias":
        out.copy_(add.to(dev))
        dadd = out
    else:
        dadd = add.to(dev) if add is not None else None
    got = T.resize_bilinear_ac_bwd(ddy, add=dadd, out=out)
    torch.cuda.synchronize()
    _bound(got, r64, r32, f"resize adjoint {in_hw} -> {out_hw} C={C} {add_mode}")
    if C != 2:
        assert bool(torch.isnan(buf[..., C:]).all())


def test_resize_adjoint_identity_is_a_copy(hip_lib, dev):
    from pemp_amd import train_ops as T
    dy = torch.randn((2, 13, 13, 256), generator=torch.Generator().manual_seed(1)).to(dev)
    assert torch.equal(T.resize_bilinear_ac_bwd(dy, size=13), dy)


def test_resize_adjoint_transposes_the_forward(hip_lib, dev):
    """<A x, y> == <x, A^T y> for the project's own forward kernel, up- and down-sampling: the adjoint uses the forward's weights.
    Both sides are float32 sums of n products of O(1) terms rounded once each: |difference| <= 1e-5 sqrt(n) leaves a factor of
    about 50 over the expected rounding (6e-8 x sqrt(n) x a few roundings per term)."""
    from pemp_amd import ops, train_ops as T
    gen = torch.Generator().manual_seed(2)
    for hi, ho in ((13, 60), (60, 13), (9, 8)):
        x, y = torch.randn((2, hi, hi, 64), generator=gen).to(dev), torch.randn((2, ho, ho, 64), generator=gen).to(dev)
        lhs = float((ops.resize_bilinear_ac(x, ho).double() * y.double()).sum())
        rhs = float((x.double() * T.resize_bilinear_ac_bwd(y, size=hi).double()).sum())
        print(f"  <Ax,y> {lhs:.6f}  <x,A^T y> {rhs:.6f}")
        assert abs(lhs - rhs) <= 1e-5 * (2 * ho * ho * 64) ** 0.5


# ---------------------------------------------------------------------------------------------------------------------------
# Weighted_GAP
# ---------------------------------------------------------------------------------------------------------------------------
def _gap_reference(dvec, mask, S, C, dtype):
    n, h, w = mask.shape
    f = torch.zeros((n, C, h, w), dtype=dtype, requires_grad=True)
    m = mask.to(dtype)[:, None]
    area = F.avg_pool2d(m, (h, w)) * h * w + 0.0005                           # networks/pfenet.py:15-20
    v = F.avg_pool2d(f * m, (h, w)) * h * w / area
    vec = v.view(n // S, S, C).mean(dim=1) if S > 1 else v.view(n, C)
    return torch.autograd.grad(vec, f, dvec.to(dtype))[0].permute(0, 2, 3, 1)


@pytest.mark.parametrize("S", [1, 5])
def test_weighted_gap_adjoint(hip_lib, dev, S):
    """Fractional masks as the bilinear resize of a binary mask gives them; one image's mask is all zero: finite, exact zeros."""
    from pemp_amd import train_ops as T
    B, h, C = 2, 13, 256
    gen = torch.Generator().manual_seed(60 + S)
    big = (torch.rand((B * S, 1, 97, 97), generator=gen) < 0.4).float()
    mask = F.interpolate(big, (h, h), mode="bilinear", align_corners=True)[:, 0].contiguous()
    mask[S - 1] = 0.0
    dvec = torch.randn((B, C), generator=gen)
    r64, r32 = _gap_reference(dvec, mask, S, C, torch.float64), _gap_reference(dvec, mask, S, C, torch.float32)
    wide = torch.full((B * S, h, h, C + 64), float("nan"), device=dev)
    got = T.weighted_gap_bwd(dvec.to(dev), mask.to(dev), S, wide[..., 32:32 + C])
    torch.cuda.synchronize()
    _bound(got, r64, r32, f"weighted-GAP adjoint S={S}")
    assert bool((got[S - 1] == 0).all())
    assert bool(torch.isnan(wide[..., :32]).all()) and bool(torch.isnan(wide[..., 32 + C:]).all())


# ---------------------------------------------------------------------------------------------------------------------------
# support half of init_merge
# ---------------------------------------------------------------------------------------------------------------------------
def _merge_reference(gs, ws, svec, dtype):
    sv = svec.to(dtype).clone().requires_grad_(True)
    wl = [w.to(dtype).clone().requires_grad_(True) for w in ws]
    ys = [F.conv2d(sv[:, :, None, None].expand(-1, -1, g.shape[1], g.shape[2]), w[:, :, None, None]) for g, w in zip(gs, wl)]
    grads = torch.autograd.grad(ys, [sv] + wl, [_nchw(g).to(dtype) for g in gs])
    return grads[0], grads[1:]


def _merge_run(dev, gs, ws, svec):
    """The weights and their gradients are columns 256..511 of [256, 513] matrices, as init_merge.k.0.weight is."""
    from pemp_amd import train_ops as T
    wide_w = [torch.full((256, 513), 5.0, device=dev) for _ in ws]
    wide_d = [torch.full((256, 513), 7.0, device=dev) for _ in ws]
    for ww, w in zip(wide_w, ws):
        ww[:, 256:512] = w.to(dev)
    dsvec = T.pfenet_merge_support_bwd([g.to(dev) for g in gs], [w[:, 256:512] for w in wide_w], svec.to(dev),
                                       [d[:, 256:512] for d in wide_d])
    torch.cuda.synchronize()
    for d in wide_d:
        assert bool((d[:, :256] == 7.0).all()) and bool((d[:, 512:] == 7.0).all()), "the query / prior columns were written"
    return dsvec, [d[:, 256:512] for d in wide_d]


def test_merge_support_adjoint(hip_lib, dev):
    B = 2
    gen = torch.Generator().manual_seed(77)
    gs = [torch.randn((B, b, b, 256), generator=gen) for b in BINS]
    ws = [torch.randn((256, 256), generator=gen) * 0.05 for _ in BINS]
    svec = torch.rand((B, 256), generator=gen)
    dsvec, dws = _merge_run(dev, gs, ws, svec)
    (s64, w64), (s32, w32) = _merge_reference(gs, ws, svec, torch.float64), _merge_reference(gs, ws, svec, torch.float32)
    _bound(dsvec, s64, s32, "merge-support adjoint dsvec")
    for k, b in enumerate(BINS):
        _bound(dws[k], w64[k], w32[k], f"merge-support adjoint dW bin {b}")


def test_merge_support_adjoint_is_exact_on_integer_probes(hip_lib, dev):
    """g in [-2,2], W in [-2,2], svec in [0,4), all integers, bins (9, 4): the column sums stay below 81 x 2, dsvec below
    2 x 256 x 2 x 162 < 2^24: float32 is exact in any order and the results must EQUAL float64 autograd."""
    gen = torch.Generator().manual_seed(78)
    gs = [torch.randint(-2, 3, (3, b, b, 256), generator=gen).float() for b in (9, 4)]
    ws = [torch.randint(-2, 3, (256, 256), generator=gen).float() for _ in gs]
    svec = torch.randint(0, 4, (3, 256), generator=gen).float()
    dsvec, dws = _merge_run(dev, gs, ws, svec)
    s64, w64 = _merge_reference(gs, ws, svec, torch.float64)
    assert torch.equal(dsvec.double().cpu(), s64)
    for a, b in zip(dws, w64):
        assert torch.equal(a.double().cpu(), b)


# ---------------------------------------------------------------------------------------------------------------------------
# the loss path of the inner heads
# ---------------------------------------------------------------------------------------------------------------------------
def _ce(low, tgt):
    return F.cross_entropy(F.interpolate(low, tuple(tgt.shape[-2:]), mode="bilinear", align_corners=True), tgt, ignore_index=255)


@pytest.mark.parametrize("out_hw", [(97, 97), (33, 41)])
def test_inner_head_loss_path(hip_lib, dev, out_hw):
    """60 x 60 logits (bin 60's ``inner_cls``) against a label at 97 x 97 and at 33 x 41, where the resize is a down-sampling:
    ``eval_tail`` gives the mean CE, ``upsample_ce_bwd`` its gradient at the 60 x 60 logits."""
    from pemp_amd import ops, train_ops as T
    B = 2
    gen = torch.Generator().manual_seed(out_hw[0])
    pred = torch.randn((B, 2, 60, 60), generator=gen) * 3
    tgt = torch.randint(0, 2, (B, *out_hw), generator=gen)
    tgt[torch.rand((B, *out_hw), generator=gen) < 0.05] = 255
    res = {}
    for dtype in (torch.float64, torch.float32):
        p = pred.to(dtype).clone().requires_grad_(True)
        loss = _ce(p, tgt)
        res[dtype] = (loss.detach(), torch.autograd.grad(loss, p)[0])
    dp, dt = pred.to(dev), tgt.to(dev)
    _, stats, _ = ops.eval_tail(dp, dt)
    loss = (stats[:, 0].sum() / stats[:, 1].sum()).float()
    dpred = T.upsample_ce_bwd(dp, dt, stats)
    torch.cuda.synchronize()
    _bound(loss.reshape(1), res[torch.float64][0].reshape(1), res[torch.float32][0].reshape(1), f"inner-head loss {out_hw}")
    _bound(dpred, res[torch.float64][1], res[torch.float32][1], f"inner-head dlogits {out_hw}")


# ---------------------------------------------------------------------------------------------------------------------------
# repeatability
# ---------------------------------------------------------------------------------------------------------------------------
def test_new_ops_are_bit_identical_over_two_calls(hip_lib, dev):
    from pemp_amd import train_ops as T
    gen = torch.Generator().manual_seed(3)
    B = 2
    gs = [torch.randn((B, b, b, 256), generator=gen).to(dev) for b in BINS]
    a, b = (T.adaptive_avgpool_bwd_multi(gs, torch.empty((B, 13, 13, 256), device=dev)) for _ in range(2))
    assert torch.equal(a, b)
    add = torch.randn((B, 13, 13, 256), generator=gen).to(dev)
    for g in (gs[0], gs[3]):                                                   # 60 -> 13 and 8 -> 13 as the forward goes 13 -> bin
        a, b = (T.resize_bilinear_ac_bwd(g, size=13, add=add) for _ in range(2))
        assert torch.equal(a, b)
    mask, dvec = torch.rand((B * 5, 13, 13), generator=gen).to(dev), torch.randn((B, 256), generator=gen).to(dev)
    a, b = (T.weighted_gap_bwd(dvec, mask, 5, torch.empty((B * 5, 13, 13, 256), device=dev)) for _ in range(2))
    assert torch.equal(a, b)
    ws = [(torch.randn((256, 513), generator=gen) * 0.05).to(dev) for _ in BINS]
    svec = torch.rand((B, 256), generator=gen).to(dev)
    runs = []
    for _ in range(2):
        dws = [torch.zeros((256, 513), device=dev) for _ in BINS]
        runs.append((T.pfenet_merge_support_bwd(gs, [w[:, 256:512] for w in ws], svec, [d[:, 256:512] for d in dws]), dws))
    assert torch.equal(runs[0][0], runs[1][0]) and all(torch.equal(x, y) for x, y in zip(runs[0][1], runs[1][1]))


def test_argument_checks_raise(hip_lib, dev):
    """A bad call is an error from the library or the wrapper, never a launch."""
    from pemp_amd import _lib, train_ops as T
    g = torch.zeros((2, 8, 8, 256), device=dev)
    with pytest.raises(ValueError):
        T.adaptive_avgpool_bwd_multi([g] * 5, torch.empty((2, 13, 13, 256), device=dev))
    with pytest.raises(ValueError):
        T.adaptive_avgpool_bwd_multi([g], torch.empty((2, 13, 13, 128), device=dev))
    with pytest.raises(_lib.PempHipError):
        T.adaptive_avgpool_bwd_multi([g[..., :6]], torch.empty((2, 13, 13, 6), device=dev))      # C % 4
    with pytest.raises(ValueError):
        T.weighted_gap_bwd(torch.zeros((2, 256), device=dev), torch.zeros((2, 13, 13), device=dev), 1,
                           torch.empty((2, 8, 8, 256), device=dev))
    with pytest.raises(ValueError):
        T.resize_bilinear_ac_bwd(g, add=torch.zeros((2, 5, 5, 256), device=dev), out=torch.empty((2, 13, 13, 256), device=dev))
