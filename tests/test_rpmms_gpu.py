"""RPMMs on the HIP path: the new kernels (csrc/rpmms.hip) against torch float64 on the CPU, the model against the
reference-made fixtures (tests/golden/make_golden_rpmms.py) with the fixture's initial mu pinned, batch / graph invariance and
entry.rpmms's Evaluator.

Bounds.  The EM and the prob map are held to a float32 torch evaluation of the same formulas: |kernel - f64| <= 3 x |torch32 -
f64| + floor (factor 3: the kernel sums in another order; floor 32 eps for the components of a unit vector, 1e-6 for a
probability).  The end-to-end bounds are those of tests/test_canet_gpu.py (2e-5 relative for layer5, 1e-4 relative for what is
computed from it, util.LOGIT_TOL for the logits, 1e-4 relative for the losses): the reference's own float32 error on these
logits is 2.9e-4 (the fixtures' f64_err_p*), 14 % of util.LOGIT_TOL.

Measured on one MI355X: see DESIGN.md section 1 (RPMMs)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import util

pytestmark = pytest.mark.gpu
WGEN_SEED = 1259
C = 256
GROUPS = ((0, 1), (1, 3), (4, 6))          # (first column, K) of the mixtures K = 1 | 3 | 6
EM_SHAPES = ((2, 3, 3), (3, 9, 11), (1, 13, 13), (1, 51, 51))


# -- operands ----------------------------------------------------------------------------------------------------------------
def _mu0(gen):
    rows = []
    for _, k in GROUPS:
        mu = torch.empty(1, C, k).normal_(0, (2.0 / k) ** 0.5, generator=gen)
        rows.append((mu / (1e-6 + mu.norm(dim=1, keepdim=True)))[0].t())
    return torch.cat(rows).contiguous()


def _clusters(B, h, w, scale, gen):
    """Six uniform[0,1) centres in 256 dimensions, every pixel a random centre + 0.3 uniform noise, times ``scale``; a uniform
    mask cut to 0 below 0.4 and to 1 above 0.7."""
    centres = torch.rand(6, C, generator=gen)
    idx = torch.randint(0, 6, (B, h, w), generator=gen)
    f = ((centres[idx] + 0.3 * torch.rand(B, h, w, C, generator=gen)) * scale).contiguous()
    m = torch.rand(B, h, w, generator=gen)
    m = torch.where(m < 0.4, torch.zeros_like(m), torch.where(m > 0.7, torch.ones_like(m), m)).contiguous()
    return f, m


def _em_torch(f, m, mu0, iters=10):
    """The recurrence of include/pemp_hip.h (pemp_rpmms_em_f32) in the dtype of ``f``: -> mu [B,2,10,C]."""
    B = f.shape[0]
    out = []
    for side in (0, 1):
        wgt = (m if side == 0 else 1 - m).reshape(B, -1, 1)
        x = wgt * f.reshape(B, -1, C)
        mu = mu0.to(f.dtype)[None].repeat(B, 1, 1)
        for _ in range(iters):
            z = 20 * torch.bmm(x, mu.transpose(1, 2))
            s = torch.cat([torch.softmax(z[..., j0:j0 + k], dim=2) for j0, k in GROUPS], dim=2)
            mu = torch.bmm(s.transpose(1, 2), x) / (1e-6 + s.sum(dim=1))[..., None]
            mu = mu / (1e-6 + mu.norm(dim=2, keepdim=True))
        out.append(mu)
    return torch.stack(out, dim=1)


def _em_cases(got, f, m, mu0, what, rows):
    """One row (what, e32, err) per (image, side, K)."""
    r64 = _em_torch(f.double(), m.double(), mu0.double())
    r32 = _em_torch(f, m, mu0).double()
    assert torch.isfinite(got).all(), what
    for b in range(f.shape[0]):
        for side in (0, 1):
            for j0, k in GROUPS:
                sl = (b, side, slice(j0, j0 + k))
                rows.append((f"{what} b{b} s{side} K{k}", (r32[sl] - r64[sl]).abs().max().item(),
                             (got[sl].double() - r64[sl]).abs().max().item()))
    return r64


def _em_verdict(rows, max_left_out=0.05):
    held = [r for r in rows if r[1] <= 1e-5]                                # e32 > 1e-5: ill-conditioned, left out
    worst = max(held, key=lambda r: r[2] / (3 * r[1] + 4e-6))
    print(f"EM: {len(rows)} cases, {len(rows) - len(held)} left out, worst e32 {max(r[1] for r in held):.2e}, "
          f"worst err / bound {worst[2] / (3 * worst[1] + 4e-6):.3f} ({worst[0]}: err {worst[2]:.2e}, e32 {worst[1]:.2e})")
    assert len(rows) - len(held) <= max_left_out * len(rows), [r for r in rows if r[1] > 1e-5]
    bad = [r for r in held if r[2] > 3 * r[1] + 4e-6]
    assert not bad, bad[:10]


# -- the EM -----------------------------------------------------------------------------------------------------------------
def test_em_matches_float64_within_three_times_the_float32_torch_error(hip_lib, dev):
    from pemp_amd import ops
    rows = []
    for B, h, w in EM_SHAPES:
        for k, scale in enumerate((0.05, 1.0, 8.0)):
            gen = torch.Generator().manual_seed(1000 * h + 10 * w + k)
            f, m = _clusters(B, h, w, scale, gen)
            mu0 = _mu0(gen)
            got = ops.rpmms_em(f.to(dev), m.to(dev), mu0.to(dev)).cpu()
            _em_cases(got, f, m, mu0, f"{B}x{h}x{w} scale {scale}", rows)
    _em_verdict(rows)


def test_em_reads_a_channel_slice_and_is_bit_stable(hip_lib, dev):
    from pemp_amd import ops
    gen = torch.Generator().manual_seed(5)
    f, m = _clusters(2, 9, 11, 1.0, gen)
    mu0 = _mu0(gen)
    wide = torch.full((2, 9, 11, C + 64), 3.0)
    wide[..., 32:32 + C] = f
    a = ops.rpmms_em(f.to(dev), m.to(dev), mu0.to(dev)).cpu()
    b = ops.rpmms_em(wide.to(dev)[..., 32:32 + C], m.to(dev), mu0.to(dev)).cpu()
    assert torch.equal(a, b)
    assert torch.equal(a, ops.rpmms_em(f.to(dev), m.to(dev), mu0.to(dev)).cpu())


@pytest.mark.parametrize("fill", [0.0, 1.0])
def test_em_with_an_empty_side_gives_zero_prototypes_there(hip_lib, dev, fill):
    from pemp_amd import ops
    gen = torch.Generator().manual_seed(17)
    f, _ = _clusters(1, 9, 11, 1.0, gen)
    m = torch.full((1, 9, 11), fill)
    mu0 = _mu0(gen)
    got = ops.rpmms_em(f.to(dev), m.to(dev), mu0.to(dev)).cpu()
    assert torch.isfinite(got).all()
    empty = 0 if fill == 0.0 else 1
    assert (got[:, empty] == 0).all()                                       # every weight 0: x = 0, mu' = 0, mu = 0 / 1e-6
    rows = []
    _em_cases(got, f, m, mu0, f"mask {fill}", rows)
    _em_verdict([r for r in rows if f" s{1 - empty} " in r[0]], max_left_out=0.0)
    assert got[:, 1 - empty, 0].norm().item() > 0.99


@pytest.mark.parametrize("h,w", [(9, 11), (51, 51)])
def test_em_does_not_depend_on_the_batch(hip_lib, dev, h, w):
    from pemp_amd import ops
    gen = torch.Generator().manual_seed(h)
    f, m = _clusters(3, h, w, 1.0, gen)
    mu0 = _mu0(gen)
    all3 = ops.rpmms_em(f.to(dev), m.to(dev), mu0.to(dev)).cpu()
    alone = ops.rpmms_em(f[1:2].contiguous().to(dev), m[1:2].contiguous().to(dev), mu0.to(dev)).cpu()
    assert torch.equal(all3[1:2], alone)
    assert not torch.equal(all3[0], all3[1])


# -- the prob map -----------------------------------------------------------------------------------------------------------
def _protos(B, gen, dead=True):
    mu = torch.randn(B, 2, 10, C, generator=gen)
    mu = mu / mu.norm(dim=3, keepdim=True)
    if dead:
        mu[:, 0, 5] = 0.0                                                   # a component that attracted no pixel
    return mu.contiguous()


def _prob_torch(q, mu):
    """-> [3,B,h,w,2] (P_b, P_f) in the dtype of ``q``."""
    B, h, w, _ = q.shape
    out = []
    for j0, k in GROUPS:
        both = torch.cat((mu[:, 0, j0:j0 + k], mu[:, 1, j0:j0 + k]), dim=1)            # [B,2K,C]: foreground first
        p = torch.softmax(torch.bmm(q.reshape(B, -1, C), both.transpose(1, 2)), dim=2)
        out.append(torch.stack((p[..., k:].sum(-1), p[..., :k].sum(-1)), dim=-1).view(B, h, w, 2))
    return torch.stack(out)


@pytest.mark.parametrize("B,h,w", EM_SHAPES)
def test_prob_map_matches_float64(hip_lib, dev, B, h, w):
    from pemp_amd import ops
    gen = torch.Generator().manual_seed(7 * h + w)
    q, _ = _clusters(B, h, w, 1.0, gen)
    q = (q - 0.4) * 4                                                       # both signs: the dots spread over a few units
    mu = _protos(B, gen)
    out = torch.full((3, B, h, w, 288), 7.0, device=dev)
    ops.rpmms_prob_map(q.to(dev), mu.to(dev), out)
    got = out[..., C:C + 2].cpu().double()
    assert (out[..., :C] == 7.0).all() and (out[..., C + 2:] == 7.0).all()  # neighbouring channels untouched
    r64 = _prob_torch(q.double(), mu.double())
    e32 = (_prob_torch(q, mu).double() - r64).abs().max().item()
    err = (got - r64).abs().max().item()
    print(f"prob map {B}x{h}x{w}: err {err:.3e}, torch float32 {e32:.3e}, spread of P_f {r64[..., 1].min().item():.3f} .. {r64[..., 1].max().item():.3f}")
    assert err <= 3 * e32 + 1e-6
    assert (got.sum(-1) - 1).abs().max().item() <= 4 * 2.0 ** -23
    assert r64[..., 1].max().item() - r64[..., 1].min().item() > 0.2        # not a constant map


# -- the proto sum ----------------------------------------------------------------------------------------------------------
def _conv_params(ops, w_oihw, bias, relu, pad, dil):
    packed, kpad = ops.pack_conv_weight(w_oihw)
    co, ci, kh, kw = w_oihw.shape
    packed = packed.contiguous()
    return ops.ConvParams(packed, None, bias, ci, co, kh, kw, 1, pad, dil, kpad, False, relu, ops.pack_split3(packed))


def _proto_sum_ref(q, mu, wt, bias):
    """float64: per mixture the sum over its prototypes of relu(conv(cat(q, vec_i)) + bias), zero padding 2, dilation 2
    -> [3,B,h,w,C]."""
    B, h, w, _ = q.shape
    qc = q.permute(0, 3, 1, 2)
    terms = [F.conv2d(torch.cat((qc, mu[:, 0, i].view(B, C, 1, 1).expand(B, C, h, w)), dim=1), wt, bias, 1, 2, 2).clamp_min(0)
             for i in range(10)]
    return torch.stack([sum(terms[j0 + 1:j0 + k], terms[j0]) for j0, k in GROUPS]).permute(0, 1, 3, 4, 2)


@pytest.mark.parametrize("B,h,w", [(1, 3, 3), (3, 3, 3), (3, 9, 11), (1, 13, 13), (1, 51, 51)])
def test_proto_sum_is_exact_on_integer_probes(hip_lib, dev, B, h, w):
    """Small-integer weights, prototypes, query and bias: every fp32 sum is exact in any order, so the three sums must EQUAL
    the float64 result of the ten materialised convs -- on a 3 x 3 map every pixel is on the border ring."""
    from pemp_amd import ops
    gen = torch.Generator().manual_seed(B * 100 + h)
    q = torch.randint(0, 8, (B, h, w, C), generator=gen).double()
    mu = torch.randint(0, 4, (B, 2, 10, C), generator=gen).double()
    mu[:, 0, 2] = 0.0                                                       # a dead component still adds relu(base + bias)
    wt = torch.randint(-3, 4, (C, 2 * C, 3, 3), generator=gen).double()
    bias = torch.randint(-50, 50, (C,), generator=gen).double()
    ref = _proto_sum_ref(q, mu, wt, bias)
    assert ref.abs().max().item() < 2 ** 24
    prm = _conv_params(ops, wt[:, :C].float().contiguous().to(dev), None, False, 2, 2)
    base = ops.conv2d(q.float().to(dev), prm)
    out = torch.full((3, B, h, w, 288), 7.0, device=dev)
    ops.rpmms_proto_sum(ops.pack_canet_zweights(wt[:, C:].float().to(dev)), mu.float().to(dev), base, bias.float().to(dev),
                        out[..., :C])
    assert torch.equal(out[..., :C].cpu().double(), ref)
    assert (out[..., C:] == 7.0).all()                                      # written into a slice of a wider buffer
    assert ref[1].abs().max().item() > 0 and not torch.equal(ref[1], ref[2])


@pytest.mark.parametrize("B,h", [(2, 13), (1, 51)])
def test_proto_sum_error_is_within_the_materialised_conv_error(hip_lib, dev, B, h):
    """Random values: against float64 (one base conv + proto sum) errs at most 1.5 x what the conv engine errs on the ten
    materialised 512-channel inputs, summed in fp32 (maximum and rms; the factor of
    test_zterm_error_is_within_the_materialised_conv_error)."""
    from pemp_amd import ops
    gen = torch.Generator().manual_seed(h)
    q = (torch.rand((B, h, h, C), generator=gen) - 0.3).clamp_min(0.0)
    mu = _protos(B, gen, dead=False)
    wt = torch.randn(C, 2 * C, 3, 3, generator=gen) * (1.0 / (2 * C * 9) ** 0.5)
    bias = torch.randn(C, generator=gen) * 0.1
    ref = _proto_sum_ref(q.double(), mu.double(), wt.double(), bias.double())
    full_p = _conv_params(ops, wt.to(dev), bias.to(dev), True, 2, 2)
    terms = []
    for i in range(10):
        cat = torch.cat((q, mu[:, 0, i].view(B, 1, 1, C).expand(B, h, h, C)), dim=3).contiguous()
        terms.append(ops.conv2d(cat.to(dev), full_p).clone())
    full = torch.stack([sum(terms[j0 + 1:j0 + k], terms[j0]) for j0, k in GROUPS]).cpu().double()
    base = ops.conv2d(q.to(dev), _conv_params(ops, wt[:, :C].contiguous().to(dev), None, False, 2, 2))
    out = torch.zeros((3, B, h, h, 288), device=dev)
    ops.rpmms_proto_sum(ops.pack_canet_zweights(wt[:, C:].to(dev)), mu.to(dev), base, bias.to(dev), out[..., :C])
    split = out[..., :C].cpu().double()
    rms = lambda e: e.pow(2).mean().sqrt().item()
    for g in range(3):
        e_full, e_split = (full[g] - ref[g]).abs(), (split[g] - ref[g]).abs()
        print(f"proto sum {h}x{h} K={GROUPS[g][1]}: max {e_split.max().item():.3e} vs {e_full.max().item():.3e}, "
              f"rms {rms(e_split):.3e} vs {rms(e_full):.3e}")
        assert e_split.max().item() <= 1.5 * e_full.max().item()
        assert rms(e_split) <= 1.5 * rms(e_full)


# -- model against the reference's fixtures -----------------------------------------------------------------------------------
def _net(dev, g=None):
    from pemp_amd import synth
    from pemp_amd.networks import rpmms as m
    net = m.RPMMs(None)
    net.load_state_dict(synth.wgen_state_dict_for(net, WGEN_SEED))
    net = net.to(dev).eval()
    if g is not None:
        net.set_pmm_init({k: torch.from_numpy(g[f"mu0_k{k}"]) for k in (1, 3, 6)})
    return net


def _batch(seeds, H, dev):
    from pemp_amd import synth
    b = synth.make_batch([int(s) for s in seeds], shot=1, height=H, width=H, out_hw=(H, H))
    return [torch.from_numpy(b[k]).to(dev) for k in ("sup_img", "sup_mask", "qry_img")]


def _labels(seeds, H, hw):
    from pemp_amd import synth
    return torch.from_numpy(np.concatenate([synth.make_episode(int(s), shot=1, height=H, width=H, out_hw=hw)["qry_mask"]
                                            for s in seeds]))


def _close(got, ref, rel, what):
    ref = np.asarray(ref, np.float64)
    err = np.abs(np.asarray(got, np.float64) - ref).max()
    bound = rel * max(1.0, np.abs(ref).max())
    print(f"{what}: max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"
    return err


def _sample(t, H):
    t = t.permute(0, 3, 1, 2).cpu().numpy()
    return t[:, ::16] if H <= 97 else t[:, ::32, ::5, ::5]


def _sample_pm(t, H):
    t = t.permute(0, 3, 1, 2).cpu().numpy()
    return t if H <= 97 else t[:, :, ::5, ::5]


@pytest.mark.parametrize("name", ["rpmms_small", "rpmms_full"])
def test_rpmms_matches_reference_golden(hip_lib, dev, name):
    from pemp_amd import ops
    g = util.gold(name)
    seeds, H = g["seeds"], int(g["H"])
    B = len(seeds)
    net = _net(dev, g)
    sup, msk, qry = _batch(seeds, H, dev)
    with torch.no_grad():
        ret = net(sup, msk, qry)
    assert isinstance(ret, tuple) and len(ret) == 4
    feat, outs = ret[0], ret[1:]
    h, w = net.feature_hw(H, H)
    assert tuple(feat.shape) == (B, 256, h, w) and all(tuple(o.shape) == (B, 2, h, w) for o in outs)
    eng = net._engine_for(dev)["rpmms"]
    # the stages in pipeline order, so that a failure names the first one that is off
    _close(_sample(eng.last_layer5, H), g["layer5_s"], 2e-5, f"{name} layer5")
    assert torch.equal(feat, eng.last_layer5[:B].permute(0, 3, 1, 2))
    for j0, k in GROUPS:
        _close(eng.last_mu[:, 0, j0:j0 + k].cpu().numpy(), g[f"mu_f_k{k}"], 1e-4, f"{name} mu_f K={k}")
        _close(eng.last_mu[:, 1, j0:j0 + k].cpu().numpy(), g[f"mu_b_k{k}"], 1e-4, f"{name} mu_b K={k}")
    for p in range(3):
        _close(_sample_pm(eng.last_layer56_in[p][..., 256:258], H), g[f"p{p}_prob_s"], 1e-4, f"{name} prob map {p}")
    assert (eng.last_layer56_in[..., 258:] == 0).all()
    _close(_sample(eng.last_aspp_in, H), g["aspp_in_s"], 1e-4, f"{name} ASPP input (last pass)")
    losses = {}
    for p, low in enumerate(outs):
        err = float(np.abs(low.cpu().numpy().astype(np.float64) - g[f"p{p}_logits"]).max())
        print(f"{name} pass {p}: max |d logit| {err:.3e} (the reference's own float32 error: {float(g[f'f64_err_p{p}']):.3e})")
        assert err <= util.LOGIT_TOL, f"{name} pass {p} logits: {err:.3e}"
        n = 0
        while f"o{n}_out_hw" in g:
            hw = tuple(int(v) for v in g[f"o{n}_out_hw"])
            lg = ops.upsample_bilinear_ac(low, hw).cpu()
            ref_am = np.unpackbits(g[f"p{p}_o{n}_argmax_bits"])[:B * hw[0] * hw[1]].reshape(B, *hw)
            util.assert_argmax_exact(lg, ref_am, what=f"{name} pass {p} out {hw}")
            loss = F.cross_entropy(lg, _labels(seeds, H, hw)).item()
            want = float(g[f"p{p}_o{n}_loss"])
            assert abs(loss - want) <= 1e-4 * max(1.0, abs(want)), (name, p, hw, loss, want)
            losses[(p, n)] = want
            n += 1
    # the reference's loss / prediction contracts on the first output size
    hw = tuple(int(v) for v in g["o0_out_hw"])
    label = _labels(seeds, H, hw).to(dev)
    total, l_p1, l_p2 = net.get_loss(ret, label[:, None])
    want = [losses[(p, 0)] for p in range(3)]
    assert abs(total.item() - sum(want)) <= 1e-4 * max(1.0, sum(want))
    assert abs(l_p1.item() - want[2]) <= 1e-4 * max(1.0, want[2]) and abs(l_p2.item() - want[1]) <= 1e-4 * max(1.0, want[1])
    soft, pred = net.get_pred(ret, torch.empty((B, 1) + hw))
    assert tuple(soft.shape) == (B, 2) + hw and tuple(pred.shape) == (B,) + hw
    ref_am = np.unpackbits(g["p2_o0_argmax_bits"])[:B * hw[0] * hw[1]].reshape(B, *hw)
    assert torch.equal(pred.cpu(), ops.upsample_bilinear_ac(outs[2], hw).argmax(1).cpu())
    assert (pred.cpu().numpy() != ref_am).mean() <= 0.03
    # lowres: the final output first
    with torch.no_grad():
        low = net.lowres(sup, msk, qry)
    assert torch.equal(low[0], outs[2]) and torch.equal(low[1], outs[0]) and torch.equal(low[2], outs[1])


def test_batch_1_equals_batch_2_and_graph_equals_eager(hip_lib, dev, exact_eval_variants):
    g = util.gold("rpmms_small")
    seeds, H = g["seeds"], int(g["H"])
    net = _net(dev, g)
    sup, msk, qry = _batch(seeds, H, dev)
    with torch.no_grad():
        both = [o.clone() for o in net.lowres(sup, msk, qry)]
        for b in range(len(seeds)):
            alone = net.lowres(sup[b:b + 1], msk[b:b + 1], qry[b:b + 1])
            for o2, o1 in zip(both, alone):
                assert torch.equal(o2[b:b + 1], o1)
        graphed = [o.clone() for o in net.lowres_graphed(sup, msk, qry)]
        for a, b_ in zip(both, graphed):
            assert torch.equal(a, b_)
        # a replay reads the buffer's current contents: another init, another result, and again the eager one
        net.resample_pmm_init(torch.Generator().manual_seed(3))
        eager = [o.clone() for o in net.lowres(sup, msk, qry)]
        replay = [o.clone() for o in net.lowres_graphed(sup, msk, qry)]
    for a, b_ in zip(eager, replay):
        assert torch.equal(a, b_)
    assert not torch.equal(eager[0], both[0])
    assert not torch.equal(both[0], both[1]) and not torch.equal(both[1], both[2])


# -- evaluator ----------------------------------------------------------------------------------------------------------------
def test_test_step_keeps_the_reference_contract(hip_lib, dev):
    from pemp_amd.entry import rpmms as entry
    g = util.gold("rpmms_small")
    seeds, H = g["seeds"], int(g["H"])
    net = _net(dev, g)
    hw = tuple(int(v) for v in g["o0_out_hw"])
    inputs = [t.cpu() for t in _batch(seeds, H, dev)]
    label = _labels(seeds, H, hw)
    for use_graph in (True, False):
        ev = entry.Evaluator(net, device=dev, use_graph=use_graph)
        pred, loss, loss_p1, loss_p2 = ev.test_step(inputs, label[:, None])
        want = [float(g[f"p{p}_o0_loss"]) for p in range(3)]
        assert pred.shape == (len(seeds),) + hw
        assert abs(loss_p1 - want[2]) <= 1e-4 * max(1.0, want[2])            # the final output's CE
        assert abs(loss_p2 - want[1]) <= 1e-4 * max(1.0, want[1])
        assert abs(loss - sum(want)) <= 1e-4 * max(1.0, sum(want))
        ref_am = np.unpackbits(g["p2_o0_argmax_bits"])[:len(seeds) * hw[0] * hw[1]].reshape(len(seeds), *hw)
        assert (pred != ref_am).mean() <= 0.03
        assert net.pmm_init_pinned                                          # a pinned init survives the steps


def test_a_short_round_is_the_same_at_batch_1_and_3(hip_lib, dev, exact_eval_variants):
    from pemp_amd.entry import rpmms as entry
    net = _net(dev, util.gold("rpmms_small"))                               # pinned: the steps share one init
    rows = []
    for batch in (1, 3):
        data = entry.SyntheticEpisodes(6, 5678, 1, split=0, height=97, width=97)
        data.sample_tasks()
        ev = entry.Evaluator(net, device=dev)
        eps = [data.task(i)[:2] for i in range(len(data))]
        if batch == 1:
            rows.append(torch.cat([ev.test_step_device(*ep)[1] for ep in eps]).cpu())
        else:
            rows.append(torch.cat([ev.test_step_batch(eps[i:i + batch]) for i in range(0, len(eps), batch)]).cpu())
    assert torch.equal(rows[0], rows[1])
    assert rows[0][:, 5].sum().item() > 0                                   # some foreground is found
    data = entry.SyntheticEpisodes(6, 5678, 1, split=0, height=97, width=97)
    loss, miou, biou = entry.Evaluator(net, device=dev).start_eval_loop(data, 20, 0, te_epochs=1, batch=3)
    st = rows[0].numpy()
    assert abs(loss - float(np.mean(st[:, 0] / st[:, 1]))) <= 1e-9 * max(1.0, abs(loss))


def test_an_unpinned_init_is_drawn_again_for_every_step(hip_lib, dev):
    from pemp_amd.entry import rpmms as entry
    net = _net(dev)
    assert not net.pmm_init_pinned
    ev = entry.Evaluator(net, device=dev)
    data = entry.SyntheticEpisodes(2, 5678, 1, split=0, height=97, width=97)
    data.sample_tasks()
    inputs, qry_msk, _ = data.task(0)
    seen, protos = [], []
    for _ in range(2):
        ev.test_step_device(inputs, qry_msk)
        seen.append(net.pmm_mu0.clone())
        protos.append(net._engine_for(dev)["rpmms"].last_mu.clone())
    assert not torch.equal(seen[0], seen[1])
    assert (seen[1].norm(dim=1) - 1).abs().max().item() <= 1e-5
    assert not torch.equal(protos[0], protos[1])                            # the replayed graph read the new init
