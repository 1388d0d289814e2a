"""RPMMs head training on the GPU: the kernels of csrc/rpmms_bwd.hip against torch float64 (autograd) on the CPU, whole training
steps against the reference-made fixtures (tests/golden/make_golden_rpmms_train.py) and against the torch restatement of the
head on the engine's own trunk features (tests/rpmms_ref.py), a five-step trajectory, the trainer's plumbing and the
``train_head`` command.  Everything at 97 x 97 (a 13 x 13 feature map) or smaller."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import rpmms_ref, util

pytestmark = pytest.mark.gpu

C = 256
GROUPS = ((0, 1), (1, 3), (4, 6))
STEP_CASES = ["rpmms_trainstep", "rpmms_trainstep_p0"]
#: (B, h, w) at dilation 2: a 97 x 97 step; non-square; every pixel lacks a vertical tap; centre tap only (twice)
SHAPES = [(2, 13, 13), (3, 9, 11), (1, 4, 5), (1, 2, 2), (1, 1, 1)]


@pytest.fixture(autouse=True)
def fixed_picks(monkeypatch):
    """One fixed kernel variant per layer from empty pick caches (as tests/test_canet_train_gpu.py): timing-based picks regroup
    float32 sums differently from box to box."""
    from pemp_amd import ops
    saved = (dict(ops._TILE_CACHE), dict(ops.WGRAD_PICKS))
    ops._TILE_CACHE.clear()
    ops.WGRAD_PICKS.clear()
    monkeypatch.setattr(ops, "AUTOTUNE", False)
    monkeypatch.setattr(ops, "PICK_HOOK", None)
    yield
    ops._TILE_CACHE.clear()
    ops.WGRAD_PICKS.clear()
    ops._TILE_CACHE.update(saved[0])
    ops.WGRAD_PICKS.update(saved[1])


def _bound(got, ref64, ref32, what):
    """|got - f64| <= 3 x |torch float32 on the CPU - f64| + 1e-6 max|f64|."""
    e_hip = float((got.double().cpu() - ref64).abs().max())
    e_ref = float((ref32.double() - ref64).abs().max())
    scale = float(ref64.abs().max())
    print(f"  {what}: |hip - f64| {e_hip:.2e}, |torch f32 - f64| {e_ref:.2e}, scale {scale:.2e}")
    assert e_hip <= 3 * e_ref + 1e-6 * scale, (what, e_hip, e_ref, scale)


# ---------------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------------
def _materialised(base, bias, wz, mu, mult, dtype, dout=None, dil=2):
    """The materialised form: per column i, cat(base, prototype i broadcast) -> 3x3 conv (dilation, zero padding; the first
    256 input channels through an identity at the centre tap, so they contribute ``base`` exactly; the last 256 through ``wz``
    [Cout,9,Cin]) + bias -> ReLU -> column i's multiplier -> sum over the mixture.  -> out [3,B,h,w,C]; with ``dout`` also
    autograd's (dbase [B,h,w,C], dWz [Cout,9,Cin], dbias [C])."""
    B, h, w, _ = base.shape
    eye = torch.zeros(C, C, 3, 3, dtype=dtype)
    eye[torch.arange(C), torch.arange(C), 1, 1] = 1.0
    x = base.to(dtype).permute(0, 3, 1, 2).clone().requires_grad_(dout is not None)
    Wz = wz.to(dtype).permute(0, 2, 1).reshape(C, C, 3, 3).clone().requires_grad_(dout is not None)
    bb = bias.to(dtype).clone().requires_grad_(dout is not None)
    W = torch.cat((eye, Wz), dim=1)
    terms = []
    for i in range(10):
        vec = mu[:, 0, i].to(dtype)[:, :, None, None].expand(B, C, h, w)
        terms.append(F.relu(F.conv2d(torch.cat((x, vec), dim=1), W, bb, 1, dil, dil)) * mult[:, i].to(dtype)[:, :, None, None])
    out = torch.stack([sum(terms[j0 + 1:j0 + k], terms[j0]) for j0, k in GROUPS]).permute(0, 1, 3, 4, 2)
    if dout is None:
        return out.detach()
    dx, dW, db = torch.autograd.grad(out, [x, Wz, bb], dout.to(dtype))
    return out.detach(), dx.permute(0, 2, 3, 1), dW.reshape(C, C, 9).permute(0, 2, 1), db


def _case(B, h, w, seed, ints):
    gen = torch.Generator().manual_seed(seed)
    if ints:
        ri = lambda shape, lo, hi: torch.randint(lo, hi + 1, shape, generator=gen).float()
        base, bias, wz, mu = ri((B, h, w, C), -8, 8), ri((C,), -4, 4), ri((C, 9, C), -2, 2), ri((B, 2, 10, C), 0, 3)
        mult, dout = ri((B, 10, C), 0, 1) * 2.0, ri((3, B, h, w, C), -4, 4)
    else:
        base, bias = torch.randn((B, h, w, C), generator=gen), torch.randn(C, generator=gen) * 0.1
        wz = torch.randn((C, 9, C), generator=gen) * (1.0 / (C * 9) ** 0.5)
        mu = torch.randn((B, 2, 10, C), generator=gen)
        mu = mu / mu.norm(dim=3, keepdim=True)
        mult, dout = (torch.rand((B, 10, C), generator=gen) < 0.5).float() * 2.0, torch.randn((3, B, h, w, C), generator=gen)
    mult[:, 2] = 0.0                                                       # whole zero columns: one for every image, one for image 0
    mult[0, 7] = 0.0
    return base, bias, wz, mu, mult, dout


def _clear_of_zero(base, bias, wz, mu, dil=2, margin=1e-3):
    """ReLU's gate is discontinuous: a pre-activation within rounding of zero is a coin flip for ANY float32 evaluation, torch's
    included.  Move ``base`` by 0.01 wherever one of the ten columns' float64 pre-activations lies within ``margin`` of zero
    (repeat until none does), so that the random-value backward compares arithmetic, not coin flips."""
    B, h, w, _ = base.shape
    Wz = wz.double().permute(0, 2, 1).reshape(C, C, 3, 3)
    R = torch.stack([F.conv2d(mu[:, 0, i].double()[:, :, None, None].expand(B, C, h, w), Wz, None, 1, dil, dil) for i in range(10)])
    for _ in range(20):
        pre = base.double().permute(0, 3, 1, 2)[None] + bias.double()[None, None, :, None, None] + R
        near = (pre.abs() < margin).any(dim=0).permute(0, 2, 3, 1).contiguous()
        if not bool(near.any()):
            return base
        base = torch.where(near, base + 0.01, base).contiguous()
    raise AssertionError("could not clear the pre-activations of zero")


def _wz_packed(wz):
    return wz.permute(1, 0, 2).contiguous()                              # [Cout,9,Cin] -> ops.pack_canet_zweights' [9,Cout,Cin]


def _forward(dev, base, bias, wz, mu, mult):
    from pemp_amd import train_ops as T
    B, h, w, _ = base.shape
    out = torch.full((3, B, h, w, 320), 7.0, device=dev)
    _, taps = T.rpmms_proto_sum_train(_wz_packed(wz).to(dev), mu.to(dev), base.to(dev), bias.to(dev), mult.to(dev), out[..., :C])
    torch.cuda.synchronize()
    assert bool((out[..., C:] == 7.0).all())                              # written into a slice of a wider buffer
    return out[..., :C], taps


def _backward(dev, base, bias, wz, mu, mult, dout):
    """-> (dbase, dWz [Cout,9,Cin], dbias, G): the weight gradient lands in the prototype half of a wider KRSC gradient."""
    from pemp_amd import train_ops as T
    B, h, w, _ = base.shape
    d_base, d_bias, d_mu, d_mult = base.to(dev), bias.to(dev), mu.to(dev), mult.to(dev)
    wide_out = torch.zeros((3, B, h, w, 320), device=dev)
    _, taps = T.rpmms_proto_sum_train(_wz_packed(wz).to(dev), d_mu, d_base, d_bias, d_mult, wide_out[..., :C])
    wide_d = torch.zeros((3, B, h, w, 288), device=dev)
    wide_d[..., :C] = dout.to(dev)
    dwide = torch.full((C, 9, 2 * C), 7.0, device=dev)
    dbias = torch.empty(C, device=dev)
    dbase, G = T.rpmms_proto_sum_bwd(wide_d[..., :C], d_base, d_bias, taps, d_mult, dil=2, mu=d_mu, dw_z=dwide[:, :, C:], dbias=dbias)
    torch.cuda.synchronize()
    assert bool((dwide[:, :, :C] == 7.0).all()), "the query half of the gradient buffer was written"
    return dbase, dwide[:, :, C:], dbias, G


@pytest.mark.parametrize("B,h,w", SHAPES)
def test_train_forward_with_unit_multipliers_is_the_eval_kernel(hip_lib, dev, B, h, w):
    from pemp_amd import ops
    base, bias, wz, mu, mult, _ = _case(B, h, w, 100 * h + w + B, ints=False)
    got, taps = _forward(dev, base, bias, wz, mu, torch.ones_like(mult))
    ref, rtaps = torch.zeros((3, B, h, w, 288), device=dev), torch.empty((B, 10, 9, C), device=dev)
    ops.rpmms_proto_sum(_wz_packed(wz).to(dev), mu.to(dev), base.to(dev), bias.to(dev), ref[..., :C], taps=rtaps)
    assert torch.equal(got, ref[..., :C]) and torch.equal(taps, rtaps)
    assert float(got.abs().max()) > 0


@pytest.mark.parametrize("B,h,w", SHAPES)
def test_train_forward_with_masks_matches_the_materialised_form(hip_lib, dev, B, h, w):
    """Masks that include whole zero columns: within 3 x the float32 torch error of the materialised form + 1e-6 of the output
    maximum (float64 is the reference)."""
    base, bias, wz, mu, mult, _ = _case(B, h, w, 200 * h + w + B, ints=False)
    got, _ = _forward(dev, base, bias, wz, mu, mult)
    r64, r32 = _materialised(base, bias, wz, mu, mult, torch.float64), _materialised(base, bias, wz, mu, mult, torch.float32)
    _bound(got, r64, r32, f"proto sum train {(B, h, w)}")
    assert bool((got[1][0] * (mult[0, 1:4].sum(0) == 0).to(dev) == 0).all())     # channels dropped in all three columns: exact zeros


@pytest.mark.parametrize("B,h,w", SHAPES)
def test_backward_is_exact_on_integer_probes(hip_lib, dev, B, h, w):
    """base in [-8,8], bias in [-4,4], Wz in [-2,2], mu in [0,3], multipliers in {0, 2}, dout in [-4,4], all integers: the tap
    products stay below 256 * 6, every pre-activation below 2^15, dbase below 10 * 8, the tap sums below 2 * 4 * 169 and dWz
    below 3 * 10 * 3 * 1352 < 2^24, so every float32 add and fma is exact in ANY order: the forward, dbase, the G-derived dWz
    and the bias gradient must EQUAL float64 autograd of the materialised form -- including the maps where only the centre
    tap is inside (exact zeros elsewhere in G)."""
    base, bias, wz, mu, mult, dout = _case(B, h, w, 300 * h + w + B, ints=True)
    out, _ = _forward(dev, base, bias, wz, mu, mult)
    dbase, dW, db, G = _backward(dev, base, bias, wz, mu, mult, dout)
    r_out, r_dx, r_dW, r_db = _materialised(base, bias, wz, mu, mult, torch.float64, dout)
    assert torch.equal(out.double().cpu(), r_out)
    assert torch.equal(dbase.double().cpu(), r_dx) and torch.equal(dW.double().cpu(), r_dW) and torch.equal(db.double().cpu(), r_db)
    assert float(r_dx.abs().max()) > 0 and float(r_dW.abs().max()) > 0
    assert bool((G[:, 2] == 0).all()) and bool((G[0, 7] == 0).all())        # dropped columns carry no gradient
    if h <= 2 and w <= 2:
        assert bool((G[:, :, [0, 1, 2, 3, 5, 6, 7, 8]] == 0).all())


@pytest.mark.parametrize("B,h,w", SHAPES)
def test_backward_on_random_values(hip_lib, dev, B, h, w):
    base, bias, wz, mu, mult, dout = _case(B, h, w, 400 * h + w + B, ints=False)
    base = _clear_of_zero(base, bias, wz, mu)
    got = _backward(dev, base, bias, wz, mu, mult, dout)[:3]
    r64 = _materialised(base, bias, wz, mu, mult, torch.float64, dout)[1:]
    r32 = _materialised(base, bias, wz, mu, mult, torch.float32, dout)[1:]
    for name, a, b, c in zip(("dbase", "dWz", "dbias"), got, r64, r32):
        _bound(a, b, c, f"proto sum adjoint {(B, h, w)} {name}")


def _history_case(B, h, w, seed):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn((B, 2, h, w), generator=gen) * 3, torch.randn((B, h, w, 2), generator=gen), torch.randn((B, 2, h, w), generator=gen))


@pytest.mark.parametrize("B,h,w", [(2, 13, 13), (1, 1, 1)])
def test_history_bwd_matches_autograd_of_softmax(hip_lib, dev, B, h, w):
    """dpred += J_softmax^T dh against float64 autograd, accumulated onto a non-zero dpred; dh is a two-channel slice of the
    64-channel buffer the padded conv writes."""
    from pemp_amd import ops, train_ops as T
    logits, dh, dpred0 = _history_case(B, h, w, 9 + h)

    def ref(dtype):
        lg = logits.to(dtype).clone().requires_grad_(True)
        g, = torch.autograd.grad(F.softmax(lg, dim=1), lg, dh.to(dtype).permute(0, 3, 1, 2))
        return dpred0.to(dtype) + g

    prob = ops.canet_history_update(logits.to(dev), out=torch.empty((B, 2, h, w), device=dev))
    wide = torch.full((B, h, w, 64), 5.0, device=dev)
    wide[..., :2] = dh.to(dev)
    dpred = dpred0.to(dev).clone()
    T.rpmms_history_bwd(wide[..., :2], prob, dpred)
    _bound(dpred, ref(torch.float64), ref(torch.float32), f"history bwd {(B, h, w)}")
    assert float((dpred.cpu() - dpred0).abs().max()) > 0


def test_new_ops_are_bit_identical_over_two_calls(hip_lib, dev):
    from pemp_amd import ops, train_ops as T
    base, bias, wz, mu, mult, dout = _case(2, 13, 13, 5, ints=False)
    a, b = _forward(dev, base, bias, wz, mu, mult), _forward(dev, base, bias, wz, mu, mult)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    a, b = _backward(dev, base, bias, wz, mu, mult, dout), _backward(dev, base, bias, wz, mu, mult, dout)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    logits, dh, dpred0 = (t.to(dev) for t in _history_case(2, 13, 13, 3))
    prob = ops.canet_history_update(logits, out=torch.empty_like(logits))
    outs = [T.rpmms_history_bwd(dh, prob, dpred0.clone()) for _ in range(2)]
    assert torch.equal(*outs)


# ---------------------------------------------------------------------------------------------------------------------------
# steps
# ---------------------------------------------------------------------------------------------------------------------------
def _trainer(dev, p=0.5, lr=1e-4, mu0=None):
    from pemp_amd.networks import rpmms
    from pemp_amd.train_rpmms import RPMMsTrainer
    net = rpmms.RPMMs(None, drop_rate=p)
    net.load_state_dict(rpmms_ref.fixture_state_dict())
    if mu0 is not None:
        net.set_pmm_init(mu0)
    return RPMMsTrainer(net.freeze_trunk(), lr=lr, device=dev), net


def _fixture_step(dev, name):
    g, sup, msk, qry, gt, mu0, draws = rpmms_ref.fixture_inputs(name)
    tr, net = _trainer(dev, float(g["p"]), mu0=mu0)
    tr.eng.draws = {k: v.to(dev) for k, v in draws.items()}
    loss, outs = tr.forward_backward(sup.to(dev), msk.to(dev), qry.to(dev), gt.to(dev))
    torch.cuda.synchronize()
    return g, tr, net, [float(loss), float(tr.last_losses[2]), float(tr.last_losses[1])], outs, (sup, msk, qry, gt, mu0, draws)


@pytest.mark.parametrize("name", STEP_CASES)
def test_train_step_gradients_match_reference(hip_lib, dev, name):
    """One forward + backward with the fixture's initial mu and Dropout2d draws against the REFERENCE's own float32 and float64
    steps: util.check_gradients (3 x the reference's float32 error + 3e-3, per tensor), the three low-resolution logits within
    util.LOGIT_TOL of float64 and the three losses within 2 x that.

    The p = 0.5 fixture's Dropout2d draws are the first that pass the generator's draw condition (make_golden_rpmms_train.py: a
    float32-sized difference of the trunk, probed on the reference alone, moves no sampled gradient by more than 1.5e-3): with
    Wgen weights one switched ReLU can carry more of the gradient than the 3e-3 this check allows for switches in all.  Measured
    on one MI355X: the worst ratio of a sampled gradient to its bound is 0.25 (p = 0.5) and 0.26 (p = 0); logits within 1.2e-4 /
    3.3e-4 / 5.7e-4 of float64 over the passes (the reference's float32: 9.6e-5 / 2.6e-4 / 4.5e-4)."""
    g, tr, net, losses, outs, _ = _fixture_step(dev, name)
    g64 = util.gold(name + "_f64")
    dl = [float((o.double().cpu() - torch.from_numpy(g64[f"low64_p{q}"])).abs().max()) for q, o in enumerate(outs)]
    dref = [float(np.abs(g[f"low32_p{q}"] - g64[f"low64_p{q}"]).max()) for q in range(3)]
    print(f"{name}: |logits - f64| {[f'{v:.2e}' for v in dl]} (reference f32: {[f'{v:.2e}' for v in dref]}); losses {losses} "
          f"(f64 {g64['loss64'].tolist()})")
    worst = util.check_gradients(g, g64, dict(net.named_parameters()), name, eps=3e-3)
    print(f"{name}: worst gradient ratio to its bound {worst:.3f}")
    assert max(dl) <= util.LOGIT_TOL
    assert np.abs(np.array(losses) - g64["loss64"]).max() <= 2 * util.LOGIT_TOL


def _head_only(dev, name):
    g, tr, net, losses, outs, (sup, msk, qry, gt, mu0, draws) = _fixture_step(dev, name)
    hip = {k: dict(net.named_parameters())[k].grad.detach().cpu().clone() for k in rpmms_ref.HEAD}
    cat_s, cat_q = (t.detach().cpu() for t in tr.eng.last_cat23)
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    run = lambda dt, cut: rpmms_ref.head_step(cat_s, cat_q, msk, gt, sd, mu0, dt, draws=draws, p=float(g["p"]), cut_history=cut)
    return hip, losses, run


@pytest.mark.parametrize("name", STEP_CASES)
def test_head_gradients_match_the_restatement_on_the_engines_own_trunk(hip_lib, dev, name):
    """The head alone: tests/rpmms_ref.py in float32 and float64 on the ENGINE's two cat((f2, f3)) groups with the same initial
    mu and draws, whole tensors (util.check_gradients_live) -- what is left when the trunk's rounding is taken out."""
    hip, losses, run = _head_only(dev, name)
    o32, o64 = run(torch.float32, False), run(torch.float64, False)
    assert abs(losses[0] - o64[0][0]) <= 3 * abs(o32[0][0] - o64[0][0]) + 1e-5
    drop = lambda d: {k: v for k, v in d.items() if k not in rpmms_ref.ZERO_GRAD}
    util.check_gradients_live(drop(hip), drop(o32[2]), drop(o64[2]), name + " head only")
    zero = rpmms_ref.ZERO_GRAD[0]                                         # a bias in front of a batch-statistics BatchNorm
    assert float(hip[zero].abs().max()) <= 1e-6 * float(hip["layer5.1.bias"].abs().max())


def test_the_head_only_comparison_sees_a_cut_history_gradient(hip_lib, dev):
    """Point 2 (the history carries a gradient) is visible to the test above: against a restatement whose history is DETACHED the
    engine's gradients of ``residule1.1.weight`` or ``layer9.weight`` miss the bound.  Nothing is cut in the engine."""
    hip, _, run = _head_only(dev, "rpmms_trainstep_p0")
    o32, o64 = run(torch.float32, True), run(torch.float64, True)
    missed = []
    for k in ("residule1.1.weight", "layer9.weight"):
        try:
            util.check_gradients_live({k: hip[k]}, {k: o32[2][k]}, {k: o64[2][k]}, "cut history")
        except AssertionError:
            missed.append(k)
    assert missed, "a restatement without the history gradient passes: the comparison cannot see point 2"


def test_trajectory(hip_lib, dev):
    """Five SGD steps (lr 1e-4, momentum 0.9, wd 5e-4, p = 0, the initial mu pinned) against the reference's trajectory: per
    step |hip - f64| <= 3 |ref32 - f64| + 2 LOGIT_TOL on the summed loss, and the last loss is below the first."""
    t = util.gold("rpmms_trajectory")
    g, sup, msk, qry, gt, mu0, _ = rpmms_ref.fixture_inputs("rpmms_trainstep_p0")
    tr, net = _trainer(dev, 0.0, lr=float(t["lr"]), mu0=mu0)
    assert tr.momentum == float(t["momentum"]) and tr.wd == float(t["weight_decay"]) and tr.max_norm == 0.0
    losses = [float(tr.train_step(sup, msk, qry, qry_msk=gt)[0]) for _ in range(5)]
    print("  trajectory: hip", [round(v, 5) for v in losses], "f64", [round(float(v), 5) for v in t["losses64"][:, 0]],
          "ref32", [round(float(v), 5) for v in t["losses32"][:, 0]])
    for k, (l, l32, l64) in enumerate(zip(losses, t["losses32"][:, 0], t["losses64"][:, 0])):
        assert abs(l - l64) <= 3 * abs(l32 - l64) + 2 * util.LOGIT_TOL, (k, l, l64)
    assert losses[4] < losses[0]


def test_trainer_plumbing(hip_lib, dev):
    """Three steps (p = 0.5, Philox masks, fresh initial mu per step): every head parameter moves, no ``model_res`` parameter
    does; the trunk's and ``layer5.1``'s running statistics move and ``num_batches_tracked`` rises by 2 per step (two batches
    per step: supports, queries); the three returned losses are (sum, CE of out2, CE of out1); ``train()``-mode ``model(...)``
    still raises.  lr 1e-3: ``layer5.0.bias`` has a zero gradient (it sits in front of a batch-statistics BatchNorm) and moves
    by weight decay alone, lr * wd = 5e-7 of its value per step -- several float32 ulps."""
    g, sup, msk, qry, gt, _, _ = rpmms_ref.fixture_inputs("rpmms_trainstep")
    tr, net = _trainer(dev, 0.5, lr=1e-3)
    before = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    outs = [tr.train_step(sup, msk, qry, qry_msk=gt) for _ in range(3)]
    for loss, p1, p2 in outs:
        assert np.isfinite(float(loss)) and float(p1) > 0 and float(p2) > 0 and float(loss) > float(p1) + float(p2)
    assert len({round(float(o[0]), 6) for o in outs}) == 3
    after = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    params = {k for k, _ in net.named_parameters()}
    for k in before:
        if k in rpmms_ref.HEAD:
            assert not torch.equal(before[k], after[k]), k
        elif k in params:
            assert k.startswith("model_res.") and torch.equal(before[k], after[k]), k
        elif k.endswith("num_batches_tracked"):
            assert int(after[k]) == int(before[k]) + 6, k
        else:
            assert k.endswith(("running_mean", "running_var")) and not torch.equal(before[k], after[k]), k
    assert "layer5.1.running_mean" in before and "layer5.1.num_batches_tracked" in before
    with pytest.raises(NotImplementedError, match="RPMMs is an inference path here"):
        net(sup.to(dev), msk.to(dev), qry.to(dev))


def test_two_trainers_from_one_seed_take_the_same_steps(hip_lib, dev):
    """Dropout2d on (p = 0.5) with no pinned draws and no pinned initial mu: the masks come from the Philox stream and the mu
    from torch's generator, both seeded by ``torch.manual_seed``; the kernel variants are fixed and no reduction is atomic.  So
    two trainers end two ``train_step``s on one batch with equal flat parameters and equal losses, bit for bit."""
    g, sup, msk, qry, gt, _, _ = rpmms_ref.fixture_inputs("rpmms_trainstep")
    runs = []
    for _ in range(2):
        torch.manual_seed(77)
        tr, _ = _trainer(dev, 0.5)
        assert tr.eng.draws is None and tr.eng.drop_rate2 == 0.5
        losses = [torch.stack(tr.train_step(sup, msk, qry, qry_msk=gt)) for _ in range(2)]
        torch.cuda.synchronize()
        runs.append((torch.stack(losses), tr.eng.flat.data.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and float(runs[0][0][0, 0]) != float(runs[0][0][1, 0]), runs
    assert torch.equal(runs[0][1], runs[1][1])


def test_train_head_command_end_to_end(hip_lib, dev, tmp_path, caplog):
    """``train_head``: one epoch of 2 steps at 97 x 97 + evaluation through the command layer logs the reference's
    ``loss / loss_p1 / loss_p2`` line for the epoch and writes ckpt.pth / bestckpt.pth (the reference's keys) that a fresh model
    loads and evaluates; the trunk's weights are the checkpoint's."""
    import logging
    from pemp_amd.entry import rpmms as e
    from pemp_amd.networks import rpmms
    common = ["split=0", f"g.model_dir={tmp_path}", "data.height=97", "data.width=97", "data.test_n=6", "te.epochs=1", "data.test_bs=2"]

    def run(*argv):
        try:
            return e.ex.run_commandline(["prog", *argv])
        finally:
            for ing in e.INGREDIENTS[1:] + [e.net_ingredient, e.ex]:
                ing._updates.clear()
                ing._cfg = None

    with caplog.at_level(logging.INFO):
        msg = run("train_head", "with", *common, "tr.total_epochs=1", "data.train_n=4", "data.bs=2", "tr.lr=0.0001", "ckpt=wgen")
    lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith("[TRAIN] loss:")]
    assert len(lines) == 1 and " - loss_p1: " in lines[0] and " - loss_p2: " in lines[0] and " - lr: " in lines[0], lines
    d = tmp_path / "rpmms" / "1"
    assert sorted(p.name for p in d.iterdir()) == ["bestckpt.pth", "ckpt.pth"] and "rpmms/1" in msg.replace("\\", "/")
    sd = torch.load(str(d / "ckpt.pth"), map_location="cpu")
    assert [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()] == util.key_spec("rpmms")
    w0 = rpmms_ref.fixture_state_dict()
    assert not torch.equal(sd["layer9.weight"], w0["layer9.weight"]) and torch.equal(sd["model_res.conv1.weight"], w0["model_res.conv1.weight"])
    assert int(sd["layer5.1.num_batches_tracked"]) == int(w0["layer5.1.num_batches_tracked"]) + 4
    fresh = rpmms.RPMMs(None)
    fresh.load_state_dict(sd)
    fresh = fresh.to(dev).eval()
    g, sup, msk, qry, gt, mu0, _ = rpmms_ref.fixture_inputs("rpmms_trainstep_p0")
    fresh.set_pmm_init(mu0)
    out = fresh.lowres(sup.to(dev), msk.to(dev), qry.to(dev))[0]
    assert tuple(out.shape) == (2, 2, 13, 13) and bool(torch.isfinite(out).all())
    assert run("test", "with", *common, "exp_id=1").startswith("Loss_p1:")
