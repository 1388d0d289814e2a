"""CANet head training on the GPU: the adjoint kernels of csrc/canet_bwd.hip against torch float64 autograd on the CPU, whole
training steps against the reference-made fixtures (tests/golden/make_golden_canet_train.py) and against the torch restatement
of the head on the engine's own trunk features (tests/canet_ref.py), a five-step trajectory, the trainer's plumbing and the
``train_head`` command.  Everything at 97 x 97 (a 13 x 13 feature map) or smaller."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import canet_ref, util

pytestmark = pytest.mark.gpu

STEP_CASES = ["canet_trainstep", "canet_trainstep5", "canet_trainstep_nh"]


@pytest.fixture(autouse=True)
def fixed_picks(monkeypatch):
    """One fixed kernel variant per layer from empty pick caches, as tests/conftest.py: pinned_picks does for the other
    whole-step parity modules: timing-based picks regroup float32 sums differently from box to box."""
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


def _ints(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def _bound(got, ref64, ref32, what):
    """|got - f64| <= 3 x |torch float32 on the CPU - f64| + 1e-6 max|f64| (the factor of util.check_gradients)."""
    e_hip = float((got.double().cpu() - ref64).abs().max())
    e_ref = float((ref32.double() - ref64).abs().max())
    scale = float(ref64.abs().max())
    print(f"  {what}: |hip - f64| {e_hip:.2e}, |torch f32 - f64| {e_ref:.2e}, scale {scale:.2e}")
    assert e_hip <= 3 * e_ref + 1e-6 * scale, (what, e_hip, e_ref, scale)


# ---------------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------------
def _zterm_reference(g, z, wz, dil, dtype, cq=4):
    """Autograd of F.conv2d(cat(q, z broadcast), W, padding=dil, dilation=dil) w.r.t. z and the z half of W, for the output
    gradient g (NHWC) -> (G [B,9,Cout] clipped tap sums of g, dz, dWz [Cout,9,Cin])."""
    B, h, w, cout = g.shape
    cin = z.shape[1]
    g, z = g.to(dtype), z.to(dtype).clone().requires_grad_(True)
    W = torch.cat((torch.zeros(cout, cq, 3, 3, dtype=dtype), wz.to(dtype).permute(0, 2, 1).reshape(cout, cin, 3, 3)), dim=1)
    W.requires_grad_(True)
    x = torch.cat((torch.ones(B, cq, h, w, dtype=dtype), z[:, :, None, None].expand(-1, -1, h, w)), dim=1)
    out = F.conv2d(x, W, None, 1, dil, dil)
    dz, dW = torch.autograd.grad(out, [z, W], g.permute(0, 3, 1, 2))
    G = torch.zeros(B, 9, cout, dtype=dtype)
    for tap in range(9):
        dy, dx = (tap // 3 - 1) * dil, (tap % 3 - 1) * dil
        y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
        if y0 < y1 and x0 < x1:
            G[:, tap] = g[:, y0:y1, x0:x1].sum(dim=(1, 2))
    return G, dz, dW[:, cq:].reshape(cout, cin, 9).permute(0, 2, 1)


def _zterm_run(dev, g, z, wz, dil, cq):
    """The kernel on g NHWC, z [B,Cin], wz [Cout,9,Cin]: the weight and its gradient are the z halves of wider KRSC buffers."""
    from pemp_amd import train_ops as T
    cout, _, cin = wz.shape
    wide = torch.full((cout, 9, cq + cin), 5.0, device=dev)
    wide[:, :, cq:] = wz.to(dev)
    dwide = torch.full((cout, 9, cq + cin), 7.0, device=dev)
    G, dz = T.canet_zterm_bwd(g.to(dev), wide[:, :, cq:], z.to(dev), dwide[:, :, cq:], dil)
    torch.cuda.synchronize()
    assert bool((dwide[:, :, :cq] == 7.0).all()), "the other half of the gradient buffer was written"
    return G, dz, dwide[:, :, cq:]


ZTERM_SHAPES = [(1, 2, 2, 256, 256), (1, 3, 3, 256, 256), (3, 3, 3, 256, 256), (2, 4, 5, 36, 260), (3, 9, 11, 256, 256),
                (2, 13, 13, 256, 256)]


@pytest.mark.parametrize("B,h,w,cin,cout", ZTERM_SHAPES)
def test_zterm_adjoint_is_exact_on_integer_probes(hip_lib, dev, B, h, w, cin, cout):
    """g in [-4,4], z in [0,8), Wz in [-3,3], all integers: every partial sum stays below 2^24 (the largest, dz, is at most
    9 * 260 rows x 3 x 4 * 169 < 4.8e6), so float32 adds and fmas are exact in ANY order and G, dz, dWz must EQUAL float64
    autograd -- including the 2 x 2 map, where all eight off-centre taps fall outside (exact zeros)."""
    gen = torch.Generator().manual_seed(1000 * h + w + B)
    g, z, wz = _ints(gen, (B, h, w, cout), -4, 4), _ints(gen, (B, cin), 0, 7), _ints(gen, (cout, 9, cin), -3, 3)
    G, dz, dW = _zterm_run(dev, g, z, wz, 2, 256)
    rG, rdz, rdW = _zterm_reference(g, z, wz, 2, torch.float64)
    assert torch.equal(G.double().cpu(), rG) and torch.equal(dz.double().cpu(), rdz) and torch.equal(dW.double().cpu(), rdW)
    if h <= 2 and w <= 2:
        assert bool((G[:, [0, 1, 2, 3, 5, 6, 7, 8]] == 0).all())


@pytest.mark.parametrize("B,h,w", [(2, 13, 13), (3, 9, 11), (2, 2, 2)])
def test_zterm_adjoint_on_random_values(hip_lib, dev, B, h, w):
    gen = torch.Generator().manual_seed(7 + h)
    g, z, wz = torch.randn((B, h, w, 256), generator=gen), torch.rand((B, 256), generator=gen), torch.randn((256, 9, 256), generator=gen) * 0.05
    got = _zterm_run(dev, g, z, wz, 2, 256)
    r64, r32 = _zterm_reference(g, z, wz, 2, torch.float64), _zterm_reference(g, z, wz, 2, torch.float32)
    for name, a, b, c in zip(("G", "dz", "dWz"), got, r64, r32):
        _bound(a, b, c, f"zterm adjoint {(B, h, w)} {name}")


@pytest.mark.parametrize("S", [1, 5])
def test_support_vector_adjoint(hip_lib, dev, S):
    """df = dz m / (S (sum m + 1e-5)) against float64 autograd of the forward's formula, written into a channel-slice view; one
    shot's mask is empty (exact zeros).  Bound 1e-6 max|ref|: the kernel rounds sum + 1e-5, S * that, the quotient and the
    product -- a few float32 roundings per element (6e-8 each), nothing accumulates."""
    from pemp_amd import train_ops as T
    B, H, h, C = 2, 97, 13, 256
    gen = torch.Generator().manual_seed(40 + S)
    mask = torch.zeros(B * S, 2, H, H)
    mask[:, 0] = (torch.rand((B * S, H, H), generator=gen) < 0.4).float()
    mask[S - 1, 0] = 0.0                                                       # an empty shot
    mask[:, 1] = 1 - mask[:, 0]
    dz = torch.randn((B, C), generator=gen)
    f = torch.zeros(B * S, C, h, h, dtype=torch.float64, requires_grad=True)
    m = F.interpolate(mask[:, :1].double(), (h, h), mode="nearest")
    zf = ((f * m).sum(dim=(2, 3)) / (m.sum(dim=(2, 3)) + 1e-5)).view(B, S, C).mean(dim=1)
    ref, = torch.autograd.grad(zf, f, dz.double())
    wide = torch.full((B * S, h, h, 320), 3.0, device=dev)
    T.canet_support_vector_bwd(dz.to(dev), mask.to(dev), S, wide[..., 32:288])
    torch.cuda.synchronize()
    got = wide[..., 32:288].permute(0, 3, 1, 2).double().cpu()
    err, scale = float((got - ref).abs().max()), float(ref.abs().max())
    print(f"  support-vector adjoint S={S}: max error {err:.2e}, scale {scale:.2e}")
    assert err <= 1e-6 * scale
    assert bool((got[S - 1] == 0).all()) and bool((wide[..., :32] == 3.0).all()) and bool((wide[..., 288:] == 3.0).all())


def _ce_case(out_hw, weighted, seed):
    gen = torch.Generator().manual_seed(seed)
    B, h = 3, 13
    pred = torch.randn((B, 2, h, h), generator=gen) * 3
    tgt = torch.randint(0, 2, (B, *out_hw), generator=gen)
    tgt[torch.rand((B, *out_hw), generator=gen) < 0.05] = 255
    tgt[1] = 255                                                               # one image of the batch is all "ignore"
    wmap = (1 + torch.rand((B, *out_hw), generator=gen)) if weighted else None
    return pred, tgt, wmap


def _dpred_reference(pred, tgt, wmap, dtype):
    p = pred.to(dtype).clone().requires_grad_(True)
    return torch.autograd.grad(canet_ref.loss_of(p, tgt, wmap), p)[0]


@pytest.mark.parametrize("out_hw", [(97, 97), (80, 120)])
@pytest.mark.parametrize("weighted", [False, True])
def test_upsample_ce_bwd_and_cls_bwd(hip_lib, dev, out_hw, weighted):
    from pemp_amd import ops, train_ops as T
    pred, tgt, wmap = _ce_case(out_hw, weighted, 11 + out_hw[1])
    r64, r32 = _dpred_reference(pred, tgt, wmap, torch.float64), _dpred_reference(pred, tgt, wmap, torch.float32)
    dp, dt = pred.to(dev), tgt.to(dev)
    dw_map = wmap.to(dev) if weighted else None
    _, stats, _ = ops.eval_tail(dp, dt, weight=dw_map)
    dpred = T.upsample_ce_bwd(dp, dt, stats, weight=dw_map)
    _bound(dpred, r64, r32, f"upsample_ce_bwd {out_hw} weighted={weighted}")
    assert bool((dpred[1] == 0).all())                                         # the all-ignore image gets no gradient
    # a given dlogits takes the same path
    lg = F.interpolate(pred.double(), out_hw, mode="bilinear", align_corners=True).requires_grad_(True)
    dl = torch.autograd.grad(canet_ref.loss_of(lg, tgt, wmap), lg)[0]
    _bound(T.upsample_ce_bwd(dlogits=dl.float().to(dev), low_hw=(13, 13)), r64, r32, f"upsample_ce_bwd(dlogits) {out_hw}")
    # the classifier behind it: x [B,13,13,256] as a channel-slice view, W [2,256]
    gen = torch.Generator().manual_seed(5)
    x, W = torch.randn((3, 13, 13, 256), generator=gen), torch.randn((2, 256), generator=gen) * 0.1
    wide = torch.zeros((3, 13, 13, 320), device=dev)
    wide[..., 64:] = x.to(dev)
    dx, dW, db = torch.full((3, 13, 13, 320), 2.0, device=dev), torch.empty((2, 256), device=dev), torch.empty(2, device=dev)
    T.canet_cls_bwd(dpred, wide[..., 64:], W.to(dev), dx[..., :256], dW, db)
    for dtype, store in ((torch.float64, {}), (torch.float32, {})):
        xx, ww, bb = x.to(dtype).requires_grad_(True), W.to(dtype).requires_grad_(True), torch.zeros(2, dtype=dtype, requires_grad=True)
        y = F.conv2d(xx.permute(0, 3, 1, 2), ww[:, :, None, None], bb)
        store.update(zip(("dx", "dW", "db"), torch.autograd.grad(y, [xx, ww, bb], dpred.cpu().to(dtype))))
        if dtype == torch.float64:
            c64 = store
        else:
            c32 = store
    for name, got in (("dx", dx[..., :256]), ("dW", dW), ("db", db)):
        _bound(got, c64[name], c32[name], f"cls_bwd {name}")
    assert bool((dx[..., 256:] == 2.0).all())


def test_new_ops_are_bit_identical_over_two_calls(hip_lib, dev):
    from pemp_amd import ops, train_ops as T
    gen = torch.Generator().manual_seed(3)
    g, z = torch.randn((2, 13, 13, 256), generator=gen).to(dev), torch.rand((2, 256), generator=gen).to(dev)
    wz, dwa, dwb = (torch.randn((256, 9, 512), generator=gen) * 0.05).to(dev), torch.zeros((256, 9, 512), device=dev), torch.zeros((256, 9, 512), device=dev)
    a = T.canet_zterm_bwd(g, wz[:, :, 256:], z, dwa[:, :, 256:], 2)
    b = T.canet_zterm_bwd(g, wz[:, :, 256:], z, dwb[:, :, 256:], 2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(dwa, dwb)
    mask = (torch.rand((2, 2, 97, 97), generator=gen) < 0.5).float().to(dev)
    fa, fb = torch.empty((2, 13, 13, 256), device=dev), torch.empty((2, 13, 13, 256), device=dev)
    T.canet_support_vector_bwd(a[1], mask, 1, fa)
    T.canet_support_vector_bwd(a[1], mask, 1, fb)
    assert torch.equal(fa, fb)
    pred, tgt, wmap = (t.to(dev) for t in _ce_case((97, 97), True, 2))
    _, stats, _ = ops.eval_tail(pred, tgt, weight=wmap)
    da, db_ = T.upsample_ce_bwd(pred, tgt, stats, weight=wmap), T.upsample_ce_bwd(pred, tgt, stats, weight=wmap)
    assert torch.equal(da, db_)
    W = (torch.randn((2, 256), generator=gen) * 0.1).to(dev)
    outs = []
    for _ in range(2):
        dx, dW, db = torch.empty_like(g), torch.empty((2, 256), device=dev), torch.empty(2, device=dev)
        T.canet_cls_bwd(da[:2], g, W, dx, dW, db)
        outs.append((dx, dW, db))
    assert all(torch.equal(p, q) for p, q in zip(*outs))


# ---------------------------------------------------------------------------------------------------------------------------
# steps
# ---------------------------------------------------------------------------------------------------------------------------
def _trainer(dev, history=True, p=0.5, lr=1e-4, sd=None):
    from pemp_amd.networks import canet
    from pemp_amd.train_canet import CANetTrainer
    net = canet.CaNet(None, init_channels=3, drop_rate=p, history=history, freeze_backbone=True)
    net.load_state_dict(canet_ref.fixture_state_dict(history) if sd is None else sd)
    return CANetTrainer(net, lr=lr, device=dev), net


def _fixture_step(dev, name):
    g, sup, msk, qry, gt, hist, draws = canet_ref.fixture_inputs(name)
    tr, net = _trainer(dev, bool(g["use_history"]), float(g["p"]))
    tr.eng.draws = {k: v.to(dev) for k, v in draws.items()}
    loss, low = tr.forward_backward(sup.to(dev), msk.to(dev), qry.to(dev), gt.to(dev), history_mask=hist[:, None].to(dev))
    torch.cuda.synchronize()
    return g, tr, net, float(loss), low, (sup, msk, qry, gt, hist, draws)


@pytest.mark.parametrize("name", STEP_CASES)
def test_train_step_gradients_match_reference(hip_lib, dev, name):
    """One forward + backward with the fixture's Dropout2d draws and history against the REFERENCE's own float32 and float64
    steps: util.check_gradients (3 x the reference's float32 error + 3e-3, per tensor, L2 / max / norm), the low-resolution
    logits within util.LOGIT_TOL of float64 and the loss within 2 x that (CE is 1-Lipschitz in the logit difference)."""
    g, tr, net, loss, low, _ = _fixture_step(dev, name)
    g64 = util.gold(name + "_f64")
    worst = util.check_gradients(g, g64, dict(net.named_parameters()), name, eps=3e-3)
    dl = float((low.double().cpu() - torch.from_numpy(g64["low64"])).abs().max())
    print(f"{name}: worst gradient ratio to its bound {worst:.3f}; |logits - f64| {dl:.2e} (reference f32: "
          f"{np.abs(g['low32'] - g64['low64']).max():.2e}); loss {loss:.6f} (f64 {float(g64['loss64']):.6f})")
    assert dl <= util.LOGIT_TOL
    assert abs(loss - float(g64["loss64"])) <= 2 * util.LOGIT_TOL


@pytest.mark.parametrize("name", ["canet_trainstep", "canet_trainstep5"])
def test_head_gradients_match_the_restatement_on_the_engines_own_trunk(hip_lib, dev, name):
    """The head alone: tests/canet_ref.py in float32 and float64 on the ENGINE's cat((f2, f3)) with the same draws, whole
    tensors (util.check_gradients_live) -- what is left when the trunk's rounding is taken out."""
    g, tr, net, loss, low, (sup, msk, qry, gt, hist, draws) = _fixture_step(dev, name)
    hip = {k: dict(net.named_parameters())[k].grad.detach().cpu().clone() for k in canet_ref.HEAD}
    cat23 = tr.eng.last_cat23.detach().cpu()
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    B, S = sup.shape[:2]
    out = {dt: canet_ref.head_step(cat23, msk, gt, sd, B, S, dt, history=hist, draws=draws, p=float(g["p"])) for dt in (torch.float32, torch.float64)}
    assert abs(loss - out[torch.float64][0]) <= 3 * abs(out[torch.float32][0] - out[torch.float64][0]) + 1e-5
    util.check_gradients_live(hip, out[torch.float32][2], out[torch.float64][2], name + " head only")


def test_trajectory(hip_lib, dev):
    """Five SGD steps (lr 1e-4, momentum 0.9, wd 5e-4, p = 0) with the history chained through the returned softmax against the
    reference's trajectory: per step |hip - f64| <= 3 |ref32 - f64| + 2 LOGIT_TOL, and the loss falls below half."""
    t = util.gold("canet_trajectory")
    g, sup, msk, qry, gt, _, _ = canet_ref.fixture_inputs("canet_trainstep")
    tr, net = _trainer(dev, True, 0.0, lr=float(t["lr"]))
    assert tr.momentum == float(t["momentum"]) and tr.wd == float(t["weight_decay"]) and tr.max_norm == 0.0
    hist, losses = None, []
    for _ in range(5):
        loss, prob = tr.train_step(sup, msk, qry, qry_msk=gt, history_mask=hist)
        losses.append(float(loss))
        hist = prob[:, None]
    print("  trajectory: hip", [round(v, 5) for v in losses], "f64", [round(float(v), 5) for v in t["losses64"]])
    for k, (l, l32, l64) in enumerate(zip(losses, t["losses32"], t["losses64"])):
        assert abs(l - l64) <= 3 * abs(l32 - l64) + 2 * util.LOGIT_TOL, (k, l, l64)
    assert losses[4] < 0.5 * losses[0]


def test_trainer_plumbing(hip_lib, dev):
    """Three steps move every head parameter and no encoder PARAMETER; the encoder's BatchNorm buffers move as the reference's
    do (train() mode: batch statistics, running statistics updated with momentum 0.1 -- freeze_bn only freezes the affine
    parameters; checked against the oracle's train-mode trunk); ``model.eval()`` then serves the updated weights (engine
    invalidation), bit for bit what a fresh model loaded from the trained state_dict gives; ``train()``-mode ``model(...)``
    still raises; with p = 0.5 and no pinned draws three steps on one batch give three different losses."""
    from oracle import ref_cpu
    from pemp_amd.networks import canet
    g, sup, msk, qry, gt, hist, _ = canet_ref.fixture_inputs("canet_trainstep")
    tr, net = _trainer(dev, True, 0.5)
    before = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    losses = [float(tr.train_step(sup, msk, qry, qry_msk=gt, history_mask=hist[:, None])[0]) for _ in range(3)]
    assert len({round(l, 6) for l in losses}) == 3 and all(np.isfinite(losses)), losses
    after = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    params = {k for k, _ in net.named_parameters()}
    for k in before:
        if k in canet_ref.HEAD:
            assert not torch.equal(before[k], after[k]), k
        elif k in params:
            assert torch.equal(before[k], after[k]), k
    # the buffers: three train-mode passes of the oracle's trunk over the same batch
    sd = {k: v.clone() for k, v in before.items() if k.startswith("encoder.")}
    x = torch.cat((sup.flatten(0, 1), qry.flatten(0, 1)))
    ref_cpu.TRAIN = True
    try:
        with torch.no_grad():
            for _ in range(3):
                f = ref_cpu.resnet_stem(x, sd, "encoder")
                for name, n in (("layer1", 3), ("layer2", 4), ("layer3", 6)):
                    f = ref_cpu._res_layer(f, sd, "encoder", name, n)
    finally:
        ref_cpu.TRAIN = False
    for k in sd:
        if k.endswith("num_batches_tracked"):
            assert int(after[k]) == int(before[k]) + 3, k
        elif k.endswith(("running_mean", "running_var")):
            assert not torch.equal(before[k], after[k]), k
            assert float((after[k] - sd[k]).abs().max()) <= 1e-4 * float(sd[k].abs().max()) + 1e-6, k
    # evaluation after training
    with pytest.raises(NotImplementedError, match="CANet is an inference path here"):
        net(sup.to(dev), msk.to(dev), qry.to(dev))
    net.eval()
    dsup, dmsk, dqry, dh = sup.to(dev), msk.to(dev), qry.to(dev), hist[:, None].to(dev)
    got = net(dsup, dmsk, dqry, False, history_mask=dh)
    fresh = canet.CaNet(None)
    fresh.load_state_dict(after)
    fresh = fresh.to(dev).eval()
    assert torch.equal(got, fresh(dsup, dmsk, dqry, False, history_mask=dh))
    stale = canet.CaNet(None)
    stale.load_state_dict(before)
    assert not torch.equal(got, stale.to(dev).eval()(dsup, dmsk, dqry, False, history_mask=dh))


def test_two_trainers_from_one_seed_take_the_same_steps(hip_lib, dev, monkeypatch):
    """Dropout2d on (p = 0.5) with no pinned draws: the masks come from the Philox stream, seeded from torch's seed at
    construction; the kernel variants are fixed (AUTOTUNE off) and no reduction is atomic.  So two trainers, each built after
    the same ``torch.manual_seed``, end two ``train_step``s on one batch with equal flat parameters and equal losses, bit for
    bit -- and the two steps of a trainer draw different masks."""
    from pemp_amd import ops
    monkeypatch.setattr(ops, "AUTOTUNE", False)
    g, sup, msk, qry, gt, hist, _ = canet_ref.fixture_inputs("canet_trainstep")
    runs = []
    for _ in range(2):
        torch.manual_seed(77)
        tr, _ = _trainer(dev, True, 0.5)
        assert tr.eng.draws is None and tr.eng.drop_rate2 == 0.5
        losses = [tr.train_step(sup, msk, qry, qry_msk=gt, history_mask=hist[:, None])[0] for _ in range(2)]
        torch.cuda.synchronize()
        runs.append((torch.stack(losses), tr.eng.flat.data.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and float(runs[0][0][0]) != float(runs[0][0][1]), runs
    assert torch.equal(runs[0][1], runs[1][1])


def test_history_drop_follows_the_reference_sampler():
    """``HistorySlots``: a key's first episode reads -1; on a second pass over the same keys the read slot is -1 exactly where a
    replayed RandomState(9876) draws <= 0.3 (one draw per episode that has a stored history, in batch order)."""
    from pemp_amd.entry.canet import HistorySlots
    hs = HistorySlots()
    keys = [(1, 0), (2, 5), (1, 3), (4, 4), (3, 1), (2, 2), (5, 0), (1, 7)]
    read, write = hs.slots(keys[:4])
    assert read == [-1] * 4 and write == [0, 1, 2, 3]
    read, write = hs.slots(keys[4:])
    assert read == [-1] * 4 and write == [4, 5, 6, 7]
    rs = np.random.RandomState(9876)
    for lo in (0, 4, 0, 4):
        read, write = hs.slots(keys[lo:lo + 4])
        want = [-1 if rs.random_sample() <= 0.3 else lo + j for j in range(4)]
        assert read == want and write == [lo + j for j in range(4)]
    r, w = hs.slots([(1, 0), (9, 9), (1, 0)])                       # a key twice in a batch: the last episode's softmax stays
    assert w == [-1, 8, 0] and r[1] == -1
    hs.clear()
    assert hs.slots(keys[:2]) == ([-1, -1], [0, 1])


def test_train_head_command_end_to_end(hip_lib, dev, tmp_path):
    """``train_head``: one epoch of 2 steps at 97 x 97 + evaluation through the command layer writes ckpt.pth / bestckpt.pth that
    ``test`` loads; ``train`` still raises."""
    from pemp_amd.entry import canet as e
    common = ["split=0", f"g.model_dir={tmp_path}", "data.height=97", "data.width=97", "data.test_n=6", "te.epochs=1", "data.test_bs=2"]

    def run(*argv):
        try:
            return e.ex.run_commandline(["prog", *argv])
        finally:
            for ing in e.INGREDIENTS[1:] + [e.net_ingredient, e.ex]:
                ing._updates.clear()
                ing._cfg = None

    msg = run("train_head", "with", *common, "tr.total_epochs=1", "data.train_n=4", "data.bs=2", "tr.lr=0.0001", "ckpt=wgen")
    d = tmp_path / "canet" / "1"
    assert sorted(p.name for p in d.iterdir()) == ["bestckpt.pth", "ckpt.pth"] and "canet/1" in msg.replace("\\", "/")
    sd = torch.load(str(d / "ckpt.pth"), map_location="cpu")
    assert [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()] == util.key_spec("canet")
    w0 = canet_ref.fixture_state_dict(True)
    assert not torch.equal(sd["layer7.weight"], w0["layer7.weight"]) and torch.equal(sd["encoder.conv1.weight"], w0["encoder.conv1.weight"])
    out = run("test", "with", *common, "exp_id=1")
    assert out.startswith("Loss:") and "mIoU" in out
    with pytest.raises(NotImplementedError, match="CANet is an inference path here"):
        run("train", "with", "split=0")
    with pytest.raises(ValueError, match="synthetic episodes only"):
        run("train_head", "with", *common, "ckpt=wgen", f"data.base_dir={tmp_path}")
