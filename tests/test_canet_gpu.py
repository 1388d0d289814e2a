"""CANet on the HIP path: the new kernels (csrc/canet.hip) against torch float64 on the CPU, the model against the
reference-made fixtures (tests/golden/make_golden_canet.py) over three passes of the refinement loop, and the evaluation
protocol (batching with the group-closing rule, graph replay with changing slots, entry.canet's Evaluator).

Measured on one MI355X (max |d logit| against the reference over the three passes; bound util.LOGIT_TOL = 2e-3): see the
table in DESIGN.md section 1 (CANet)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import util

pytestmark = pytest.mark.gpu
WGEN_SEED = 1259


# -- kernels --------------------------------------------------------------------------------------------------------------------
def _feats(shape, gen):
    return (torch.rand(shape, generator=gen) - 0.3).clamp_min(0.0)          # post-ReLU-like


@pytest.mark.parametrize("S,h,H", [(1, 13, 97), (5, 13, 97), (1, 51, 401), (5, 51, 401)])
def test_support_vector_matches_float64(hip_lib, dev, S, h, H):
    from pemp_amd import ops
    gen = torch.Generator().manual_seed(10 * S + h)
    B, C = 2, 256
    f = _feats((B * S, h, h, C + 32), gen)
    m = (torch.rand((B * S, 2, H, H), generator=gen) > 0.5).float()
    m[0, 0] = 0.0                                                           # an empty mask: episode 0's shot 0
    got = ops.canet_support_vector(f.to(dev)[..., 16:16 + C], m.to(dev), S).cpu()        # a channel-slice input view
    ms = F.interpolate(m[:, :1], (h, h), mode="nearest")[:, 0]              # the nearest indices are ATen's own
    fd, md = f[..., 16:16 + C].double(), ms.double()
    z = (fd * md[..., None]).sum((1, 2)) / (md.sum((1, 2))[:, None] + 1e-5)
    ref = z.view(B, S, C).mean(1)
    err = (got.double() - ref).abs().max().item()
    print(f"support vector S={S} {h}x{h} from {H}: max err {err:.3e}")
    assert err <= 1e-5 * max(1.0, ref.abs().max().item())
    assert ref.abs().max().item() > 0.1
    alone = ops.canet_support_vector(f[:1].to(dev)[..., 16:16 + C], m[:1].to(dev), 1).cpu()
    assert (alone == 0).all()                                               # all-zero mask -> exactly 0
    assert torch.equal(got, ops.canet_support_vector(f.to(dev)[..., 16:16 + C], m.to(dev), S).cpu())     # bit-stable


def _conv_params(ops, w_oihw, bias, relu, pad, dil):
    packed, kpad = ops.pack_conv_weight(w_oihw)
    co, ci, kh, kw = w_oihw.shape
    packed = packed.contiguous()
    return ops.ConvParams(packed, None, bias, ci, co, kh, kw, 1, pad, dil, kpad, False, relu, ops.pack_split3(packed))


@pytest.mark.parametrize("B,h,w", [(1, 13, 13), (3, 13, 13), (1, 51, 51), (3, 9, 11), (1, 3, 3), (3, 3, 3)])
def test_zterm_is_exact_on_integer_probes(hip_lib, dev, B, h, w):
    """Small-integer q, z, weights and bias: every fp32 sum is exact in any order, so relu(conv(q) + bias + R) must EQUAL the
    float64 conv over cat(q, z broadcast) with zero padding 2, dilation 2 -- on a 3 x 3 map every pixel is a border pixel."""
    from pemp_amd import ops
    gen = torch.Generator().manual_seed(B * 100 + h)
    C = 256
    q = torch.randint(0, 8, (B, h, w, C), generator=gen).double()
    z = torch.randint(0, 8, (B, C), generator=gen).double()
    wt = torch.randint(-3, 4, (C, 2 * C, 3, 3), generator=gen).double()
    bias = torch.randint(-50, 50, (C,), generator=gen).double()
    cat = torch.cat((q.permute(0, 3, 1, 2), z.view(B, C, 1, 1).expand(B, C, h, w)), dim=1)
    ref = F.conv2d(cat, wt, bias, 1, 2, 2)
    assert ref.abs().max().item() < 2 ** 24
    ref_r = F.conv2d(cat[:, C:], wt[:, C:], None, 1, 2, 2).permute(0, 2, 3, 1)
    wide = torch.full((B, h, w, C + 32), 7.0, device=dev)
    R = ops.canet_zterm(ops.pack_canet_zweights(wt[:, C:].float().to(dev)), z.float().to(dev), h, w, 2, out=wide[..., :C])
    assert torch.equal(R.cpu().double(), ref_r)                             # R alone, written into a slice of a wider buffer
    assert (wide[..., C:] == 7.0).all()
    prm = _conv_params(ops, wt[:, :C].float().to(dev), bias.float().to(dev), True, 2, 2)
    y = ops.conv2d(q.float().to(dev), prm, residual=R)
    assert torch.equal(y.cpu().double(), ref.clamp_min(0).permute(0, 2, 3, 1))


@pytest.mark.parametrize("B,h", [(2, 13), (1, 51)])
def test_zterm_error_is_within_the_materialised_conv_error(hip_lib, dev, B, h):
    """Random values: against float64 the z-term path errs at most 1.5 x what the conv engine errs on the materialised
    512-channel input (maximum and rms): splitting the sum costs no accuracy against the path it replaces."""
    from pemp_amd import ops
    gen = torch.Generator().manual_seed(h)
    C = 256
    q, z = _feats((B, h, h, C), gen), _feats((B, C), gen)
    wt = torch.randn(C, 2 * C, 3, 3, generator=gen) * (1.0 / (2 * C * 9) ** 0.5)
    bias = torch.randn(C, generator=gen) * 0.1
    cat = torch.cat((q, z.view(B, 1, 1, C).expand(B, h, h, C)), dim=3).contiguous()
    ref = F.conv2d(cat.double().permute(0, 3, 1, 2), wt.double(), bias.double(), 1, 2, 2).clamp_min(0).permute(0, 2, 3, 1)
    full = ops.conv2d(cat.to(dev), _conv_params(ops, wt.to(dev), bias.to(dev), True, 2, 2)).cpu().double()
    R = ops.canet_zterm(ops.pack_canet_zweights(wt[:, C:].to(dev)), z.to(dev), h, h, 2)
    split = ops.conv2d(q.to(dev), _conv_params(ops, wt[:, :C].contiguous().to(dev), bias.to(dev), True, 2, 2), residual=R).cpu().double()
    e_full, e_split = (full - ref).abs(), (split - ref).abs()
    rms = lambda e: e.pow(2).mean().sqrt().item()
    print(f"z-term {h}x{h}: max {e_split.max().item():.3e} vs {e_full.max().item():.3e}, rms {rms(e_split):.3e} vs {rms(e_full):.3e}")
    assert e_split.max().item() <= 1.5 * e_full.max().item()
    assert rms(e_split) <= 1.5 * rms(e_full)


def test_block_input_copies_rectifies_and_reads_both_history_sources(hip_lib, dev):
    from pemp_amd import ops
    gen = torch.Generator().manual_seed(3)
    B, h, w, C = 3, 9, 11, 256
    x = torch.randn((B, h, w, C + 64), generator=gen).to(dev)
    hist = torch.randn((B, 2, h, w), generator=gen).to(dev)                 # negative values too: they are rectified
    xs = x[..., 32:32 + C]
    out = torch.full((B, h, w, 288), 5.0, device=dev)
    ops.canet_block_input(xs, out, history=hist)
    assert torch.equal(out[..., :C], torch.relu(xs))
    assert torch.equal(out[..., C:C + 2], torch.relu(hist).permute(0, 2, 3, 1))
    assert (out[..., C + 2:] == 5.0).all()                                  # neighbouring channels untouched
    table = torch.randn((6, 2, h, w), generator=gen).to(dev)
    table[4], table[1], table[0] = hist[0], hist[1], hist[2]
    slot = torch.tensor([4, 1, 0], dtype=torch.int32, device=dev)
    out2 = torch.full((B, h, w, 288), 5.0, device=dev)
    ops.canet_block_input(xs, out2, history=table, slot=slot)
    assert torch.equal(out2, out)                                           # tensor source and table source agree
    slot = torch.tensor([4, -1, 0], dtype=torch.int32, device=dev)
    ops.canet_block_input(xs, out2, history=table, slot=slot)
    assert (out2[1, ..., C:C + 2] == 0).all() and torch.equal(out2[0], out[0]) and torch.equal(out2[2], out[2])
    ops.canet_block_input(xs, out2, with_history=True)                      # no source: zeros
    assert (out2[..., C:C + 2] == 0).all() and torch.equal(out2[..., :C], torch.relu(xs))
    plain = torch.full((B, h, w, C + 32), 5.0, device=dev)
    ops.canet_block_input(xs, plain[..., :C])                               # residual_2 / 3 and history=False: the copy only
    assert torch.equal(plain[..., :C], torch.relu(xs)) and (plain[..., C:] == 5.0).all()
    with pytest.raises(ValueError):
        ops.canet_block_input(xs, out, history=table)                       # a table needs slots


def test_history_update_matches_float64_softmax(hip_lib, dev):
    from pemp_amd import ops
    gen = torch.Generator().manual_seed(4)
    B, h, w = 4, 13, 13
    lg = torch.randn((B, 2, h, w), generator=gen) * 10
    lg[0, 0, 0, 0], lg[0, 1, 0, 0] = 35.0, -35.0                            # 70 apart: no overflow
    lg[0, 0, 0, 1], lg[0, 1, 0, 1] = -60.0, 10.0
    ref = torch.softmax(lg.double(), dim=1)
    table = torch.full((7, 2, h, w), -3.0, device=dev)
    slot = torch.tensor([5, -1, 0, 2], dtype=torch.int32, device=dev)
    out = torch.empty((B, 2, h, w), device=dev)
    ops.canet_history_update(lg.to(dev), table=table, slot=slot, out=out)
    assert (out.cpu().double() - ref).abs().max().item() <= 1e-6
    assert torch.isfinite(out).all()
    for b, s in enumerate([5, -1, 0, 2]):
        if s >= 0:
            assert torch.equal(table[s], out[b])
    for s in (1, 3, 4, 6):
        assert (table[s] == -3.0).all()                                     # other rows (and the row of slot -1) unchanged
    only = ops.canet_history_update(lg.to(dev), out=torch.empty((B, 2, h, w), device=dev))
    assert torch.equal(only, out)


# -- model against the reference's fixtures --------------------------------------------------------------------------------------
def _net(dev, history=True):
    from pemp_amd.networks import canet as m
    net = m.CaNet(None, init_channels=3, drop_rate=0.5, history=history, freeze_backbone=True)
    from pemp_amd import synth
    net.load_state_dict(synth.wgen_state_dict_for(net, WGEN_SEED))
    return net.to(dev).eval()


def _batch(seeds, shot, H, dev):
    from pemp_amd import synth
    b = synth.make_batch([int(s) for s in seeds], shot=shot, height=H, width=H, out_hw=(H, H))
    return [torch.from_numpy(b[k]).to(dev) for k in ("sup_img", "sup_mask", "qry_img")]


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


def _check_outputs(g, pre, low, seeds, shot, H, name):
    """Logits at util.LOGIT_TOL, and per output size arg-max (exact outside util.MARGIN) and CE loss at 1e-4 relative."""
    from pemp_amd import ops, synth
    B = len(seeds)
    err = float(np.abs(low.cpu().numpy().astype(np.float64) - g[f"{pre}logits"]).max())
    print(f"{name} {pre}: max |d logit| {err:.3e}")
    assert err <= util.LOGIT_TOL, f"{name} {pre} logits: {err:.3e}"
    n = 0
    while f"o{n}_out_hw" in g:
        hw = tuple(int(v) for v in g[f"o{n}_out_hw"])
        lg = ops.upsample_bilinear_ac(low, hw).cpu()
        ref_am = np.unpackbits(g[f"{pre}o{n}_argmax_bits"])[:B * hw[0] * hw[1]].reshape(B, *hw)
        util.assert_argmax_exact(lg, ref_am, what=f"{name} {pre} out {hw}")
        gt = torch.from_numpy(np.concatenate([synth.make_episode(int(s), shot=shot, height=H, width=H, out_hw=hw)["qry_mask"]
                                              for s in seeds]))
        loss = F.cross_entropy(lg, gt, ignore_index=255).item()
        want = float(g[f"{pre}o{n}_loss"])
        assert abs(loss - want) <= 1e-4 * max(1.0, abs(want)), (name, pre, hw, loss, want)
        n += 1
    return err


@pytest.mark.parametrize("name", ["canet_small", "canet_small5", "canet_full"])
def test_canet_matches_reference_golden_over_three_passes(hip_lib, dev, name):
    """Pass 0 from a zero history; passes 1 and 2 are fed OUR softmax of the pass before through the table path (slots), not
    the reference's: the whole loop is what is compared."""
    g = util.gold(name)
    seeds, shot, H = g["seeds"], int(g["shot"]), int(g["H"])
    B = len(seeds)
    net = _net(dev)
    sup, msk, qry = _batch(seeds, shot, H, dev)
    h, w = net.feature_hw(H, H)
    table = torch.zeros((B + 3, 2, h, w), device=dev)
    rows = torch.arange(B, dtype=torch.int32, device=dev) + 2               # not rows 0..B-1: a mis-addressed table shows
    none = torch.full((B,), -1, dtype=torch.int32, device=dev)
    for p in range(3):
        with torch.no_grad():
            low = net.lowres_slots(sup, msk, qry, table, none if p == 0 else rows, rows).clone()
        if p == 0:          # the stages in pipeline order, so that a failure names the first one that is off
            eng = net._engine_for(dev)["canet"]
            _close(eng.last_z.cpu().numpy(), g["z"], 2e-5, f"{name} support vector")
            _close(_sample(eng.last_layer5, H), g["layer5_s"], 2e-5, f"{name} layer5")
            _close(_sample(eng.last_layer55, H), g["layer55_s"], 1e-4, f"{name} layer55")
            _close(_sample(eng.last_aspp_in, H), g["aspp_in_s"], 1e-4, f"{name} ASPP input")
        _check_outputs(g, f"p{p}_", low, seeds, shot, H, name)
    # the reference's own calling convention on pass 1: a history tensor [B,1,2,h,w] (here: the reference's softmax of pass 0)
    hist = torch.softmax(torch.from_numpy(g["p0_logits"]), dim=1)[:, None].to(dev)
    with torch.no_grad():
        low = net(sup, msk, qry, False, history_mask=hist)
    assert float(np.abs(low.cpu().numpy().astype(np.float64) - g["p1_logits"]).max()) <= util.LOGIT_TOL


def test_history_false_model_matches_its_fixture(hip_lib, dev):
    g = util.gold("canet_small")
    seeds, H = g["seeds"], int(g["H"])
    net = _net(dev, history=False)
    sup, msk, qry = _batch(seeds, 1, H, dev)
    with torch.no_grad():
        low = net(sup, msk, qry, False)
        ignored = net(sup, msk, qry, False, history_mask=torch.rand((len(seeds), 1, 2, 13, 13), device=dev))
    _check_outputs(g, "nh_p0_", low, seeds, 1, H, "canet_small history=False")
    assert torch.equal(low, ignored)


# -- protocol --------------------------------------------------------------------------------------------------------------------
def _round_data(n=30, pool=2):
    from pemp_amd.entry import canet as entry
    return entry.SyntheticHistoryEpisodes(n, 5678, 1, split=0, height=97, width=97, pool=pool)


def test_a_round_with_repeating_keys_is_the_same_at_batch_1_4_and_25(hip_lib, dev, exact_eval_variants):
    from pemp_amd.entry import canet as entry
    net = _net(dev)
    rows = []
    for batch in (1, 4, 25):
        data = _round_data()
        data.sample_tasks()
        keys = [data.history_key(i) for i in range(len(data))]
        assert len(set(keys)) < len(keys) / 2                               # keys repeat: the history path is exercised
        ev = entry.Evaluator(net, device=dev)
        r, classes = ev.eval_round(data, batch=batch)
        rows.append(r.cpu())
        assert classes == [k[0] for k in keys]
    assert torch.equal(rows[0], rows[1]) and torch.equal(rows[0], rows[2])
    # the history matters for these rows: the same round with every key forgotten after each step differs
    data = _round_data()
    data.sample_tasks()
    ev = entry.Evaluator(net, device=dev)
    ev.reset_history(len(data), 97, 97)
    fresh = []
    for i in range(len(data)):
        inputs, qry_msk, _ = data.task(i)
        ev.slot_of = {}
        fresh.append(ev.test_step_history([(inputs, qry_msk)], [data.history_key(i)]).cpu())
    assert not torch.equal(torch.cat(fresh), rows[0])


def test_graph_replay_equals_eager_with_other_slots_than_captured(hip_lib, dev, exact_eval_variants):
    net = _net(dev)
    sup, msk, qry = _batch([21, 22, 23], 1, 97, dev)
    h, w = net.feature_hw(97, 97)
    gen = torch.Generator().manual_seed(9)
    init = torch.rand((8, 2, h, w), generator=gen).to(dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    steps = [(i32([0, 1, 2]), i32([3, 4, 5])), (i32([5, -1, 3]), i32([6, 0, -1])), (i32([6, 0, 4]), i32([1, 2, 7]))]
    results = []
    for graphed in (False, True):
        table = init.clone() if not graphed else results[0][2]              # the graph's table: one buffer for all replays
        if graphed:
            table.copy_(init)
        outs = []
        with torch.no_grad():
            for rs, ws in steps:
                fn = net.lowres_graphed_slots if graphed else net.lowres_slots
                outs.append(fn(sup, msk, qry, table, rs, ws).clone())
        results.append((outs, table.clone(), table))
    for a, b in zip(results[0][0], results[1][0]):
        assert torch.equal(a, b)
    assert torch.equal(results[0][1], results[1][1])
    assert not torch.equal(results[0][0][0], results[0][0][1])              # the slots change the result
    with torch.no_grad():                                                   # the tensor form through the shared graph path
        hist = init[:3][:, None].contiguous()
        eager = net.lowres(sup, msk, qry, hist)[0].clone()
        assert torch.equal(net.lowres_graphed(sup, msk, qry, hist)[0], eager)


def test_evaluator_rounds_match_a_python_loop_with_a_host_history(hip_lib, dev):
    """Two rounds through entry.canet.Evaluator against the reference's own loop body: ``model(...)`` per episode, the softmax
    kept in a host dict by key, the dict emptied at ``sample_tasks`` (so a second round starts from an empty table)."""
    from pemp_amd.core.metrics import FewShotMetric
    from pemp_amd.entry import canet as entry
    net = _net(dev)
    data = _round_data(n=12, pool=2)
    ev = entry.Evaluator(net, device=dev)
    loss, miou, biou = ev.start_eval_loop(data, 20, 0, te_epochs=2, batch=4)
    data.reset_sampler()
    labels = entry.get_val_labels(0)
    want = {"loss": [], "miou": [], "biou": []}
    for _ in range(2):
        data.sample_tasks()
        history, metric, losses = {}, FewShotMetric(20), []
        with torch.no_grad():
            for i in range(len(data)):
                (sup, msk, qry), qry_msk, cls = data.task(i)
                key = data.history_key(i)
                hist = history.get(key)
                low = net(sup.to(dev), msk.to(dev), qry.to(dev), False, history_mask=None if hist is None else hist.to(dev))
                history[key] = torch.softmax(low, dim=1).cpu()[:, None]
                gt = qry_msk[0].to(dev)
                out = F.interpolate(low, tuple(gt.shape[-2:]), mode="bilinear", align_corners=True)
                losses.append(F.cross_entropy(out, gt, ignore_index=255).item())
                metric.update(out.argmax(1).cpu().numpy(), qry_msk[0].numpy(), cls.tolist())
        assert len(history) < len(data)                                     # keys repeated inside the round
        want["loss"].append(np.mean(losses))
        want["miou"].append(metric.mIoU(labels)[1])
        want["biou"].append(metric.mIoU(labels, binary=True)[1])
    assert np.abs(ev.round_miou.mean(axis=1) - np.array(want["miou"])).max() <= 1e-6
    assert np.abs(ev.round_biou.mean(axis=1) - np.array(want["biou"])).max() <= 1e-6
    assert abs(loss - float(np.mean(want["loss"]))) <= 1e-4
    pred, l1 = ev.test_step(*data.task(0)[:2])
    assert pred.shape[0] == 1 and np.isfinite(l1)
