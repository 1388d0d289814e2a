"""PFENet on the HIP path: the new kernels (csrc/pfenet.hip) against torch float64 on the CPU, the model against the
reference-made fixtures (tests/golden/make_golden_pfenet.py), and the evaluation protocol (batching, graph replay,
entry.pfenet's Evaluator)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import util

pytestmark = pytest.mark.gpu
WGEN_SEED = 1259


# -- kernels --------------------------------------------------------------------------------------------------------------------
def _prior_ref(q, s, m, S):
    """networks/pfenet.py:201-227 in float64 on the operands the kernel sees (the masked support fl32(m * s)).  -> (prior
    [B,h,w], spread [B,S]: max - min over the query pixels of each shot's similarity before its normalisation)."""
    B, h, w, C = q.shape
    sm = (s * m[..., None]).double()                    # fp32 product, then exact in f64
    qd = q.double().reshape(B, h * w, C)
    out = torch.zeros(B, h * w, dtype=torch.float64)
    spread = torch.zeros(B, S, dtype=torch.float64)
    for b in range(B):
        for i in range(S):
            sv = sm[b * S + i].reshape(h * w, C)
            sim = (sv @ qd[b].T) / (sv.norm(dim=1)[:, None] * qd[b].norm(dim=1)[None, :] + 1e-7)
            sim = sim.max(0)[0]
            spread[b, i] = sim.max() - sim.min()
            out[b] += (sim - sim.min()) / (sim.max() - sim.min() + 1e-7)
    return (out / S).reshape(B, h, w), spread


def _feats(shape, gen):
    return (torch.rand(shape, generator=gen) - 0.3).clamp_min(0.0)          # post-ReLU-like


def _mask(shape, gen):
    """Support masks with fractional values (bilinear-resized masks), at least one foreground pixel per image."""
    m = (torch.rand(shape, generator=gen) > 0.4).float() * torch.rand(shape, generator=gen).clamp_min(0.5)
    m.view(shape[0], -1)[:, 0] = 1.0
    return m


@pytest.mark.parametrize("S,h,w,C", [(1, 7, 7, 64), (5, 7, 7, 96), (1, 13, 13, 2048), (5, 13, 13, 256), (1, 9, 11, 128),
                                     (2, 51, 51, 512)])
def test_prior_mask_matches_float64(hip_lib, dev, S, h, w, C):
    """Every episode and shot with a real mask and varying query pixels: 51 x 51 = 41 support tiles, C = 2048 (the long K
    loop), 9 x 11 (tails in both tile directions), episode b = 1 (its query rows are found by b = bs / S)."""
    from pemp_amd import ops
    gen = torch.Generator().manual_seed(100 * S + h + C)
    B = 2
    q, s, m = _feats((B, h, w, C), gen), _feats((B * S, h, w, C), gen), _mask((B * S, h, w), gen)
    ref, spread = _prior_ref(q, s, m, S)
    assert (spread > 1e-3).all(), spread                # no episode or shot is degenerate: the check compares real values
    got = ops.prior_mask(q.to(dev), s.to(dev), m.to(dev), S)
    err = (got.cpu().double() - ref).abs().max().item()
    print(f"prior S={S} {h}x{w} C={C}: max err {err:.3e}, min spread {spread.min().item():.3e}")
    assert err < 1e-4, err
    assert ref.abs().max().item() > 0.5
    again = ops.prior_mask(q.to(dev), s.to(dev), m.to(dev), S)
    assert torch.equal(got, again)                      # bit-stable


@pytest.mark.parametrize("h,w", [(1, 1), (13, 13)])
def test_prior_mask_edge_cases(hip_lib, dev, h, w):
    """Three 2-shot episodes: episode 0's shot 0 has an empty mask (its similarity is 0 everywhere and normalises to 0, so the
    episode's prior is half its shot 1 map), episode 1 has one query vector at every pixel (constant similarity -> exactly
    0), episode 2 is ordinary.  A 1-pixel map is constant by definition.  Then the empty shot alone (1-shot): exactly 0."""
    from pemp_amd import ops
    gen = torch.Generator().manual_seed(7 + h)
    B, S, C = 3, 2, 128
    q, s, m = _feats((B, h, w, C), gen), _feats((B * S, h, w, C), gen), _mask((B * S, h, w), gen)
    m[0] = 0.0
    q[1] = q[1, 0, 0]
    ref, spread = _prior_ref(q, s, m, S)
    got = ops.prior_mask(q.to(dev), s.to(dev), m.to(dev), S).cpu()
    assert (got[1] == 0).all()
    assert (got.double() - ref).abs().max().item() < 1e-4
    if h * w == 1:
        assert (got == 0).all()
    else:
        assert spread[0, 1] > 1e-3 and spread[2].min() > 1e-3 and ref[0].abs().max() > 0.2 and ref[2].abs().max() > 0.5
        shot1, _ = _prior_ref(q[:1], s[1:2], m[1:2], 1)
        assert (got[0].double() - shot1[0] / 2).abs().max().item() < 1e-4      # the empty shot adds exactly 0
    alone = ops.prior_mask(q[:1].to(dev), s[:1].to(dev), m[:1].to(dev), 1).cpu()
    assert (alone == 0).all()


@pytest.mark.parametrize("hin,outs", [(51, (60, 30, 15, 8)), (13, (60,))])
def test_adaptive_avgpool_matches_torch(hip_lib, dev, hin, outs):
    from pemp_amd import ops
    gen = torch.Generator().manual_seed(hin)
    x = torch.randn((2, hin, hin, 64), generator=gen)
    for o in outs:
        wide = torch.full((2, o, o, 160), 7.0, device=dev)
        ops.adaptive_avgpool(x.to(dev), o, out=wide[..., 32:96])              # a channel slice of a wider buffer
        ref = F.adaptive_avg_pool2d(x.double().permute(0, 3, 1, 2), o).permute(0, 2, 3, 1)
        assert (wide[..., 32:96].cpu().double() - ref).abs().max().item() < 1e-5, o
        assert (wide[..., :32] == 7.0).all() and (wide[..., 96:] == 7.0).all()


@pytest.mark.parametrize("hin,win,hout,wout", [(13, 13, 51, 51), (51, 51, 8, 8), (1, 1, 5, 5), (5, 7, 1, 1), (1, 4, 3, 1),
                                               (51, 51, 60, 60)])
def test_resize_bilinear_ac_matches_torch(hip_lib, dev, hin, win, hout, wout):
    from pemp_amd import ops
    gen = torch.Generator().manual_seed(hin * 100 + hout)
    big = torch.randn((2, hin, win, 48), generator=gen)
    x = big[..., 8:40]                                                         # slice in
    out = torch.full((2, hout, wout, 64), 3.0, device=dev)
    ops.resize_bilinear_ac(big.to(dev)[..., 8:40], (hout, wout), out=out[..., 16:48])    # slice out
    ref = F.interpolate(x.double().permute(0, 3, 1, 2), (hout, wout), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    # the interpolation weights are computed in fp32 (scale * dst, as ATen does): each is off by up to ~2 ulp(dst), which
    # moves a result by that times the difference of two neighbours (<= 2 max|x|)
    tol = max(1e-6, 2 * 2.0 ** -23 * max(hout, wout) * 2 * x.abs().max().item())
    assert (out[..., 16:48].cpu().double() - ref).abs().max().item() < tol
    assert (out[..., :16] == 3.0).all() and (out[..., 48:] == 3.0).all()
    # NCHW output through the strides (the model's logits) and a binarised mask plane read in place
    nchw = torch.empty((2, 32, hout, wout), device=dev)
    ops.resize_bilinear_ac(big.to(dev)[..., 8:40], (hout, wout), out=nchw.permute(0, 2, 3, 1))
    assert (nchw.cpu().double() - ref.permute(0, 3, 1, 2)).abs().max().item() < tol
    planes = (torch.rand((2, 2, hin, win), generator=gen) > 0.5).float()
    planes[:, 0, 0, 0] = 0.5                                                    # not == 1: read as 0
    got = ops.resize_bilinear_ac(planes.to(dev)[:, 0].unsqueeze(-1), (hout, wout), binarize=True)
    ref_m = F.interpolate((planes[:, :1] == 1).double(), (hout, wout), mode="bilinear", align_corners=True)
    assert (got[..., 0].cpu().double() - ref_m[:, 0]).abs().max().item() < max(1e-6, 4 * 2.0 ** -23 * max(hout, wout))


@pytest.mark.parametrize("S", [1, 5])
def test_weighted_gap_matches_float64(hip_lib, dev, S):
    from pemp_amd import ops
    gen = torch.Generator().manual_seed(S)
    B, h, w, C = 2, 13, 13, 256
    f = _feats((B * S, h, w, C + 32), gen)
    m = torch.rand((B * S, h, w), generator=gen) * (torch.rand((B * S, h, w), generator=gen) > 0.5)
    got = ops.weighted_gap(f.to(dev)[..., :C], m.to(dev), S)
    fd, md = f[..., :C].double(), m.double()
    g = (fd * md[..., None]).sum((1, 2)) / (md.sum((1, 2))[:, None] + 5e-4)       # pfenet.py:15-20
    ref = g.view(B, S, C).mean(1)
    assert (got.cpu().double() - ref).abs().max().item() < 1e-5 * max(1.0, ref.abs().max().item())


# -- model against the reference's fixtures --------------------------------------------------------------------------------------
def _net(dev, shot):
    from pemp_amd.networks import pfenet as m
    net = m.PFENet(shot, None)
    net.load_state_dict(util.wgen_state_dict("pfenet", seed=WGEN_SEED))
    return net.to(dev).eval()


def _batch(seeds, shot, H, dev):
    from pemp_amd import synth
    b = synth.make_batch([int(s) for s in seeds], shot=shot, height=H, width=H, out_hw=(H, H))
    return [torch.from_numpy(b[k]).to(dev) for k in ("sup_img", "sup_mask", "qry_img")]


def _close(got, ref, rel, what):
    ref = np.asarray(ref, np.float64)
    err = np.abs(np.asarray(got, np.float64) - ref).max()
    bound = rel * max(1.0, np.abs(ref).max())
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"
    return err


@pytest.mark.parametrize("name", ["pfenet_small", "pfenet_small5", "pfenet_full"])
def test_pfenet_matches_reference_golden(hip_lib, dev, name):
    g = util.gold(name)
    seeds, shot, H = g["seeds"], int(g["shot"]), int(g["H"])
    B = len(seeds)
    net = _net(dev, shot)
    sup, msk, qry = _batch(seeds, shot, H, dev)
    n = 0
    while f"o{n}_out_hw" in g:
        hw = tuple(int(v) for v in g[f"o{n}_out_hw"])
        with torch.no_grad():
            out = net(sup, msk, qry, None, hw)
        eng = net._engine_for(dev)["pfenet"]
        if n == 0:          # the stages in pipeline order, so that a failure names the first one that is off
            q4 = eng.last_layer4[B * shot:].permute(0, 3, 1, 2).cpu().numpy()
            q4 = q4[:, ::16] if H <= 97 else q4[:, ::32, ::5, ::5]
            _close(q4, g["q4_s"], 2e-5, f"{name} layer 4")
            for k in range(4):
                err = np.abs(eng.last_bins[k].cpu().numpy() - g[f"prior_bin{k}"]).max()
                assert err <= 1e-4, f"{name} prior at bin {k}: {err:.3e}"
            _close(eng.last_supp_vec.cpu().numpy(), g["supp_vec"], 2e-5, f"{name} support vector")
            r1 = eng.last_res1_in.permute(0, 3, 1, 2).cpu().numpy()
            r1 = r1[:, ::16] if H <= 97 else r1[:, ::32, ::5, ::5]
            _close(r1, g["res1_in_s"], 1e-4, f"{name} res1 input")
        # logits at util.LOGIT_TOL, arg-max exact outside util.MARGIN = 2 * LOGIT_TOL: the Wgen PFENet logits reach ~70 (the
        # other models' 20 * cos stay within 20), but the measured error stays far inside the absolute bound (1.9e-4 ..
        # 2.4e-4 over these fixtures), so the range does not force a wider one
        lg = out.cpu()
        ref = g[f"o{n}_logits"]
        sampled = lg.numpy() if H <= 97 else lg[:, :, ::7, ::7].numpy()
        err = float(np.abs(sampled.astype(np.float64) - ref).max())
        print(f"{name} out {hw}: max |d logit| {err:.3e}")
        assert err <= util.LOGIT_TOL, f"{name} logits, out {hw}: {err:.3e}"
        ref_am = np.unpackbits(g[f"o{n}_argmax_bits"])[:B * hw[0] * hw[1]].reshape(B, *hw)
        util.assert_argmax_exact(lg, ref_am, what=f"{name} out {hw}")
        from pemp_amd import synth
        gt = torch.from_numpy(np.concatenate([synth.make_episode(int(s), shot=shot, height=H, width=H, out_hw=hw)["qry_mask"]
                                              for s in seeds]))
        loss = F.cross_entropy(lg, gt, ignore_index=255).item()
        assert abs(loss - float(g[f"o{n}_loss"])) <= 1e-4 * max(1.0, abs(float(g[f"o{n}_loss"]))), (name, hw, loss)
        n += 1


# -- protocol --------------------------------------------------------------------------------------------------------------------
def test_batch_of_one_equals_batch_of_k_and_graph_replay_equals_eager(hip_lib, dev, exact_eval_variants):
    net = _net(dev, 1)
    seeds = [21, 22, 23]
    sup, msk, qry = _batch(seeds, 1, 97, dev)
    with torch.no_grad():
        together = net.lowres(sup, msk, qry)[0].clone()
        for i in range(len(seeds)):
            alone = net.lowres(sup[i:i + 1], msk[i:i + 1], qry[i:i + 1])[0]
            assert torch.equal(alone, together[i:i + 1]), i
        graphed = net.lowres_graphed(sup, msk, qry)[0].clone()
        replay = net.lowres_graphed(sup, msk, qry)[0].clone()
    assert torch.equal(graphed, together) and torch.equal(replay, together)


def test_evaluator_round_matches_per_episode_forwards(hip_lib, dev):
    from pemp_amd.core.metrics import FewShotMetric
    from pemp_amd.entry import pfenet as entry
    net = _net(dev, 1)
    data = entry.SyntheticEpisodes(6, 5678, 1, split=0, height=97, width=97)
    ev = entry.Evaluator(net, device=dev)
    loss, miou, biou = ev.start_eval_loop(data, 20, 0, te_epochs=1)
    data.reset_sampler()
    data.sample_tasks()
    metric = FewShotMetric(20)
    losses = []
    with torch.no_grad():
        for i in range(len(data)):
            (sup, msk, qry), qry_msk, cls = data.task(i)
            gt = qry_msk[0].to(dev)
            out = net(sup.to(dev), msk.to(dev), qry.to(dev), None, tuple(gt.shape[-2:]))
            losses.append(F.cross_entropy(out, gt, ignore_index=255).item())
            metric.update(out.argmax(1).cpu().numpy(), qry_msk[0].numpy(), cls.tolist())
    labels = entry.get_val_labels(0)
    assert abs(float(np.mean(miou)) - metric.mIoU(labels)[1]) <= 1e-6
    assert abs(float(np.mean(biou)) - metric.mIoU(labels, binary=True)[1]) <= 1e-6
    assert abs(loss - float(np.mean(losses))) <= 1e-4
    pred, l1 = ev.test_step(*data.task(0)[:2])
    assert pred.shape[0] == 1 and np.isfinite(l1)
