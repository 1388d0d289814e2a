"""PFENet head training on the GPU: whole training steps against the reference-made fixtures (tests/golden/
make_golden_pfenet_train.py), the train-mode trunk against their feature samples and BatchNorm statistics, the head alone against
the torch restatement (tests/pfenet_ref.py) on the engine's own trunk features, a five-step trajectory, the trainer's plumbing and
the ``train_head`` command.  Everything at 97 x 97 (a 13 x 13 feature map).  The adjoint kernels have their own module,
tests/test_pfenet_bwd_ops_gpu.py."""
import numpy as np
import pytest
import torch

from tests import pfenet_ref, util

pytestmark = pytest.mark.gpu

STEP_CASES = ["pfenet_trainstep", "pfenet_trainstep5", "pfenet_trainstep_p0"]


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


def _state_dict(shot):
    from pemp_amd import synth
    from pemp_amd.networks.pfenet import WGEN_SEED, ModelClass
    return synth.wgen_state_dict_for(ModelClass(shot, None), WGEN_SEED)


def _trainer(dev, shot, drop=True, sd=None, **kw):
    from pemp_amd.networks.pfenet import ModelClass
    from pemp_amd.train_pfenet import PFENetTrainer
    net = ModelClass(shot, None)
    net.load_state_dict(_state_dict(shot) if sd is None else sd)
    tr = PFENetTrainer(net, device=dev, **kw)
    tr.eng.drop_scale = 1.0 if drop else 0.0
    return tr, net


def _inputs(name):
    from pemp_amd import synth
    g = util.gold(name)
    shot, H = int(g["shot"]), int(g["H"])
    b = synth.make_batch([int(s) for s in g["seeds"]], shot=shot, height=H, width=H, out_hw=(H, H))
    sup, msk, qry, gt = (torch.from_numpy(b[k]) for k in ("sup_img", "sup_mask", "qry_img", "qry_mask"))
    draws = {k: torch.from_numpy(g["draws__" + k]) for k in pfenet_ref.DROPS}
    return g, sup, msk, qry, gt.reshape(-1, H, H), draws


_STEPS = {}


def _fixture_step(dev, name):
    """One forward + backward on the fixture's inputs and draws, computed once per case and shared (nothing changes it)."""
    if name not in _STEPS:
        g, sup, msk, qry, gt, draws = _inputs(name)
        tr, net = _trainer(dev, int(g["shot"]), bool(g["dropout"]))
        tr.eng.draws = {k: v.to(dev) for k, v in draws.items()}
        loss, aux, low = tr.forward_backward(sup.to(dev), msk.to(dev), qry.to(dev), gt.to(dev))
        torch.cuda.synchronize()
        _STEPS[name] = (g, tr, net, float(loss), float(aux), low, (sup, msk, qry, gt, draws))
    return _STEPS[name]


def _kernel_bound(got, ref64, ref32, what):
    e_hip = float((got.double().cpu() - ref64).abs().max())
    e_ref = float((ref32.double() - ref64).abs().max())
    scale = float(ref64.abs().max())
    print(f"  {what}: |hip - f64| {e_hip:.2e}, |ref f32 - f64| {e_ref:.2e}, scale {scale:.2e}")
    assert e_hip <= 3 * e_ref + 1e-6 * scale, (what, e_hip, e_ref, scale)


@pytest.mark.parametrize("name", ["pfenet_trainstep", "pfenet_trainstep5"])
def test_trunk_in_train_mode_matches_reference(hip_lib, dev, name):
    """The S + 1 batch-statistics passes: the query's layer-3 / layer-4 samples and the prior at the bounds tests/test_pfenet_gpu.py
    applies to its eval fixtures (2e-5 relative, 1e-4 absolute), the three stored BatchNorms' running statistics after the step at
    the kernel-test bound against float64, ``num_batches_tracked`` = S + 1."""
    g, tr, net, *_ = _fixture_step(dev, name)
    g64 = util.gold(name + "_f64")
    for key, feat in (("l3_s", tr.eng.last_layer3), ("l4_s", tr.eng.last_layer4)):
        got, ref = feat.permute(0, 3, 1, 2)[:, ::64].cpu().numpy().astype(np.float64), g[key].astype(np.float64)
        err, bound = np.abs(got - ref).max(), 2e-5 * max(1.0, np.abs(ref).max())
        print(f"  {name} {key}: max err {err:.2e} (bound {bound:.2e})")
        assert err <= bound, (key, err, bound)
    err = np.abs(tr.eng.last_prior_bin0.cpu().numpy() - g["prior_bin0"]).max()
    print(f"  {name} prior at bin 0: max err {err:.2e}")
    assert err <= 1e-4
    mods = dict(net.named_modules())
    for key in [k for k in g.files if k.startswith("bn__")]:
        mod, attr = key[len("bn__"):].rsplit(".", 1)
        got = getattr(mods[mod], attr)
        if attr == "num_batches_tracked":
            assert int(got) == int(g["shot"]) + 1 == int(g[key]), key
        else:
            _kernel_bound(got, torch.from_numpy(g64["bn64__" + key[len("bn__"):]]), torch.from_numpy(g[key]), f"{name} {mod}.{attr}")


@pytest.mark.parametrize("name", STEP_CASES)
def test_train_step_gradients_match_reference(hip_lib, dev, name):
    """One forward + backward with the fixture's Dropout2d draws against the REFERENCE's own float32 and float64 steps:
    util.check_gradients (3 x the reference's float32 error + 3e-3, per tensor, L2 / max / norm), the low-resolution and inner
    logits within util.LOGIT_TOL of float64, both losses within 2 x that; the trunk has no gradient."""
    g, tr, net, loss, aux, low, _ = _fixture_step(dev, name)
    g64 = util.gold(name + "_f64")
    params = dict(net.named_parameters())
    worst = util.check_gradients(g, g64, params, name, eps=3e-3)
    for k, p in params.items():
        if k.startswith(pfenet_ref.TRUNK):
            assert not p.requires_grad and p.grad is None, k
    dl = float((low.double().cpu() - torch.from_numpy(g64["low64"])).abs().max())
    di = [float((o.double().cpu() - torch.from_numpy(g64[f"inner64__{k}"])).abs().max()) for k, o in enumerate(tr.last_inner)]
    print(f"{name}: worst gradient ratio to its bound {worst:.3f}; |logits - f64| {dl:.2e} (reference f32: "
          f"{np.abs(g['low32'] - g64['low64']).max():.2e}), inner {['%.2e' % v for v in di]}; loss {loss:.6f} (f64 "
          f"{float(g64['loss64']):.6f}), aux {aux:.6f} (f64 {float(g64['aux64']):.6f})")
    assert dl <= util.LOGIT_TOL and max(di) <= util.LOGIT_TOL
    assert abs(loss - float(g64["loss64"])) <= 2 * util.LOGIT_TOL and abs(aux - float(g64["aux64"])) <= 2 * util.LOGIT_TOL


@pytest.mark.parametrize("name", ["pfenet_trainstep", "pfenet_trainstep5"])
def test_head_gradients_match_the_restatement_on_the_engines_own_trunk(hip_lib, dev, name):
    """The head alone: tests/pfenet_ref.py in float32 and float64 on the ENGINE's trunk features, masks and prior with the same
    draws, whole tensors (util.check_gradients_live) -- what is left when the trunk's rounding is taken out."""
    g, tr, net, loss, aux, low, (sup, msk, qry, gt, draws) = _fixture_step(dev, name)
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    hip = {k: dict(net.named_parameters())[k].grad.detach().cpu().clone() for k in pfenet_ref.head_keys(sd) if k in dict(net.named_parameters())}
    feats = [t.detach().cpu() for t in tr.eng.last_head_inputs]
    out = {dt: pfenet_ref.head_step(*feats, gt, sd, int(g["shot"]), dt, draws, drop=bool(g["dropout"])) for dt in (torch.float32, torch.float64)}
    o32, o64 = out[torch.float32], out[torch.float64]
    assert abs(loss - o64[0]) <= 3 * abs(o32[0] - o64[0]) + 1e-5 and abs(aux - o64[1]) <= 3 * abs(o32[1] - o64[1]) + 1e-5
    util.check_gradients_live(hip, o32[4], o64[4], name + " head only")


def test_trajectory(hip_lib, dev):
    """Five SGD steps (lr 1e-4, momentum 0.9, wd 1e-4, every p = 0) against the reference's trajectory: per step and per loss
    |hip - f64| <= 3 |ref32 - f64| + 2 LOGIT_TOL, and the total falls below half."""
    t = util.gold("pfenet_trajectory")
    g, sup, msk, qry, gt, _ = _inputs("pfenet_trainstep_p0")
    tr, net = _trainer(dev, 1, drop=False, lr=float(t["lr"]), momentum=float(t["momentum"]), weight_decay=float(t["weight_decay"]))
    assert tr.max_norm == 0.0
    steps = [tuple(float(v) for v in tr.train_step(sup, msk, qry, qry_msk=gt)) for _ in range(5)]
    print("  trajectory: hip", [(round(a, 5), round(b, 5)) for a, b in steps], "f64 total", (t["losses64"] + t["aux64"]).round(5))
    for k, (l, a) in enumerate(steps):
        assert abs(l - t["losses64"][k]) <= 3 * abs(t["losses32"][k] - t["losses64"][k]) + 2 * util.LOGIT_TOL, (k, l)
        assert abs(a - t["aux64"][k]) <= 3 * abs(t["aux32"][k] - t["aux64"][k]) + 2 * util.LOGIT_TOL, (k, a)
    assert sum(steps[4]) < 0.5 * sum(steps[0])


def test_trainer_plumbing(hip_lib, dev):
    """Identical steps from identical states give identical bits; ``use_graph`` and ``query = 2`` raise; ``loss_coef = 0`` leaves the
    ``inner_cls`` gradients exactly zero and every other gradient equal to a run without the auxiliary branch; after a step
    ``model.eval()`` serves the updated head and the moved running statistics, bit for bit what a fresh model loaded from the saved
    state_dict gives, and a ``train()``-mode ``model(...)`` still raises."""
    from pemp_amd.networks.pfenet import ModelClass
    from pemp_amd.train_pfenet import PFENetTrainer
    g, sup, msk, qry, gt, draws = _inputs("pfenet_trainstep")
    dsup, dmsk, dqry, dgt = sup.to(dev), msk.to(dev), qry.to(dev), gt.to(dev)
    with pytest.raises(ValueError, match="eagerly"):
        PFENetTrainer(ModelClass(1, None), device=dev, use_graph=True)
    grads = []
    for coef, skip in ((1.0, False), (1.0, False), (0.0, False), (0.0, True)):
        tr, net = _trainer(dev, 1, loss_coef=coef)
        tr.eng.draws, tr.eng.skip_aux = {k: v.to(dev) for k, v in draws.items()}, skip
        tr.forward_backward(dsup, dmsk, dqry, dgt)
        torch.cuda.synchronize()
        grads.append({k: p.grad.detach().clone() for k, p in net.named_parameters() if p.requires_grad})
    assert all(torch.equal(grads[0][k], grads[1][k]) for k in grads[0])
    for k in grads[2]:
        if k.startswith("inner_cls."):
            assert bool((grads[2][k] == 0).all()) and bool((grads[3][k] == 0).all()), k
        else:
            assert torch.equal(grads[2][k], grads[3][k]), k
    with pytest.raises(ValueError, match="one query"):
        tr.forward_backward(dsup, dmsk, torch.cat((dqry, dqry), dim=1), dgt)
    # evaluation after a step
    tr, net = _trainer(dev, 1)
    net.eval()
    with torch.no_grad():
        before = net(dsup, dmsk, dqry).clone()
    net.train()
    loss, aux = tr.train_step(sup, msk, qry, qry_msk=gt)
    assert np.isfinite(float(loss)) and np.isfinite(float(aux))
    with pytest.raises(NotImplementedError, match="PFENet is an inference path here"):
        net(dsup, dmsk, dqry)
    after = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    sd0 = _state_dict(1)
    assert not torch.equal(after["cls.3.weight"], sd0["cls.3.weight"]) and torch.equal(after["layer0.0.weight"], sd0["layer0.0.weight"])
    assert not torch.equal(after["layer4.2.bn3.running_mean"], sd0["layer4.2.bn3.running_mean"])
    net.eval()
    with torch.no_grad():
        got = net(dsup, dmsk, dqry)
        fresh = ModelClass(1, None)
        fresh.load_state_dict(after)
        assert torch.equal(got, fresh.to(dev).eval()(dsup, dmsk, dqry))
    assert not torch.equal(got, before)


def test_train_head_command_end_to_end(hip_lib, dev, tmp_path):
    """``train_head``: one epoch of 2 steps at 97 x 97 + evaluation through the command layer writes ckpt.pth / bestckpt.pth with
    the reference's keys, shapes and dtypes, which ``test`` loads."""
    from pemp_amd.entry import pfenet as e
    common = ["split=0", f"g.model_dir={tmp_path}", "data.height=97", "data.width=97", "data.test_n=6", "te.epochs=1", "data.test_bs=2"]

    def run(*argv):
        try:
            return e.ex.run_commandline(["prog", *argv])
        finally:
            for ing in e.INGREDIENTS[1:] + [e.ex]:
                ing._updates.clear()
                ing._cfg = None

    msg = run("train_head", "with", *common, "tr.total_epochs=1", "data.train_n=4", "data.bs=2", "tr.lr=0.0001", "ckpt=wgen")
    d = tmp_path / "pfenet" / "1"
    assert sorted(p.name for p in d.iterdir()) == ["bestckpt.pth", "ckpt.pth"] and "pfenet/1" in msg.replace("\\", "/")
    sd = torch.load(str(d / "ckpt.pth"), map_location="cpu")
    assert [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()] == util.key_spec("pfenet")
    w0 = _state_dict(1)
    assert not torch.equal(sd["cls.3.weight"], w0["cls.3.weight"]) and torch.equal(sd["layer0.0.weight"], w0["layer0.0.weight"])
    assert int(sd["layer0.1.num_batches_tracked"]) == 2 * 2                   # two steps of S + 1 = 2 trunk calls
    out = run("test", "with", *common, "exp_id=1")
    assert out.startswith("Loss:") and "mIoU" in out
    with pytest.raises(ValueError, match="one query"):
        run("train_head", "with", *common, "ckpt=wgen", "query=2")
