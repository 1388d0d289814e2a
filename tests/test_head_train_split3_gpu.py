"""``trunk_precision="split3"`` of the three head trainers: the frozen trunk's convs on the split3 family with the statistics
epilogue.  One forward + backward per reference-made fixture at the bounds the fp32-chain step is held to (util.check_gradients
with eps 3e-3, logits within util.LOGIT_TOL of float64, losses within twice that), the switch observed through ops.conv2d_stats,
the default path bit for bit, and the command end to end.  Fixtures, state dicts and the pick pinning are those of the three
test_*_train_gpu.py modules."""
import numpy as np
import pytest
import torch

from tests import canet_ref, pfenet_ref, rpmms_ref, util
from tests import test_canet_train_gpu as tc, test_pfenet_train_gpu as tp, test_rpmms_train_gpu as trp
from tests.test_canet_train_gpu import fixed_picks  # noqa: F401  (autouse: one fixed kernel variant per layer, empty pick caches)

pytestmark = pytest.mark.gpu

CASES = [("canet", n) for n in tc.STEP_CASES] + [("pfenet", "pfenet_trainstep"), ("pfenet", "pfenet_trainstep5")] + \
        [("rpmms", n) for n in trp.STEP_CASES]
_RUNS = {}


def _build(dev, family, g, precision, mu0=None):
    """(trainer, net) of the family's fixture configuration; ``precision`` None: built without the keyword."""
    kw = {} if precision is None else {"trunk_precision": precision}
    if family == "canet":
        from pemp_amd.networks import canet
        from pemp_amd.train_canet import CANetTrainer
        net = canet.CaNet(None, init_channels=3, drop_rate=float(g["p"]), history=bool(g["use_history"]), freeze_backbone=True)
        net.load_state_dict(canet_ref.fixture_state_dict(bool(g["use_history"])))
        return CANetTrainer(net, lr=1e-4, device=dev, **kw), net
    if family == "pfenet":
        return tp._trainer(dev, int(g["shot"]), bool(g["dropout"]), **kw)
    from pemp_amd.networks import rpmms
    from pemp_amd.train_rpmms import RPMMsTrainer
    net = rpmms.RPMMs(None, drop_rate=float(g["p"]))
    net.load_state_dict(rpmms_ref.fixture_state_dict())
    if mu0 is not None:
        net.set_pmm_init(mu0)
    return RPMMsTrainer(net.freeze_trunk(), lr=1e-4, device=dev, **kw), net


def _trunk_modules(family, net):
    if family == "canet":
        return [net.encoder]
    if family == "pfenet":
        return [getattr(net, n.rstrip(".")) for n in pfenet_ref.TRUNK]
    return [net.model_res]


def _frozen_convs(eng):
    """Every _FrozenConv handle of an engine: the stem(s) and the bottleneck blocks."""
    from pemp_amd.train_engine import _FrozenConv
    stems = eng.stem if isinstance(eng.stem, list) else [eng.stem]
    out = [c for c, _ in stems]
    for b in list(eng.blocks) + list(getattr(eng, "blocks4", [])):
        out += [b["c1"], b["c2"], b["c3"]] + ([b["ds"][0]] if b["ds"] is not None else [])
    assert out and all(isinstance(c, _FrozenConv) for c in out)
    return out


def _run(dev, family, name, precision, monkeypatch):
    """One forward_backward on the fixture's inputs and draws, computed once per (case, precision) and shared; every call of
    ops.conv2d_stats during it is recorded as (ConvParams, w3 set)."""
    key = (name, precision)
    if key in _RUNS:
        return _RUNS[key]
    from pemp_amd import ops
    calls, real = [], ops.conv2d_stats

    def counting(x, p, *a, **kw):
        calls.append((p, p.w3 is not None))
        return real(x, p, *a, **kw)

    monkeypatch.setattr(ops, "conv2d_stats", counting)
    if family == "canet":
        g, sup, msk, qry, gt, hist, draws = canet_ref.fixture_inputs(name)
        tr, net = _build(dev, family, g, precision)
        tr.eng.draws = {k: v.to(dev) for k, v in draws.items()}
        loss, low = tr.forward_backward(sup.to(dev), msk.to(dev), qry.to(dev), gt.to(dev), history_mask=hist[:, None].to(dev))
        g64 = util.gold(name + "_f64")
        logits, losses = [(low, g64["low64"])], [(float(loss), float(g64["loss64"]))]
    elif family == "pfenet":
        g, sup, msk, qry, gt, draws = tp._inputs(name)
        tr, net = _build(dev, family, g, precision)
        tr.eng.draws = {k: v.to(dev) for k, v in draws.items()}
        loss, aux, low = tr.forward_backward(sup.to(dev), msk.to(dev), qry.to(dev), gt.to(dev))
        g64 = util.gold(name + "_f64")
        logits = [(low, g64["low64"])] + [(o, g64[f"inner64__{k}"]) for k, o in enumerate(tr.last_inner)]
        losses = [(float(loss), float(g64["loss64"])), (float(aux), float(g64["aux64"]))]
    else:
        g, sup, msk, qry, gt, mu0, draws = rpmms_ref.fixture_inputs(name)
        tr, net = _build(dev, family, g, precision, mu0)
        tr.eng.draws = {k: v.to(dev) for k, v in draws.items()}
        loss, outs = tr.forward_backward(sup.to(dev), msk.to(dev), qry.to(dev), gt.to(dev))
        g64 = util.gold(name + "_f64")
        logits = [(o, g64[f"low64_p{q}"]) for q, o in enumerate(outs)]
        losses = list(zip([float(loss), float(tr.last_losses[2]), float(tr.last_losses[1])], [float(v) for v in g64["loss64"]]))
    torch.cuda.synchronize()
    monkeypatch.setattr(ops, "conv2d_stats", real)
    _RUNS[key] = dict(g=g, g64=g64, tr=tr, net=net, logits=[(o.detach().double().cpu(), torch.from_numpy(np.asarray(r))) for o, r in logits],
                      losses=losses, flat=tr.eng.flat.grad.detach().clone(), calls=calls,
                      nbt={k: int(v) for k, v in net.state_dict().items() if k.endswith("num_batches_tracked")})
    return _RUNS[key]


@pytest.mark.parametrize("family,name", CASES)
def test_split3_trunk_step_meets_the_bounds_of_the_fp32_chain_step(hip_lib, dev, monkeypatch, family, name):
    """The bounds of test_*_train_gpu.py::test_train_step_gradients_match_reference, unchanged, on the split3 trunk; the trunk has
    no gradients and its BatchNorm counters advance as on the fp32 chain.  Prints the relative L2 distance to the same trainer's
    "f32_chain" step for the record."""
    s3 = _run(dev, family, name, "split3", monkeypatch)
    f32 = _run(dev, family, name, "f32_chain", monkeypatch)
    rel = float((s3["flat"] - f32["flat"]).double().norm() / f32["flat"].double().norm())
    dl = [float((o - r).abs().max()) for o, r in s3["logits"]]
    dl32 = [float((o - r).abs().max()) for o, r in f32["logits"]]
    print(f"{name} split3 trunk: relative L2 distance of the flat gradient to the f32_chain step {rel:.3e}; |logits - f64| "
          f"{['%.2e' % v for v in dl]} (f32_chain: {['%.2e' % v for v in dl32]}); losses {s3['losses']}")
    worst = util.check_gradients(s3["g"], s3["g64"], dict(s3["net"].named_parameters()), name + " split3 trunk", eps=3e-3)
    print(f"{name} split3 trunk: worst gradient ratio to its bound {worst:.3f}")
    assert max(dl) <= util.LOGIT_TOL
    assert max(abs(a - b) for a, b in s3["losses"]) <= 2 * util.LOGIT_TOL
    trunk = [p for m in _trunk_modules(family, s3["net"]) for p in m.parameters()]
    assert trunk and all(not p.requires_grad and p.grad is None for p in trunk)
    assert s3["nbt"] == f32["nbt"] and max(s3["nbt"].values()) >= 1


@pytest.mark.parametrize("family,name", [("canet", "canet_trainstep"), ("pfenet", "pfenet_trainstep"), ("rpmms", "rpmms_trainstep")])
def test_the_switch_moves_every_admitted_frozen_conv_and_nothing_by_default(hip_lib, dev, monkeypatch, family, name):
    """Under "split3" every frozen conv that engine.split3_admits ran ops.conv2d_stats with w3 set, the stem and every excluded
    conv without; under the default no call carried w3.  "f32_chain" is the trainer built without the keyword, bit for bit."""
    from pemp_amd.engine import split3_admits
    s3 = _run(dev, family, name, "split3", monkeypatch)
    f32 = _run(dev, family, name, "f32_chain", monkeypatch)
    convs = _frozen_convs(s3["tr"].eng)
    prms = {id(c.fwd_params(relu=False, with_bias=False)): c for c in convs}
    admitted = {i for i, c in prms.items() if split3_admits(c.fwd_params(relu=False, with_bias=False))}
    stems = [c for c in convs if c.stem]
    assert stems and all(id(c.fwd_params(relu=False, with_bias=False)) not in admitted for c in stems)
    assert len(admitted) >= 40                                          # a ResNet-50 trunk to layer3: 39 bottleneck convs + 3 downsample convs
    with_w3 = {id(p) for p, has in s3["calls"] if has}
    without = {id(p) for p, has in s3["calls"] if not has}
    assert with_w3 == admitted, (len(with_w3), len(admitted))
    assert not (without & admitted) and all(c.fwd_params(relu=False, with_bias=False).w3 is None
                                            for i, c in prms.items() if i not in admitted)
    assert f32["calls"] and not any(has for _, has in f32["calls"])
    assert all(c.fwd_params(relu=False, with_bias=False).w3 is None for c in _frozen_convs(f32["tr"].eng))
    # the head's own convs stay on the fp32 chain under either switch
    head_calls = [p for p, _ in s3["calls"] if id(p) not in prms]
    assert all(p.w3 is None for p in head_calls)
    assert not torch.equal(s3["flat"], f32["flat"])                     # (the two trunks do round differently)
    plain = _run(dev, family, name, None, monkeypatch)
    assert [a for a, _ in plain["losses"]] == [a for a, _ in f32["losses"]]
    assert torch.equal(plain["flat"], f32["flat"])


def test_refusals(hip_lib, dev, monkeypatch):
    from pemp_amd import engine
    g = util.gold("canet_trainstep")
    with pytest.raises(ValueError, match="trunk_precision"):
        _build(dev, "canet", g, "bf16")
    monkeypatch.setattr(engine, "SPLIT3", False)                        # what PEMP_SPLIT3=0 sets
    for family, name in (("canet", "canet_trainstep"), ("pfenet", "pfenet_trainstep"), ("rpmms", "rpmms_trainstep")):
        with pytest.raises(ValueError, match="PEMP_SPLIT3"):
            _build(dev, family, util.gold(name), "split3")


def test_train_head_command_with_the_split3_trunk(hip_lib, dev, tmp_path):
    """``train_head ... trunk_precision=split3``: two epochs of 2 steps at 97 x 97 on synthetic episodes write a reference-loadable
    ckpt.pth whose trunk is the checkpoint's and whose head has moved."""
    from pemp_amd.entry import canet as e
    common = ["split=0", f"g.model_dir={tmp_path}", "data.height=97", "data.width=97", "data.test_n=6", "te.epochs=1", "data.test_bs=2"]

    def run(*argv):
        try:
            return e.ex.run_commandline(["prog", *argv])
        finally:
            for ing in e.INGREDIENTS[1:] + [e.net_ingredient, e.ex]:
                ing._updates.clear()
                ing._cfg = None

    run("train_head", "with", *common, "tr.total_epochs=2", "data.train_n=4", "data.bs=2", "tr.lr=0.0001", "ckpt=wgen", "trunk_precision=split3")
    d = tmp_path / "canet" / "1"
    assert sorted(p.name for p in d.iterdir()) == ["bestckpt.pth", "ckpt.pth"]
    sd = torch.load(str(d / "ckpt.pth"), map_location="cpu")
    assert [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()] == util.key_spec("canet")
    w0 = canet_ref.fixture_state_dict(True)
    assert not torch.equal(sd["layer7.weight"], w0["layer7.weight"]) and torch.equal(sd["encoder.conv1.weight"], w0["encoder.conv1.weight"])
    assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
