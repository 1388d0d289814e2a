"""``segment_labels`` on the four bank kinds, the N-way evaluator and the ``test_nway`` command.  ``segment_labels`` must be the rule
(tests/test_nway_ops_gpu.py::rule) applied to what ``segment`` returns for the same bank and queries: the fused tail shares the
upsampling helper of ``segment``'s kernel, so every comparison is ``torch.equal``.  97 x 97 inputs (13 x 13 features), Wgen
weights and the exact conv variants, as in the tests of the banks themselves."""
import re

import pytest
import torch

from tests import util
from tests.test_nway_ops_gpu import rule

pytestmark = pytest.mark.gpu
WGEN_SEED = 1259
H = 97
HW = (H, H)
N_EPISODES, SEED = 12, 5678        # tests/test_bank_cpu.py holds that this round covers every validation class of split 0
KINDS = ["stage1_rn50", "baseline_vgg16", "pfenet", "rpmms"]
_CTX = {}


def _make(kind, dev):
    from pemp_amd import synth
    from pemp_amd.networks import baseline, pemp_stage1, pfenet, rpmms
    if kind == "stage1_rn50":
        net, sd = pemp_stage1.PEMPStage1(None), util.wgen_state_dict("stage1_rn50")
    elif kind == "baseline_vgg16":
        net, sd = baseline.Baseline(None, backbone="vgg16"), util.wgen_state_dict("baseline_vgg16")
    elif kind == "pfenet":
        net, sd = pfenet.PFENet(1, None), util.wgen_state_dict("pfenet", seed=WGEN_SEED)
    else:
        net = rpmms.RPMMs(None)
        sd = synth.wgen_state_dict_for(net, WGEN_SEED)
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    if kind == "rpmms":                                             # the EM's initial mu pinned, as in tests/test_rpmms_gpu.py
        g = util.gold("rpmms_small")
        net.set_pmm_init({k: torch.from_numpy(g[f"mu0_k{k}"]) for k in (1, 3, 6)})
    return net


@pytest.fixture
def ctx(hip_lib, dev, exact_eval_variants, request):
    """Per model kind, made once: the model, six episodes, a K = 3 bank of the first three supports, the three queries and what
    ``segment`` gives on them."""
    kind = request.param
    if kind not in _CTX:
        from pemp_amd import synth
        net = _make(kind, dev)
        b = synth.make_batch([31, 32, 33, 34, 35, 36], shot=1, height=H, width=H, out_hw=HW)
        sup, msk, qry = (torch.from_numpy(b[k]).to(dev) for k in ("sup_img", "sup_mask", "qry_img"))
        q = qry[:3, 0].contiguous()
        with torch.no_grad():
            bank = net.enroll(sup[:3], msk[:3], labels=[7, 8, 9])
            full = net.segment(bank, q).clone()                     # [3,3,2,97,97]
        _CTX[kind] = dict(kind=kind, net=net, sup=sup, msk=msk, qry=qry, q=q, bank=bank, full=full)
    return _CTX[kind]


@pytest.fixture(scope="module", autouse=True)
def _drop_models():
    yield
    _CTX.clear()


@pytest.mark.parametrize("ctx", KINDS, indirect=True)
def test_segment_labels_is_the_rule_on_segment(ctx, dev):
    net, bank, q, full = ctx["net"], ctx["bank"], ctx["q"], ctx["full"]
    assert full.shape == (3, 3, 2) + HW
    want_labels, want_margin, claims = rule(full)
    with torch.no_grad():
        labels = net.segment_labels(bank, q)
        both = net.segment_labels(bank, q, want_margin=True)
    assert labels.dtype == torch.uint8 and labels.shape == (3,) + HW         # out_shape: the query's size
    assert torch.equal(labels, want_labels), f"{(labels != want_labels).sum().item()} labels differ"
    assert isinstance(both, tuple) and torch.equal(both[0], want_labels) and torch.equal(both[1], want_margin)
    # a pixel is 0 iff all three binary maps of segment say background
    assert torch.equal(labels == 0, (full[:, :, 1] <= full[:, :, 0]).all(dim=1)) and torch.equal(labels == 0, ~claims.any(dim=1))
    assert 0 < int((labels > 0).sum()) < labels.numel()
    print(ctx["kind"], "pixels per label", torch.bincount(labels.flatten().long(), minlength=4).tolist(),
          "claimed by more than one class", int((claims.sum(dim=1) > 1).sum()))
    # another output size
    other = (80, 120)
    with torch.no_grad():
        lab2, mar2 = net.segment_labels(bank, q, out_shape=other, want_margin=True)
        ref2 = rule(net.segment(bank, q, out_shape=other))
    assert lab2.shape == (3,) + other and torch.equal(lab2, ref2[0]) and torch.equal(mar2, ref2[1])


@pytest.mark.parametrize("ctx", KINDS, indirect=True)
def test_graphed_equals_eager_and_reads_the_bank_in_place(ctx, dev):
    net, sup, msk, q = ctx["net"], ctx["sup"], ctx["msk"], ctx["q"]
    kw = dict(capacity=192) if ctx["kind"] == "pfenet" else {}       # PFENet: HW = 169 rounded up, a slot that holds any class
    with torch.no_grad():
        bank = net.enroll(sup[:3], msk[:3], **kw)
        g0 = net.segment_labels(bank, q, graphed=True)
        assert torch.equal(g0, rule(ctx["full"])[0])
        lab, mar = net.segment_labels(bank, q, graphed=True, want_margin=True)      # a replay
        assert torch.equal(lab, g0) and torch.equal(mar, rule(ctx["full"])[1])
        n_graphs = len(net._engine["graphs"])
        # other classes enrolled in place: the same graph sees them
        ptrs = [t.data_ptr() for t in bank.tensors()]
        assert net.enroll(sup[3:], msk[3:], out=bank) is bank and [t.data_ptr() for t in bank.tensors()] == ptrs
        g1 = net.segment_labels(bank, q, graphed=True)
        assert len(net._engine["graphs"]) == n_graphs
        fresh = net.enroll(sup[3:], msk[3:])
        assert torch.equal(g1, net.segment_labels(fresh, q)) and torch.equal(g1, net.segment_labels(bank, q))
        assert torch.equal(g1, rule(net.segment(fresh, q))[0]) and not torch.equal(g1, g0)


@pytest.mark.parametrize("ctx", KINDS, indirect=True)
def test_one_class_bank_gives_the_episodes_own_prediction(ctx, dev):
    """K = 1: the label map is the arg-max the episode path's prediction has for that episode (the reference's ``get_pred``)."""
    net, kind = ctx["net"], ctx["kind"]
    sup, msk, qry = ctx["sup"][1:2], ctx["msk"][1:2], ctx["qry"][1:2]
    with torch.no_grad():
        if kind == "rpmms":
            am = net.get_pred(net(sup, msk, qry), qry[:, 0])[1]
        elif kind == "pfenet":
            am = net(sup, msk, qry, None, HW).argmax(dim=1)
        else:
            am = net(sup, msk, qry, HW).argmax(dim=1)
        one = net.enroll(sup, msk)
        labels = net.segment_labels(one, qry[:, 0].contiguous())
    assert len(one) == 1 and torch.equal(labels, am.to(torch.uint8)) and 0 < int(labels.sum()) < labels.numel()
    # which is the binary map of that (query, class) pair in the K = 3 call
    assert torch.equal(labels[0] == 1, ctx["full"][1, 1, 1] > ctx["full"][1, 1, 0])


def _recording(monkeypatch, e):
    rows = []
    add = e.DeviceRoundTable.add

    def rec_add(self, stats, classes):
        rows.append(stats.cpu().clone())
        return add(self, stats, classes)
    monkeypatch.setattr(e.DeviceRoundTable, "add", rec_add)
    return rows


@pytest.mark.parametrize("ctx", ["stage1_rn50"], indirect=True)
def test_nway_evaluator_round_matches_per_query_calls(ctx, dev, monkeypatch):
    from pemp_amd import ops
    from pemp_amd.entry import pemp_stage1 as e
    net = ctx["net"]
    labels = [int(c) for c in e.get_val_labels(0)]
    make = lambda n=N_EPISODES: e.SyntheticEpisodes(n, SEED, 1, split=0, height=H, width=H)
    data = make()
    data.sample_tasks()
    tasks = [data.task(i) for i in range(N_EPISODES)]
    assert {int(t[2]) for t in tasks} == set(labels)                                   # every validation class occurs
    with torch.no_grad():
        bank, seen = None, set()
        for (sup, msk, _), _, cls in tasks:                         # the round's first task of a class enrolls it
            if int(cls[0]) not in seen:
                seen.add(int(cls[0]))
                one = net.enroll(sup.to(dev), msk.to(dev), labels=[int(cls[0])])
                bank = bank if bank is not None else type(one).empty_like(one, len(labels), labels=list(labels))
                bank.update(labels.index(int(cls[0])), one)
        want = []
        for (_, _, qry), qry_msk, cls in tasks:
            low = net.segment_lowres(bank, qry[:, 0].to(dev))[0]
            want.append(ops.nway_tail(low, target=qry_msk.view(-1, *qry_msk.shape[-2:]).to(dev), want=[labels.index(int(cls[0]))])[2].cpu())
    want = torch.cat(want)
    rows = _recording(monkeypatch, e)
    losses = []
    for kw, batch in ((dict(), 1), (dict(), 4), (dict(use_graph=False), 5)):
        rows.clear()
        ev = e.NWayEvaluator(net, device=dev, **kw)
        loss, miou, biou = ev.start_eval_loop(make(), 20, 0, te_epochs=1, batch=batch)
        assert len(rows) == 1 and torch.equal(rows[0], want), (kw, batch)
        assert len(ev.bank) == len(labels) and ev.bank.labels == labels and torch.equal(ev.bank.protos, bank.protos)
        losses.append(loss)
    # the loss is the class's own binary CE: the enroll-once evaluator's, exactly; the counts are under competition
    rows.clear()
    loss_b, miou_b, biou_b = e.BankEvaluator(net, device=dev).start_eval_loop(make(), 20, 0, te_epochs=1, batch=4)
    assert all(l == loss_b for l in losses), (losses, loss_b)
    assert torch.equal(rows[0][:, :2], want[:, :2])
    assert (want[:, 5] + want[:, 6] <= rows[0][:, 5] + rows[0][:, 6]).all()            # a class can only lose pixels to the others
    print("foreground pixels per query, alone", (rows[0][:, 5] + rows[0][:, 6]).tolist(), "under competition", (want[:, 5] + want[:, 6]).tolist())
    assert want[:, 5].sum().item() > 0                              # some foreground survives the competition
    # a round that misses a class is refused
    with pytest.raises(ValueError, match="validation classes"):
        e.NWayEvaluator(net, device=dev).start_eval_loop(make(3), 20, 0, te_epochs=1, batch=1)


@pytest.mark.parametrize("name", ["pemp_stage1", "rpmms"])
def test_test_nway_command_end_to_end(hip_lib, dev, exact_eval_variants, name):
    import importlib
    entry = importlib.import_module(f"pemp_amd.entry.{name}")

    def run(*argv):
        try:
            return entry.ex.run_commandline(["prog", *argv])
        finally:
            for ing in entry.ex.ingredients + [entry.ex]:
                ing._updates.clear()
                ing._cfg = None

    small = ["split=0", "ckpt=wgen", "data.height=97", "data.width=97", f"data.test_n={N_EPISODES}", f"data.test_seed={SEED}",
             "te.epochs=1"]
    line = re.compile(r"^(Loss|Loss_p1): (\d+\.\d{4}), mIoU: (\d+\.\d{2}), bIoU: (\d+\.\d{2})$")
    out = line.match(run("test_nway", "with", *small, "data.test_bs=4"))
    assert out and out.group(1) == ("Loss_p1" if name == "rpmms" else "Loss")
    assert 0.0 <= float(out.group(3)) <= 100.0 and 0.0 <= float(out.group(4)) <= 100.0
    bank = line.match(run("test_bank", "with", *small, "data.test_bs=4"))
    assert bank and out.group(2) == bank.group(2)                   # the loss is test_bank's
