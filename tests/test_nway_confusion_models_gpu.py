"""``segment_confusion`` on a prototype-matching and a query-conditioned bank family, and one ``SemanticEvaluator`` round.  The model
call must be ``ops.nway_confusion`` on what ``segment_lowres`` gives for the same bank and queries; the tables are integers, so
every comparison is ``torch.equal``.  97 x 97 inputs, Wgen weights and the exact conv variants, as in tests/test_nway_models_gpu.py."""
import re

import numpy as np
import pytest
import torch

from tests.test_nway_models_gpu import H, HW, N_EPISODES, SEED, _make

pytestmark = pytest.mark.gpu
KINDS = ["stage1_rn50", "rpmms"]
_CTX = {}


@pytest.fixture
def ctx(hip_lib, dev, exact_eval_variants, request):
    """Per model kind, made once: the model, a K = 3 bank, three queries, their low-resolution logits, a slot-label target with
    some 255, binary masks, and ragged copies of both."""
    kind = request.param
    if kind not in _CTX:
        from pemp_amd import synth
        net = _make(kind, dev)
        b = synth.make_batch([31, 32, 33], shot=1, height=H, width=H, out_hw=HW)
        sup, msk, qry = (torch.from_numpy(b[k]).to(dev) for k in ("sup_img", "sup_mask", "qry_img"))
        q = qry[:, 0].contiguous()
        g = torch.Generator().manual_seed(41)
        target = torch.randint(0, 4, (3,) + HW, generator=g)
        target[torch.rand((3,) + HW, generator=g) < 0.1] = 255
        binary = torch.from_numpy(b["qry_mask"]).view(3, *HW).long()
        sizes = [(80, 120), HW, (33, 47)]
        ragged = [torch.randint(0, 4, s, generator=g) for s in sizes]
        ragged[0][:9] = 255
        with torch.no_grad():
            bank = net.enroll(sup, msk, labels=[7, 8, 9])
            low = net.segment_lowres(bank, q)[0].clone()
        _CTX[kind] = dict(kind=kind, net=net, q=q, bank=bank, low=low, target=target.to(dev), binary=binary.to(dev), ragged=ragged)
    return _CTX[kind]


@pytest.fixture(scope="module", autouse=True)
def _drop_models():
    yield
    _CTX.clear()


@pytest.mark.parametrize("ctx", KINDS, indirect=True)
def test_segment_confusion_is_the_op_on_segment_lowres(ctx, dev):
    from pemp_amd import ops
    net, bank, q, low = ctx["net"], ctx["bank"], ctx["q"], ctx["low"]
    assert low.shape[:3] == (3, 3, 2)
    want_conf, want_labels = ops.nway_confusion(low, ctx["target"], want_labels=True)
    assert int(want_conf.sum()) == int((ctx["target"] != 255).sum()) and 0 < int((want_labels > 0).sum()) < want_labels.numel()
    rag_conf, rag_labels = ops.nway_confusion_ragged(low, ctx["ragged"], want_labels=True)
    bin_conf = ops.nway_confusion(low, ctx["binary"], want=[2, 0, 1])[0]
    print(ctx["kind"], "table of query 0", want_conf[0].tolist())
    with torch.no_grad():
        for graphed in (False, True, True):                         # eager, capture, replay
            conf, none = net.segment_confusion(bank, q, ctx["target"], graphed=graphed)
            assert none is None and conf.dtype == torch.int64 and torch.equal(conf, want_conf), graphed
            conf, labels = net.segment_confusion(bank, q, ctx["target"], graphed=graphed, want_labels=True)
            assert torch.equal(conf, want_conf) and torch.equal(labels, want_labels)
            assert torch.equal(labels, net.segment_labels(bank, q, graphed=graphed))
            # a ragged list, labels on the host
            conf, none = net.segment_confusion(bank, q, ctx["ragged"], graphed=graphed)
            assert none is None and torch.equal(conf, rag_conf)
            conf, labels = net.segment_confusion(bank, q, [t.to(dev) for t in ctx["ragged"]], graphed=graphed, want_labels=True)
            assert torch.equal(conf, rag_conf) and all(torch.equal(a, b) for a, b in zip(labels, rag_labels))
            # the evaluators' form: binary masks with the queries' own slots; a host target is uploaded
            for want in ([2, 0, 1], torch.tensor([2, 0, 1], dtype=torch.int32, device=dev)):
                assert torch.equal(net.segment_confusion(bank, q, ctx["binary"].cpu(), want=want, graphed=graphed)[0], bin_conf)
    # real multi-class ground truth in dataset ids goes through slot_targets
    ids = torch.tensor([0, 7, 8, 9, 255, 3])[torch.randint(0, 6, (3,) + HW, generator=torch.Generator().manual_seed(5))]
    slots = ops.slot_targets(ids.to(dev), bank.labels)
    assert set(slots.unique().tolist()) == {0, 1, 2, 3, 255}
    with torch.no_grad():
        assert torch.equal(net.segment_confusion(bank, q, slots)[0], ops.nway_confusion(low, slots)[0])


@pytest.mark.parametrize("ctx", ["stage1_rn50"], indirect=True)
def test_semantic_evaluator_round_is_the_sum_of_per_episode_tables(ctx, dev):
    from pemp_amd.core.metrics import SemanticMetric
    from pemp_amd.entry import pemp_stage1 as e
    net = ctx["net"]
    labels = [int(c) for c in e.get_val_labels(0)]
    make = lambda n=N_EPISODES: e.SyntheticEpisodes(n, SEED, 1, split=0, height=H, width=H)
    data = make()
    data.sample_tasks()
    tasks = [data.task(i) for i in range(N_EPISODES)]
    with torch.no_grad():
        bank, seen = None, set()
        for (sup, msk, _), _, cls in tasks:                         # the round's first task of a class enrolls it
            if int(cls[0]) not in seen:
                seen.add(int(cls[0]))
                one = net.enroll(sup.to(dev), msk.to(dev), labels=[int(cls[0])])
                bank = bank if bank is not None else type(one).empty_like(one, len(labels), labels=list(labels))
                bank.update(labels.index(int(cls[0])), one)
        total = torch.zeros(len(labels) + 1, len(labels) + 1, dtype=torch.int64)
        for (_, _, qry), qry_msk, cls in tasks:
            conf, _ = net.segment_confusion(bank, qry[:, 0].to(dev), qry_msk.view(-1, *qry_msk.shape[-2:]).to(dev),
                                            want=[labels.index(int(cls[0]))])
            total += conf[0].cpu()
    assert int(total.sum()) > 0 and int(total[1:].sum()) > 0
    metric = SemanticMetric(len(labels))
    metric.update(total)
    want = metric.result()
    for kw, batch in ((dict(), 1), (dict(), 5), (dict(use_graph=False), 12)):
        ev = e.SemanticEvaluator(net, device=dev, **kw)
        got = ev.start_eval_loop(make(), 20, 0, te_epochs=1, batch=batch)
        assert len(ev.round_tables) == 1 and np.array_equal(ev.round_tables[0], total.numpy()), (kw, batch)
        assert got == (want["mIoU"], want["mIoU_bg"], want["pixAcc"])
        assert np.array_equal(ev.round_iou[0], want["iou"], equal_nan=True)
    print("round table", total.tolist(), "result", got)
    assert all(0.0 <= v <= 1.0 for v in got)
    # a round that misses a class is refused, as in test_nway
    with pytest.raises(ValueError, match="validation classes"):
        e.SemanticEvaluator(net, device=dev).start_eval_loop(make(3), 20, 0, te_epochs=1, batch=1)


def test_test_semantic_command_end_to_end(hip_lib, dev, exact_eval_variants):
    from pemp_amd.entry import pemp_stage1 as entry

    def run(*argv):
        try:
            return entry.ex.run_commandline(["prog", *argv])
        finally:
            for ing in entry.ex.ingredients + [entry.ex]:
                ing._updates.clear()
                ing._cfg = None

    small = ["split=0", "ckpt=wgen", "data.height=97", "data.width=97", f"data.test_n={N_EPISODES}", f"data.test_seed={SEED}",
             "te.epochs=1", "data.test_bs=4"]
    out = re.match(r"^mIoU_sem: (\d+\.\d{2}), mIoU_sem\+bg: (\d+\.\d{2}), pixAcc: (\d+\.\d{2})$", run("test_semantic", "with", *small))
    assert out and all(0.0 <= float(v) <= 100.0 for v in out.groups())
