"""RPMMs support banks through the model: ``segment(enroll(supports), queries)`` against ``forward`` / ``lowres`` on the same
episodes, bit for bit.  The engine's support side and query side make the launches ``lowres`` makes on the same rows, and the bank
kernel is bit for bit the two episode kernels (tests/test_rpmms_bank_ops_gpu.py), so supports enrolled apart from their queries
give the same logits in all three passes.  Every comparison is ``torch.equal``.  97 x 97 inputs (13 x 13 features), Wgen weights
and the ``rpmms_small`` fixture's initial mu pinned, as in tests/test_rpmms_gpu.py."""
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu
WGEN_SEED = 1259
H = 97
HW = (H, H)
N_EPISODES, SEED = 12, 5678        # tests/test_bank_cpu.py holds that this round covers every validation class of split 0
_NETS = {}


def _net(dev, pinned=True):
    if pinned not in _NETS:
        from pemp_amd import synth
        from pemp_amd.networks import rpmms as m
        net = m.RPMMs(None)
        net.load_state_dict(synth.wgen_state_dict_for(net, WGEN_SEED))
        net = net.to(dev).eval()
        if pinned:
            g = util.gold("rpmms_small")
            net.set_pmm_init({k: torch.from_numpy(g[f"mu0_k{k}"]) for k in (1, 3, 6)})
        _NETS[pinned] = net
    return _NETS[pinned]


def _batch(seeds, dev, height=H):
    from pemp_amd import synth
    b = synth.make_batch([int(s) for s in seeds], shot=1, height=height, width=H, out_hw=(height, H))
    return [torch.from_numpy(b[k]).to(dev) for k in ("sup_img", "sup_mask", "qry_img")]


def _ptrs(bank):
    return [t.data_ptr() for t in bank.tensors()]


@pytest.fixture(scope="module")
def episodes(hip_lib, dev):
    """B = 3 episodes and what the episode path gives on them with the exact conv variants, computed once."""
    from pemp_amd import ops
    net = _net(dev)
    sup, msk, qry = _batch((31, 32, 33), dev)
    saved, ops.EVAL_SPLITK = ops.EVAL_SPLITK, False
    try:
        with torch.no_grad():
            fwd = [o.clone() for o in net(sup, msk, qry)]
            low = net.lowres(sup, msk, qry)[0].clone()
            mu = net._engine_for(dev)["rpmms"].last_mu.clone()
    finally:
        ops.EVAL_SPLITK = saved
    return dict(sup=sup, msk=msk, qry=qry, q=qry[:, 0].contiguous(), fwd=fwd, low=low, mu=mu)


def test_segment_of_enrolled_supports_equals_the_episode_path(hip_lib, dev, exact_eval_variants, episodes):
    from pemp_amd import ops
    from pemp_amd.bank import RPMMsBank
    net, B = _net(dev), 3
    sup, msk, q = episodes["sup"], episodes["msk"], episodes["q"]
    _, out0, out1, out2 = episodes["fwd"]
    eng = net._engine_for(dev)["rpmms"]
    with torch.no_grad():
        bank = net.enroll(sup, msk, labels=[7, 8, 9])
        assert isinstance(bank, RPMMsBank) and len(bank) == B and bank.labels == [7, 8, 9] and bank.nbytes() == 112640
        assert (bank.family, bank.backbone, bank.precision, bank.C) == ("rpmms", "resnet50", "f32", 256)
        assert torch.equal(bank.mu, episodes["mu"])
        assert torch.equal(bank.taps, ops.rpmms_proto_taps(eng.wz, bank.mu))
        low, none = net.segment_lowres(bank, q, index=range(B))
        assert none is None and low.shape == (B, 2, 13, 13) and torch.equal(low, episodes["low"]) and torch.equal(low, out2)
        for got, want in zip(eng.last_bank_passes, (out0, out1, out2)):
            assert torch.equal(got, want)
        assert (eng.last_bank_l56_in[..., 258:] == 0).all()
        # every query against every class: the [n, k] slice is the indexed result of the pair
        every = net.segment_lowres(bank, q)[0].clone()
        assert every.shape == (B, B, 2, 13, 13)
        passes = [p.clone().view(B, B, 2, 13, 13) for p in eng.last_bank_passes]
        for k in range(B):
            pk = net.segment_lowres(bank, q, index=[k] * B)[0]
            assert torch.equal(every[:, k], pk), k
        for n in range(B):
            assert torch.equal(every[n, n], episodes["low"][n])
            for got, want in zip(passes, (out0, out1, out2)):
                assert torch.equal(got[n, n], want[n])
        assert not torch.equal(every[0, 0], every[0, 1])
        # segment: the upsampled final logits, as get_pred makes them before its softmax
        up = ops.upsample_bilinear_ac(out2.contiguous(), HW)
        out = net.segment(bank, q, index=list(range(B)), out_shape=HW)
        assert out.shape == (B, 2) + HW and torch.equal(out, up)
        soft, _ = net.get_pred(episodes["fwd"], episodes["qry"][:, 0])
        assert torch.equal(torch.softmax(net.segment(bank, q, index=[0, 1, 2]), dim=1), soft)      # out_shape: the query's size
        full = net.segment(bank, q, out_shape=HW)
        assert full.shape == (B, B, 2) + HW and torch.equal(full[1, 1], up[1])
        with pytest.raises(ValueError, match="ret_ind"):
            net.segment(bank, q, ret_ind=True)
        with pytest.raises(ValueError, match="1-shot"):
            net.enroll(torch.cat([sup, sup], 1), torch.cat([msk, msk], 1))
        with pytest.raises(ValueError, match="classes"):
            net.enroll(sup[:1], msk[:1], out=bank)
        # a bank travels: state_dict -> host -> a new bank on the device
        sd = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in bank.state_dict().items()}
        back = RPMMsBank.from_state_dict(sd, device=dev)
        assert all(a.is_cuda and torch.equal(a, b) for a, b in zip(back.tensors(), bank.tensors())) and back.labels == bank.labels
        assert torch.equal(net.segment_lowres(back, q, index=[2, 0, 1])[0], every[[0, 1, 2], [2, 0, 1]])
        assert bank.to(dev) is bank and not bank.to("cpu").mu.is_cuda


def test_the_golden_fixture_through_the_bank(hip_lib, dev, exact_eval_variants):
    """``rpmms_small``: tests/test_rpmms_gpu.py holds the episode path to the reference's outputs on these inputs; the bank path is
    that path, bit for bit."""
    g = util.gold("rpmms_small")
    assert int(g["H"]) == H
    net = _net(dev)
    sup, msk, qry = _batch(g["seeds"], dev)
    B = sup.shape[0]
    with torch.no_grad():
        _, out0, out1, out2 = [o.clone() for o in net(sup, msk, qry)]
        bank = net.enroll(sup, msk)
        low = net.segment_lowres(bank, qry[:, 0].contiguous(), index=range(B))[0]
        assert torch.equal(low, out2)
        for got, want in zip(net._engine_for(dev)["rpmms"].last_bank_passes, (out0, out1, out2)):
            assert torch.equal(got, want)


def test_graphed_segment_reads_the_bank_in_place(hip_lib, dev, exact_eval_variants):
    net = _net(dev)
    sup, msk, qry = _batch((31, 32, 33, 34, 35, 36), dev)
    q = qry[:3, 0].contiguous()
    index = [2, 0, 1]
    with torch.no_grad():
        bank = net.enroll(sup[:3], msk[:3], labels=[1, 2, 3])
        eager = net.segment_lowres(bank, q, index=index)[0].clone()
        g0 = net.segment_graphed(bank, q, index=index)[0].clone()
        g1 = net.segment_graphed(bank, q, index=index)[0].clone()      # a replay
        assert torch.equal(g0, eager) and torch.equal(g1, eager)
        n_graphs = len(net._engine["graphs"])
        # another index through the same graph (the static int32 buffer)
        e2 = net.segment_lowres(bank, q, index=[1, 1, 0])[0].clone()
        g2 = net.segment_graphed(bank, q, index=[1, 1, 0])[0].clone()
        assert torch.equal(e2, g2) and not torch.equal(g2, eager)
        # other classes enrolled in place: the same graph sees them, no storage moved
        ptrs = _ptrs(bank)
        fresh = net.enroll(sup[3:], msk[3:])
        assert net.enroll(sup[3:], msk[3:], labels=[4, 5, 6], out=bank) is bank
        assert _ptrs(bank) == ptrs and bank.labels == [4, 5, 6]
        assert torch.equal(bank.mu, fresh.mu) and torch.equal(bank.taps, fresh.taps)
        e3 = net.segment_lowres(fresh, q, index=index)[0].clone()
        g3 = net.segment_graphed(bank, q, index=index)[0].clone()
        assert torch.equal(e3, g3) and not torch.equal(g3, eager)
        # one class back through update(): in place as well
        one = net.enroll(sup[:1], msk[:1])
        assert bank.update(1, one) is bank and _ptrs(bank) == ptrs
        g4 = net.segment_graphed(bank, q, index=index)[0].clone()
        alone = net.segment_lowres(one, q[2:3].contiguous(), index=[0])[0][0]            # query 2 meets class 1
        assert torch.equal(g4[2], alone) and not torch.equal(g4[2], g3[2]) and torch.equal(g4[:2], g3[:2])
        assert len(net._engine["graphs"]) == n_graphs
        # the all-classes form has a graph of its own
        ga = net.segment_graphed(bank, q)[0].clone()
        assert torch.equal(ga, net.segment_lowres(bank, q)[0]) and len(net._engine["graphs"]) == n_graphs + 1
        assert torch.equal(net.segment_graphed(bank, q)[0], ga)


def test_enrolment_reads_the_initial_mu_as_it_stands(hip_lib, dev):
    sup, msk, _ = _batch((31, 32), dev)
    with torch.no_grad():
        free = _net(dev, pinned=False)
        assert not free.pmm_init_pinned
        a = free.enroll(sup, msk)
        mu0 = free.pmm_mu0.clone()
        b = free.enroll(sup, msk)                                   # enroll draws nothing
        assert torch.equal(free.pmm_mu0, mu0) and torch.equal(a.mu, b.mu) and torch.equal(a.taps, b.taps)
        free.step_pmm_init()                                        # the caller's fresh draw
        c = free.enroll(sup, msk)
        assert not torch.equal(free.pmm_mu0, mu0) and not torch.equal(a.mu, c.mu)
        pinned = _net(dev)
        d = pinned.enroll(sup, msk)
        pinned.step_pmm_init()                                      # a pinned init stays
        e = pinned.enroll(sup, msk)
        assert all(torch.equal(x, y) for x, y in zip(d.tensors(), e.tensors()))


def test_a_bank_meets_queries_of_another_size(hip_lib, dev):
    net = _net(dev)
    sup, msk, _ = _batch((31, 32, 33), dev)
    _, _, qry = _batch((41, 42), dev, height=105)
    q = qry[:, 0].contiguous()
    assert tuple(q.shape) == (2, 3, 105, 97)
    with torch.no_grad():
        bank = net.enroll(sup, msk)
        low = net.segment_lowres(bank, q, index=[2, 0])[0]
        assert tuple(low.shape) == (2, 2, 14, 13) and torch.isfinite(low).all()
        every = net.segment_lowres(bank, q)[0]
        assert tuple(every.shape) == (2, 3, 2, 14, 13) and torch.isfinite(every).all()
        assert torch.equal(every[0, 2], low[0]) and torch.equal(every[1, 0], low[1])


def _recording(monkeypatch, e):
    rows = []
    add = e.DeviceRoundTable.add

    def rec_add(self, stats, classes):
        rows.append(stats.cpu().clone())
        return add(self, stats, classes)
    monkeypatch.setattr(e.DeviceRoundTable, "add", rec_add)
    return rows


def test_bank_evaluator_round_matches_per_query_segment_calls(hip_lib, dev, exact_eval_variants, monkeypatch):
    from pemp_amd import ops
    from pemp_amd.entry import pemp_stage1 as e1
    from pemp_amd.entry import rpmms as entry
    net = _net(dev)
    labels = entry.get_val_labels(0)
    data = entry.SyntheticEpisodes(N_EPISODES, SEED, 1, split=0, height=H, width=H)
    data.sample_tasks()
    assert {int(data.task(i)[2]) for i in range(N_EPISODES)} == set(labels)            # every validation class occurs
    want, banks = [], {}
    with torch.no_grad():
        for i in range(len(data)):
            (sup, msk, qry), qry_msk, cls = data.task(i)
            c = int(cls[0])
            if c not in banks:                                      # the round's first task of the class enrolls it
                banks[c] = net.enroll(sup.to(dev), msk.to(dev), labels=[c])
            low = net.segment_lowres(banks[c], qry[:, 0].to(dev), index=[0])[0]
            want.append(ops.eval_tail(low, qry_msk.view(-1, *qry_msk.shape[-2:]).to(dev))[1].cpu())
    want = torch.cat(want)
    rows = _recording(monkeypatch, e1)
    for batch in (1, 4):
        rows.clear()
        ev = entry.BankEvaluator(net, device=dev)
        loss, miou, biou = ev.start_eval_loop(entry.SyntheticEpisodes(N_EPISODES, SEED, 1, split=0, height=H, width=H), 20, 0,
                                              te_epochs=1, batch=batch)
        assert len(rows) == 1 and torch.equal(rows[0], want), batch
        assert type(ev.bank).__name__ == "RPMMsBank" and len(ev.bank) == len(labels) and ev.bank.labels == [int(c) for c in labels]
        for c, one in banks.items():
            assert torch.equal(ev.bank.mu[labels.index(c)], one.mu[0])
    assert want[:, 5].sum().item() > 0                              # some foreground is found


def test_test_bank_command_end_to_end(hip_lib, dev, exact_eval_variants):
    from pemp_amd.entry import rpmms as entry

    def run(*argv):
        try:
            return entry.ex.run_commandline(["prog", *argv])
        finally:
            for ing in entry.ex.ingredients + [entry.ex]:
                ing._updates.clear()
                ing._cfg = None

    small = ["split=0", "ckpt=wgen", "data.height=97", "data.width=97", "data.test_n=12", "te.epochs=1"]
    out = run("test_bank", "with", *small, "data.test_bs=1")
    assert out.startswith("Loss_p1: ") and "mIoU:" in out and "bIoU:" in out
    assert run("test_bank", "with", *small, "data.test_bs=4") == out                   # queries per step do not matter
