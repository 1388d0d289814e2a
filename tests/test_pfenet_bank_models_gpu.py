"""PFENet support banks through the model: ``segment(enroll(supports), queries)`` against ``forward`` on the same episodes, bit for
bit.  The engine's support side and query side make the launches ``lowres`` makes on the same rows, and the bank prior is bit for
bit ``ops.prior_mask`` (tests/test_pfenet_bank_ops_gpu.py), so supports enrolled apart from their queries give the same logits.
97 x 97 inputs (13 x 13 features), Wgen weights as in tests/test_pfenet_gpu.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import util

pytestmark = pytest.mark.gpu
WGEN_SEED = 1259
H = 97
HW = (H, H)
_NETS = {}


def _net(dev, shot):
    if shot not in _NETS:
        from pemp_amd.networks import pfenet as m
        net = m.PFENet(shot, None)
        net.load_state_dict(util.wgen_state_dict("pfenet", seed=WGEN_SEED))
        _NETS[shot] = net.to(dev).eval()
    return _NETS[shot]


def _batch(seeds, shot, dev):
    from pemp_amd import synth
    b = synth.make_batch([int(s) for s in seeds], shot=shot, height=H, width=H, out_hw=HW)
    return [torch.from_numpy(b[k]).to(dev) for k in ("sup_img", "sup_mask", "qry_img")]


def _ptrs(bank):
    return [t.data_ptr() for t in bank.tensors()]


@pytest.mark.parametrize("shot", [1, 5])
def test_segment_of_enrolled_supports_equals_forward(hip_lib, dev, exact_eval_variants, shot):
    from pemp_amd.bank import PFENetBank
    net = _net(dev, shot)
    B = 3
    sup, msk, qry = _batch((31, 32, 33), shot, dev)
    q = qry[:, 0].contiguous()
    with torch.no_grad():
        ref = net(sup, msk, qry, None, HW).clone()
        eng = net._engine_for(dev)["pfenet"]
        ref_low = net.lowres(sup, msk, qry)[0].clone()
        ref_svec, ref_prior = eng.last_supp_vec.clone(), eng.last_prior.clone()
        bank = net.enroll(sup, msk, labels=[7, 8, 9])
        assert isinstance(bank, PFENetBank) and len(bank) == B and bank.labels == [7, 8, 9]
        assert (bank.family, bank.S, bank.HW, bank.C) == ("pfenet", shot, 169, 2048) and bank.cap % 64 == 0
        assert bank.cap == -(-int(bank.count_host.max()) // 64) * 64 and torch.equal(bank.count.cpu(), bank.count_host)
        assert 1 <= int(bank.count_host.min()) and int(bank.count_host.max()) < 169          # real masks: a share of the map
        assert torch.equal(bank.svec, ref_svec)
        out = net.segment(bank, q, index=range(B), out_shape=HW)
        assert torch.equal(eng.last_bank_prior, ref_prior)
        assert out.shape == ref.shape and torch.equal(out, ref)
        low, none = net.segment_lowres(bank, q, index=list(range(B)))
        assert none is None and torch.equal(low, ref_low)
        # every query against every class: the [n, k] slice is the indexed result of the pair
        every = net.segment_lowres(bank, q)[0].clone()
        assert every.shape == (B, B, 2, 13, 13)
        for k in range(B):
            pk = net.segment_lowres(bank, q, index=[k] * B)[0]
            assert torch.equal(every[:, k], pk), k
        assert all(torch.equal(every[n, n], ref_low[n]) for n in range(B))
        assert not torch.equal(every[0, 0], every[0, 1])
        full = net.segment(bank, q, out_shape=HW)
        assert full.shape == (B, B, 2) + HW and torch.equal(full[1, 1], ref[1])
        with pytest.raises(ValueError, match="ret_ind"):
            net.segment(bank, q, ret_ind=True)
        with pytest.raises(ValueError, match="HW = 169"):
            net.segment(bank, torch.zeros((1, 3, 105, 105), device=dev))
        with pytest.raises(ValueError, match="square"):
            net.segment(bank, torch.zeros((1, 3, 97, 105), device=dev))


def test_graphed_segment_reads_the_bank_in_place(hip_lib, dev, exact_eval_variants):
    net = _net(dev, 1)
    sup, msk, qry = _batch((31, 32, 33, 34, 35, 36), 1, dev)
    q = qry[:3, 0].contiguous()
    index = [2, 0, 1]
    with torch.no_grad():
        cap = 192                                                   # HW = 169 rounded up: holds any class
        bank = net.enroll(sup[:3], msk[:3], labels=[1, 2, 3], capacity=cap)
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
        fresh = net.enroll(sup[3:], msk[3:], capacity=cap)
        assert net.enroll(sup[3:], msk[3:], labels=[4, 5, 6], out=bank) is bank
        assert _ptrs(bank) == ptrs and bank.labels == [4, 5, 6] and torch.equal(bank.count_host, fresh.count_host)
        assert torch.equal(bank.svec, fresh.svec) and torch.equal(bank.count, fresh.count)
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


def test_capacity_and_persistence(hip_lib, dev, exact_eval_variants):
    from pemp_amd.bank import PFENetBank
    net = _net(dev, 1)
    sup, msk, qry = _batch((31, 32), 1, dev)
    whole = msk.clone()
    whole[:, :, 0] = 1.0                                            # every pixel foreground: 169 rows per shot
    whole[:, :, 1] = 0.0
    with torch.no_grad():
        bank = net.enroll(sup, msk)
        assert bank.cap < 169
        for capacity in (64, 128):
            with pytest.raises(ValueError, match="needs 169 rows"):
                net.enroll(sup, whole, capacity=capacity)
        with pytest.raises(ValueError, match="multiple of 64"):
            net.enroll(sup, msk, capacity=100)
        before = [t.clone() for t in bank.tensors()]
        with pytest.raises(ValueError, match="needs 169 rows"):
            net.enroll(sup, whole, out=bank)
        assert all(torch.equal(a, b) for a, b in zip(before, bank.tensors()))          # refused before anything was written
        big = net.enroll(sup[:1], whole[:1])
        assert big.cap == 192 and int(big.count_host.max()) == 169
        with pytest.raises(ValueError, match="needs 169 rows"):
            bank.update(0, big)
        with pytest.raises(ValueError, match="classes"):
            net.enroll(sup[:1], msk[:1], out=bank)
        with pytest.raises(ValueError, match="shot"):
            net.enroll(torch.cat([sup, sup], 1), torch.cat([msk, msk], 1))
        # a bank travels: state_dict -> host -> a new bank on the device
        sd = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in bank.state_dict().items()}
        back = PFENetBank.from_state_dict(sd, device=dev)
        assert all(a.is_cuda and torch.equal(a, b) for a, b in zip(back.tensors(), bank.tensors()))
        assert torch.equal(back.count_host, bank.count_host) and back.labels == bank.labels and back.HW == bank.HW
        back.require_like(bank, "round trip")
        q = qry[:, 0].contiguous()
        assert torch.equal(net.segment_lowres(back, q, index=[0, 1])[0], net.segment_lowres(bank, q, index=[0, 1])[0])
        assert bank.to(dev) is bank and not bank.to("cpu").rows.is_cuda


def test_bank_evaluator_round_matches_per_query_segment_calls(hip_lib, dev):
    from pemp_amd.core.metrics import FewShotMetric
    from pemp_amd.entry import pfenet as entry
    from pemp_amd.entry.pemp_stage1 import BankEvaluator
    net = _net(dev, 1)
    data = entry.SyntheticEpisodes(6, 5678, 1, split=0, height=H, width=H)
    ev = BankEvaluator(net, device=dev)
    loss, miou, biou = ev.start_eval_loop(data, 20, 0, te_epochs=1)
    assert type(ev.bank).__name__ == "PFENetBank" and len(ev.bank) == 5 and ev.bank.cap == 192
    data.reset_sampler()
    data.sample_tasks()
    metric = FewShotMetric(20)
    losses, banks = [], {}
    with torch.no_grad():
        for i in range(len(data)):
            (sup, msk, qry), qry_msk, cls = data.task(i)
            c = int(cls[0])
            if c not in banks:                                      # the round's first task of the class enrolls it
                banks[c] = net.enroll(sup.to(dev), msk.to(dev), labels=[c])
            gt = qry_msk[0].to(dev)
            out = net.segment(banks[c], qry[:, 0].to(dev), index=[0], out_shape=tuple(gt.shape[-2:]))
            losses.append(F.cross_entropy(out, gt, ignore_index=255).item())
            metric.update(out.argmax(1).cpu().numpy(), qry_msk[0].numpy(), cls.tolist())
    labels = entry.get_val_labels(0)
    assert abs(float(np.mean(miou)) - metric.mIoU(labels)[1]) <= 1e-6
    assert abs(float(np.mean(biou)) - metric.mIoU(labels, binary=True)[1]) <= 1e-6
    assert abs(loss - float(np.mean(losses))) <= 1e-4
