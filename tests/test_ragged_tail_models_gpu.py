"""The ragged tails where they are used: the batched steps of the evaluators (stage 1, the enroll-once bank evaluator, the N-way
evaluator, CANet's history step) against single-episode steps, and ``segment_labels`` with one output shape per query against
single-query calls.  Every comparison is ``torch.equal``.  97 x 97 inputs, Wgen weights and the exact conv variants, as in
tests/test_eval_protocol_gpu.py."""
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu
H = 97
N_EP = 7
_CTX = {}


@pytest.fixture
def ctx(hip_lib, dev, exact_eval_variants):
    """Made once: the stage-1 model, seven synthetic episodes whose query labels keep their own sizes, a bank of three classes."""
    if not _CTX:
        from pemp_amd import synth
        from pemp_amd.entry import pemp_stage1 as e
        net = e.ModelClass(None)
        net.load_state_dict(util.wgen_state_dict("stage1_rn50"))
        net = net.to(dev).eval()
        data = e.SyntheticEpisodes(N_EP, 5678, 1, split=0, height=H, width=H)
        data.sample_tasks()
        eps = [data.task(i)[:2] for i in range(N_EP)]
        b = synth.make_batch([31, 32, 33], shot=1, height=H, width=H, out_hw=(H, H))
        with torch.no_grad():
            bank = net.enroll(torch.from_numpy(b["sup_img"]).to(dev), torch.from_numpy(b["sup_mask"]).to(dev), labels=[7, 8, 9])
        _CTX.update(net=net, eps=eps, bank=bank, slots=[i % 3 for i in range(N_EP)])
    sizes = [tuple(m.shape[-2:]) for _, m in _CTX["eps"]]
    assert len(set(sizes)) >= 4 and len(set(sizes)) < N_EP, sizes            # distinct sizes, and one of them twice
    return _CTX


@pytest.fixture(scope="module", autouse=True)
def _drop():
    yield
    _CTX.clear()


def _counting(monkeypatch, ops, names):
    """Counters in front of the named ops, for the duration of the test."""
    calls = {n: 0 for n in names}
    for name in names:
        def wrap(*a, _f=getattr(ops, name), _n=name, **kw):
            calls[_n] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(ops, name, wrap)
    return calls


def _both_ways(monkeypatch, step, n_sizes, old, new):
    """``step()`` with the ragged tail, then with it withheld (``PEMP_RAGGED_TAIL=0``: ``ops.RAGGED_TAIL`` off) -> the rows of
    the first; the fixed-size op ``old`` is not called once in the first and once per distinct size in the second."""
    from pemp_amd import ops
    with monkeypatch.context() as mp:
        calls = _counting(mp, ops, [old, new])
        assert ops.RAGGED_TAIL                                  # the default
        rows = step().cpu()
        assert calls == {old: 0, new: 1}, calls
        mp.setattr(ops, "RAGGED_TAIL", False)
        loop = step().cpu()
        assert calls == {old: n_sizes, new: 1}, calls
    assert torch.equal(rows, loop)
    return rows


def test_stage1_batched_step_is_one_ragged_launch_and_equals_single_steps(ctx, dev, monkeypatch):
    from pemp_amd.entry import pemp_stage1 as e
    net, eps = ctx["net"], ctx["eps"]
    alone = torch.cat([e.Evaluator(net, device=dev).test_step_device(*ep)[1] for ep in eps]).cpu()
    ev = e.Evaluator(net, device=dev)
    n_sizes = len({tuple(m.shape[-2:]) for _, m in eps})
    rows = _both_ways(monkeypatch, lambda: ev.test_step_batch(eps), n_sizes, "eval_tail", "eval_tail_ragged")
    assert rows.shape == (N_EP, 8) and torch.equal(rows, alone), (rows.tolist(), alone.tolist())
    assert (rows[:, 1] > 0).all() and list(ev._ws).count(("tail_ragged", N_EP)) == 1
    # labels that are already on the device take the other packing path
    on_dev = [(inp, m.to(dev)) for inp, m in eps]
    assert torch.equal(ev.test_step_batch(on_dev).cpu(), alone)


def test_bank_and_nway_batched_steps_equal_single_queries(ctx, dev, monkeypatch):
    from pemp_amd import ops
    from pemp_amd.entry import pemp_stage1 as e
    net, bank, slots = ctx["net"], ctx["bank"], ctx["slots"]
    eps = [((inp[2], slots[i]), m) for i, (inp, m) in enumerate(ctx["eps"])]
    n_sizes = len({tuple(m.shape[-2:]) for _, m in eps})
    want_bank, want_nway = [], []
    with torch.no_grad():
        for (qry, slot), m in eps:
            tgt = m.view(-1, *m.shape[-2:]).to(dev)
            low = net.segment_lowres(bank, qry[:, 0].to(dev), index=[slot])[0]
            want_bank.append(ops.eval_tail(low, tgt)[1].cpu())
            every = net.segment_lowres(bank, qry[:, 0].to(dev))[0]
            want_nway.append(ops.nway_tail(every, target=tgt, want=[slot])[2].cpu())
    ev = e.BankEvaluator(net, device=dev)                        # replayed from a graph
    ev.bank = bank
    rows = _both_ways(monkeypatch, lambda: ev.test_step_batch(eps), n_sizes, "eval_tail", "eval_tail_ragged")
    assert torch.equal(rows, torch.cat(want_bank))
    assert torch.equal(rows, torch.cat([ev.test_step_device(*ep)[1] for ep in eps]).cpu())
    nw = e.NWayEvaluator(net, device=dev, use_graph=False)
    nw.bank = bank
    rows = _both_ways(monkeypatch, lambda: nw.test_step_batch(eps), n_sizes, "nway_tail", "nway_tail_ragged")
    assert torch.equal(rows, torch.cat(want_nway))
    assert torch.equal(rows, torch.cat([nw.test_step_device(*ep)[1] for ep in eps]).cpu())
    # the loss columns are the class's own binary CE on both paths; the counts differ under competition
    assert torch.equal(torch.cat(want_bank)[:, :2], torch.cat(want_nway)[:, :2])


def test_segment_labels_with_one_shape_per_query(ctx, dev):
    net, bank = ctx["net"], ctx["bank"]
    q = torch.cat([ctx["eps"][i][0][2][:, 0] for i in range(4)]).to(dev)            # four queries [4,3,97,97]
    shapes = [(80, 120), (97, 97), (80, 120), (50, 61)]
    with torch.no_grad():
        single = [net.segment_labels(bank, q[i:i + 1], out_shape=shapes[i], want_margin=True) for i in range(4)]
        for graphed in (False, True):
            maps = net.segment_labels(bank, q, out_shape=shapes, graphed=graphed)
            pairs = net.segment_labels(bank, q, out_shape=[list(s) for s in shapes], want_margin=True, graphed=graphed)
            assert isinstance(maps, list) and len(maps) == 4 and len(pairs) == 4
            for i in range(4):
                assert maps[i].dtype == torch.uint8 and tuple(maps[i].shape) == shapes[i]
                assert torch.equal(maps[i], single[i][0][0]), (graphed, i)
                lab, mar = pairs[i]
                assert torch.equal(lab, single[i][0][0]) and torch.equal(mar, single[i][1][0]) and mar.dtype == torch.float32, (graphed, i)
            # views into one packed buffer, end to end
            assert [m.data_ptr() - maps[0].data_ptr() for m in maps] == [0, 9600, 9600 + 9409, 2 * 9600 + 9409]
        # one pair for all queries, and none, behave as before
        same = net.segment_labels(bank, q, out_shape=(80, 120))
        assert isinstance(same, torch.Tensor) and same.shape == (4, 80, 120) and torch.equal(same[0], maps[0]) and torch.equal(same[2], maps[2])
        assert torch.equal(net.segment_labels(bank, q)[1], maps[1])
    assert 0 < int((maps[3] > 0).sum()) < maps[3].numel()
    with pytest.raises(ValueError, match="segment_labels: out_shape"):
        net.segment_labels(bank, q, out_shape=shapes[:3])


def test_canet_history_step_with_mixed_sizes_equals_single_steps(hip_lib, dev, exact_eval_variants, monkeypatch):
    from pemp_amd import synth
    from pemp_amd.entry import canet as entry
    from pemp_amd.networks import canet as m
    net = m.CaNet(None, init_channels=3, drop_rate=0.5, history=True, freeze_backbone=True)
    net.load_state_dict(synth.wgen_state_dict_for(net, 1259))
    net = net.to(dev).eval()
    data = entry.SyntheticHistoryEpisodes(20, 5678, 1, split=0, height=H, width=H, pool=5)
    data.sample_tasks()
    eps, keys = [], []
    for i in range(len(data)):                                   # the round's first episodes with pairwise different keys
        if data.history_key(i) not in keys and len(keys) < 6:
            keys.append(data.history_key(i))
            eps.append(data.task(i)[:2])
    sizes = {tuple(msk.shape[-2:]) for _, msk in eps}
    assert len(eps) == 6 and 2 <= len(sizes) < 6, sizes         # mixed sizes, one of them more than once
    alone = []
    for ep, key in zip(eps, keys):                               # each side on a fresh history table: every episode reads zeros
        ev = entry.Evaluator(net, device=dev)
        ev.reset_history(len(keys), H, H)
        alone.append(ev.test_step_history([ep], [key]).cpu())
    ev = entry.Evaluator(net, device=dev)

    def step():
        ev.reset_history(len(keys), H, H)
        return ev.test_step_history(eps, keys)
    rows = _both_ways(monkeypatch, step, len(sizes), "eval_tail", "eval_tail_ragged")
    assert torch.equal(rows, torch.cat(alone)), (rows.tolist(), torch.cat(alone).tolist())
