"""The enroll-once evaluation protocol (entry.pemp_stage1.BankEvaluator) and the ``test_bank`` command.

A round through the BankEvaluator must give what the ordinary Evaluator gives on the EQUIVALENT episodes: the same tasks with
every task's supports replaced by those of the round's first task of its class -- the same table, the same loss, and (with the
exact conv variants) the same per-episode statistics rows, bit for bit, whatever the number of queries per step."""
import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu

N_EPISODES, SEED = 12, 5678        # tests/test_bank_cpu.py holds that this round covers every validation class of split 0


def _equivalent(base):
    class FirstSupportEpisodes(base):
        """Every task with the supports of the round's first task of its class."""

        def sample_tasks(self):
            super().sample_tasks()
            self._tasks = [base.task(self, i) for i in range(len(self))]
            self._first = {}
            for i, (_, _, cls) in enumerate(self._tasks):
                self._first.setdefault(int(cls), i)

        def task(self, i):
            (_, _, qry), msk, cls = self._tasks[i]
            sup, sup_mask, _ = self._tasks[self._first[int(cls)]][0]
            return (sup, sup_mask, qry), msk, cls
    return FirstSupportEpisodes


def _recording(monkeypatch, e):
    """Every round's statistics rows, classes and fetched table, as the loop hands them to / takes them from DeviceRoundTable."""
    log = {"rows": [], "classes": [], "fetched": []}
    add, fetch = e.DeviceRoundTable.add, e.DeviceRoundTable.fetch

    def rec_add(self, stats, classes):
        log["rows"].append(stats.cpu().clone())
        log["classes"].append(classes.cpu().clone())
        return add(self, stats, classes)

    def rec_fetch(self):
        out = fetch(self)
        log["fetched"].append(out)
        return out
    monkeypatch.setattr(e.DeviceRoundTable, "add", rec_add)
    monkeypatch.setattr(e.DeviceRoundTable, "fetch", rec_fetch)
    return log


@pytest.mark.parametrize("shot", [1, 2])
def test_bank_round_equals_the_round_on_equivalent_episodes(hip_lib, dev, exact_eval_variants, monkeypatch, shot):
    from pemp_amd.entry import pemp_stage1 as e
    net = e.ModelClass(None)
    net.load_state_dict(util.wgen_state_dict("stage1_rn50"))
    net = net.to(dev).eval()
    labels = e.get_val_labels(0)
    data = lambda cls=e.SyntheticEpisodes: cls(N_EPISODES, SEED, shot, split=0, height=97, width=97)
    probe = data()
    probe.sample_tasks()
    assert {int(probe.task(i)[2]) for i in range(N_EPISODES)} == set(labels)           # every validation class occurs
    log = _recording(monkeypatch, e)
    runs = []
    for make in (lambda: (e.Evaluator(net, device=dev), data(_equivalent(e.SyntheticEpisodes)), 4),
                 lambda: (e.BankEvaluator(net, device=dev), data(), 1),
                 lambda: (e.BankEvaluator(net, device=dev), data(), 4),
                 lambda: (e.BankEvaluator(net, device=dev, use_graph=False), data(), 5)):
        ev, ds, batch = make()
        for k in log:
            log[k].clear()
        res = ev.start_eval_loop(ds, 20, 0, te_epochs=2, batch=batch)
        runs.append((res, [r.clone() for r in log["rows"]], [c.clone() for c in log["classes"]], list(log["fetched"]), ev))
    (loss0, miou0, biou0), rows0, cls0, fetched0, _ = runs[0]
    assert len(rows0) == 2 and rows0[0].shape == (N_EPISODES, 8) and np.isfinite(miou0).all()
    for (loss, miou, biou), rows, cls, fetched, ev in runs[1:]:
        for r in range(2):
            assert torch.equal(cls[r], cls0[r])
            assert torch.equal(rows[r], rows0[r]), f"round {r}: statistics rows differ at {(rows[r] != rows0[r]).any(dim=1).nonzero().flatten().tolist()}"
            assert np.array_equal(fetched[r][0], fetched0[r][0]) and fetched[r][1] == fetched0[r][1] and fetched[r][2] == fetched0[r][2]
        assert np.array_equal(ev.round_miou, runs[0][4].round_miou) and np.array_equal(ev.round_biou, runs[0][4].round_biou)
        assert abs(loss - loss0) <= 1e-12 and np.abs(np.asarray(miou) - np.asarray(miou0)).max() <= 1e-12 \
            and np.abs(np.asarray(biou) - np.asarray(biou0)).max() <= 1e-12
        assert len(ev.bank) == len(labels) and ev.bank.labels == [int(c) for c in labels]


def test_test_bank_command_end_to_end(hip_lib, dev, tmp_path):
    from pemp_amd.entry import baseline as eb, pemp_stage1 as e

    def run(entry, *argv):
        try:
            return entry.ex.run_commandline(["prog", *argv])
        finally:
            for ing in entry.ex.ingredients + [entry.ex]:
                ing._updates.clear()
                ing._cfg = None

    small = ["split=0", "ckpt=wgen", "data.test_n=6", "te.epochs=1", "data.height=97", "data.width=97"]
    out = run(e, "test_bank", "with", *small)
    assert out.startswith("Loss:") and "mIoU:" in out and "bIoU:" in out
    assert run(e, "test_bank", "with", *small, "data.test_bs=4") == out                # queries per step do not matter
    assert run(eb, "test_bank", "with", *small, "shot=2").startswith("Loss:")
    # the disk route: a PASCAL-5i directory tree through the same command
    voc = tmp_path / "VOC2012"
    util.make_tiny_voc(voc, splits=("val",))
    disk = run(e, "test_bank", "with", *small, f"data.base_dir={voc}", "data.test_n=14", "data.test_bs=3")
    assert disk.startswith("Loss:") and disk != out
