"""CANet (networks/canet.py, entry/canet.py of the reference) without a GPU: the state_dict surface, the entry's configuration,
the checks that fail before any launch, the reference-made fixtures (tests/golden/make_golden_canet.py) being usable, the two
evaluator rules (group closing, key -> rank assignment) and the "test_canet" data mode."""
import contextlib
import io
import itertools

import numpy as np
import pytest
import torch

from tests import util


def _net(**cfg):
    from pemp_amd.networks import canet as m
    return m.CaNet(None, **cfg) if cfg else m.CaNet(None)


def test_state_dict_matches_the_reference_keys_shapes_and_dtypes():
    net = _net()
    spec = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in net.state_dict().items()]
    assert spec == util.key_spec("canet")
    net.load_state_dict(util.wgen_state_dict("canet", seed=1259))         # the fixtures' weights load as they are
    nh = _net(init_channels=3, drop_rate=0.5, history=False, freeze_backbone=True)
    assert nh.residual_1[1].weight.shape[1] == 256 and net.residual_1[1].weight.shape[1] == 258


def test_constructor_reads_no_pretrained_file(monkeypatch):
    from pemp_amd.networks import canet as m

    def no_load(*a, **k):
        raise AssertionError("the constructor must not read a checkpoint")
    monkeypatch.setattr(torch, "load", no_load)
    net = m.ModelClass(None)
    assert net.use_history is True and net.num_classes == 2
    assert set(m.net_ingredient.cfg) == {"init_channels", "drop_rate", "history", "freeze_backbone"}
    assert m.net_ingredient.cfg == dict(init_channels=3, drop_rate=0.5, history=True, freeze_backbone=True)


def test_entry_config_keys_match_the_reference():
    from pemp_amd.entry import canet as entry
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        entry.ex.run_commandline(["canet", "print_config"])
    text = buf.getvalue()
    for key in ("tag", "shot", "query", "split", "seed", "ckpt", "exp_id", "loss", "sigma", "history", "freeze_backbone",
                "drop_rate", "init_channels"):
        assert f"'{key}'" in text, key
    assert "'canet'" in text


def _episode(B=1, S=1, H=97, W=97, Q=1):
    return (torch.zeros(B, S, 3, H, W), torch.zeros(B, S, 2, H, W), torch.zeros(B, Q, 3, H, W))


def test_bad_inputs_fail_before_any_launch():
    net = _net().eval()
    with pytest.raises(ValueError, match="one query"):
        net(*_episode(Q=2))
    with pytest.raises(ValueError, match="history_mask"):                  # 97 x 97 gives a 13 x 13 feature map
        net(*_episode(), history_mask=torch.zeros(1, 1, 2, 12, 13))
    with pytest.raises(RuntimeError):                                       # CPU tensors: no CPU path
        net(*_episode())
    with pytest.raises(RuntimeError):
        net(*_episode(), history_mask=torch.zeros(1, 1, 2, 13, 13))
    assert net.feature_hw(401, 401) == (51, 51) and net.feature_hw(97, 97) == (13, 13)


def test_train_is_not_implemented():
    net = _net().train()
    with pytest.raises(NotImplementedError, match="CANet is an inference path here"):
        net(*_episode())
    from pemp_amd.entry import canet as entry
    with pytest.raises(NotImplementedError, match="CANet is an inference path here"):
        entry.ex.run_commandline(["canet", "train", "with", "split=0"])


@pytest.mark.parametrize("name", ["canet_small", "canet_small5", "canet_full"])
def test_fixtures_are_not_degenerate(name):
    g = util.gold(name)
    seeds, shot, H = g["seeds"], int(g["shot"]), int(g["H"])
    B, h = len(seeds), (H - 1) // 8 + 1
    assert int(g["passes"]) == 3
    for p in range(3):
        lg = g[f"p{p}_logits"]
        assert lg.shape == (B, 2, h, h) and np.isfinite(lg).all()
        n = 0
        while f"o{n}_out_hw" in g:
            ho, wo = (int(v) for v in g[f"o{n}_out_hw"])
            am = np.unpackbits(g[f"p{p}_o{n}_argmax_bits"])[:B * ho * wo].reshape(B, ho, wo)
            for b in range(B):
                assert set(np.unique(am[b])) == {0, 1}, (name, p, n, b)
            assert np.isfinite(float(g[f"p{p}_o{n}_loss"]))
            assert float(g[f"p{p}_o{n}_masked"]) <= 0.01                   # far inside assert_argmax_exact's 3 % cap
            n += 1
        assert n >= 1
    assert np.abs(g["p1_logits"] - g["p0_logits"]).max() > 100 * util.LOGIT_TOL     # the history input matters
    assert g["z"].shape == (B, 256) and (g["z"] >= 0).all() and g["z"].max() > 0
    assert g["layer5_s"].shape[0] == B * (shot + 1) and g["layer55_s"].shape[0] == B and g["aspp_in_s"].shape[0] == B
    if name == "canet_small":
        assert np.abs(g["nh_p0_logits"] - g["p0_logits"]).max() > 100 * util.LOGIT_TOL   # another model, not a copy


def _key_sequences():
    rs = np.random.RandomState(7)
    seqs = [[], [5], [1, 1, 1, 1], [1, 2, 3, 4, 5, 6, 7], [1, 2, 1, 2, 3, 3, 4, 1]]
    seqs += [[(int(c), int(q)) for c, q in zip(rs.randint(1, 4, n), rs.randint(0, 3, n))] for n in (10, 57, 200)]
    return seqs


@pytest.mark.parametrize("batch", [1, 2, 4, 25])
def test_group_closing_rule(batch):
    from pemp_amd.entry.canet import close_groups
    for keys in _key_sequences():
        groups = close_groups(keys, batch)
        assert list(itertools.chain.from_iterable(groups)) == list(range(len(keys)))         # in order, nothing lost
        for gi, g in enumerate(groups):
            assert 1 <= len(g) <= batch
            ks = [keys[i] for i in g]
            assert len(set(ks)) == len(ks)                                                   # no key twice in a group
            if len(g) < batch and gi + 1 < len(groups):                                      # short only before a repeat
                assert keys[groups[gi + 1][0]] in ks
    assert close_groups([1, 2, 3, 4, 5], 2) == [[0, 1], [2, 3], [4]]
    assert close_groups([1, 2, 1, 3], 4) == [[0, 1], [2, 3]]


@pytest.mark.parametrize("world", [1, 2, 8])
def test_key_to_rank_assignment(world):
    from pemp_amd.entry.canet import assign_ranks
    for keys in _key_sequences():
        parts = assign_ranks(keys, world)
        assert len(parts) == world
        assert sorted(itertools.chain.from_iterable(parts)) == list(range(len(keys)))        # the union is the round
        owner = {}
        for r, part in enumerate(parts):
            assert part == sorted(part)                                                      # round order kept
            for i in part:
                assert owner.setdefault(keys[i], r) == r                                     # a key lives on one rank
        assert assign_ranks(keys, world) == parts                                            # pure
    assert assign_ranks(["a", "b", "a"], 8) == [[0, 2], [1]] + [[]] * 6                      # more ranks than keys


def test_synthetic_history_episodes_repeat_their_queries():
    from pemp_amd.entry.canet import SyntheticHistoryEpisodes
    data = SyntheticHistoryEpisodes(40, 5678, 1, split=0, height=97, width=97, pool=3)
    data.sample_tasks()
    keys = [data.history_key(i) for i in range(40)]
    assert len(set(keys)) < 20 and {k[0] for k in keys} <= set(range(1, 6)) and {k[1] for k in keys} <= {0, 1, 2}
    i, j = next((i, j) for i in range(40) for j in range(i + 1, 40) if keys[i] == keys[j])
    (s0, _, q0), m0, c0 = data.task(i)
    (s1, _, q1), m1, c1 = data.task(j)
    assert torch.equal(q0, q1) and torch.equal(m0, m1) and int(c0) == int(c1) == keys[i][0]  # the query is a function of the key
    assert not torch.equal(s0, s1)                                                           # the supports are the episode's


def test_test_canet_mode_follows_the_reference_sampler(tmp_path):
    from pemp_amd.data_kits import pascal_voc as pv
    lists = util.make_tiny_voc(tmp_path, splits=("val",))
    cfg = dict(dataset="PASCAL", base_dir=str(tmp_path), height=97, width=97, seed=1234, test_seed=5678, train_n=12, test_n=9,
               cache=True, mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225], bs=4, test_bs=1, one_cls=0)
    ds, ncls = pv.load(cfg, "test_canet", 0, 2)
    assert ncls == 20 and ds.classes == [1, 2, 3, 4, 5] and len(ds) == 9
    ds.reset_sampler()
    for _ in range(2):                                       # two rounds from one sampler stream, as the reference's loop
        ds.sample_tasks()
        if _ == 0:
            rs = np.random.RandomState(5678)                 # the reference's statements, pascal_voc.py:318-323
        for i in range(9):
            c = rs.choice([1, 2, 3, 4, 5])
            idx = rs.choice(len(lists[("val", c)]), size=3, replace=False)
            assert ds.tasks[i] == (int(c), [lists[("val", c)][j] for j in idx])
            assert ds.history_key(i) == (int(c), int(idx[2]))
    sup, qry, cls = ds.decoded_task(0)
    assert len(sup) == 2 and len(qry) == 1 and cls == ds.tasks[0][0]
