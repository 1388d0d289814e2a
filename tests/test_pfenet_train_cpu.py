"""PFENet head training without a GPU: the command surface, the torch restatement of the step (tests/pfenet_ref.py) against the
reference-made fixtures (tests/golden/make_golden_pfenet_train.py), and the fixtures' non-degeneracy."""
import numpy as np
import pytest
import torch

from tests import pfenet_ref, util

CASES = ["pfenet_trainstep", "pfenet_trainstep5", "pfenet_trainstep_p0"]


def _net(shot):
    from pemp_amd import synth
    from pemp_amd.networks.pfenet import WGEN_SEED, ModelClass
    net = ModelClass(shot, None)
    net.load_state_dict(synth.wgen_state_dict_for(net, WGEN_SEED))
    return net


def _batch(seeds, shot, H):
    from pemp_amd import synth
    b = synth.make_batch([int(s) for s in seeds], shot=shot, height=H, width=H, out_hw=(H, H))
    return tuple(torch.from_numpy(b[k]) for k in ("sup_img", "sup_mask", "qry_img", "qry_mask"))


@pytest.fixture(scope="module")
def restated():
    """{(case, trunk mode): (loss, aux)} of the float64 restatement, computed once per case and mode."""
    cache = {}

    def run(case, mode):
        if (case, mode) not in cache:
            g = util.gold(case)
            shot, H = int(g["shot"]), int(g["H"])
            sup, msk, qry, gt = _batch(g["seeds"], shot, H)
            sd = _net(shot).state_dict()
            feats = pfenet_ref.trunk_features(sd, sup, msk, qry, torch.float64, mode)
            draws = {k: torch.from_numpy(g["draws__" + k]) for k in pfenet_ref.DROPS}
            out = pfenet_ref.head_step(*feats[:4], gt.reshape(-1, H, H), sd, shot, torch.float64, draws, drop=bool(g["dropout"]))
            cache[(case, mode)] = (out[0], out[1], feats[4])
        return cache[(case, mode)]
    return run


def test_commands():
    from pemp_amd.entry import pfenet as entry
    assert "train_head" in entry.ex.commands and "train" in entry.ex.commands and "test" in entry.ex.commands

    def run(*argv):
        try:
            return entry.ex.run_commandline(["pfenet", *argv])
        finally:                                                              # no update outlives its command
            for ing in entry.INGREDIENTS[1:] + [entry.ex]:
                ing._updates.clear()
                ing._cfg = None

    with pytest.raises(NotImplementedError, match="PFENet is an inference path here"):
        run("train", "with", "split=0")
    with pytest.raises(ValueError, match="one query"):
        run("train_head", "with", "split=0", "query=2", "ckpt=wgen")
    net = _net(1).train()
    sup, msk, qry, _ = _batch((3,), 1, 97)
    with pytest.raises(NotImplementedError, match="PFENet is an inference path here"):
        net(sup, msk, qry)


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_reference_step(restated, case):
    """The S + 1 per-call batch-statistics passes (query, shot 0, shot 1, ...) + the head restatement give the reference's float64
    losses to 1e-9, and leave the three stored BatchNorms with the reference's running statistics."""
    g64 = util.gold(case + "_f64")
    loss, aux, sd = restated(case, "per_call")
    print(f"  {case}: loss {loss:.12f} (ref {float(g64['loss64']):.12f}), aux {aux:.12f} (ref {float(g64['aux64']):.12f})")
    assert abs(loss - float(g64["loss64"])) <= 1e-9 and abs(aux - float(g64["aux64"])) <= 1e-9
    for key in [k for k in g64.files if k.startswith("bn64__") and not k.endswith("num_batches_tracked")]:
        ref = torch.from_numpy(g64[key])
        assert float((sd[key[len("bn64__"):]] - ref).abs().max()) <= 1e-9 * max(1.0, float(ref.abs().max())), key


@pytest.mark.parametrize("mode", ["one_pass", "eval"])
def test_other_batchnorm_orders_do_not_reproduce_it(restated, mode):
    """One pass over all B (S + 1) images, or the running statistics, is a different function: why the engine runs S + 1 passes."""
    for case in ("pfenet_trainstep", "pfenet_trainstep5"):
        g64 = util.gold(case + "_f64")
        loss, aux, _ = restated(case, mode)
        diff = max(abs(loss - float(g64["loss64"])), abs(aux - float(g64["aux64"])))
        print(f"  {case} {mode}: loss {loss:.6f} aux {aux:.6f}: off by {diff:.3e}")
        assert diff > 1e-3


@pytest.mark.parametrize("case", CASES)
def test_fixtures_are_not_degenerate(case):
    g, g64 = util.gold(case), util.gold(case + "_f64")
    names, norms = [str(n) for n in g["grad_names"]], g["grad_norms"]
    head = [n for n, v in zip(names, norms) if v >= 0]
    assert len(head) == 35 and len(names) - len(head) == 165
    assert all(n.startswith(pfenet_ref.TRUNK) for n, v in zip(names, norms) if v < 0)
    assert (norms[norms >= 0] > 0).all() and (g64["grad_norms64"][norms >= 0] > 0).all()
    sampled = {k[len("grad__"):] for k in g.files if k.startswith("grad__")}
    for part in ("down_query.", "down_supp.", "init_merge.0.", "init_merge.2.", "alpha_conv.", "beta_conv.", "inner_cls.0.0.",
                 "inner_cls.1.3.weight", "inner_cls.1.3.bias", "res1.", "res2.", "cls."):
        assert any(s.startswith(part) for s in sampled), part
    for b in range(len(g["seeds"])):
        assert set(np.unique(g64["low64"][b].argmax(0))) == {0, 1}
    shot = int(g["shot"])
    for k in g.files:
        if k.endswith("num_batches_tracked"):
            assert int(g[k]) == shot + 1
    assert tuple(g["draws__down_supp.2"].shape) == (len(g["seeds"]) * shot, 256)
    assert float(g["down_supp_support_min_abs"]) > float(g["down_supp_f32_error"])


def test_trajectory_descends():
    t = util.gold("pfenet_trajectory")
    tot = t["losses64"] + t["aux64"]
    assert len(tot) == 5 and tot[-1] < 0.5 * tot[0]
    assert np.abs(t["losses32"] - t["losses64"]).max() < 1e-5 and np.abs(t["aux32"] - t["aux64"]).max() < 1e-5
