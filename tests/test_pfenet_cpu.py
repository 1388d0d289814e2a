"""PFENet (networks/pfenet.py of the reference) without a GPU: the state_dict surface, the entry's configuration, the checks
that fail before any launch, and the reference-made fixtures (tests/golden/make_golden_pfenet.py) being usable."""
import json

import numpy as np
import pytest
import torch

from tests import util


def _net(shot=1):
    from pemp_amd.networks import pfenet as m
    return m.PFENet(shot, None)


def test_state_dict_matches_the_reference_keys_shapes_and_dtypes():
    net = _net()
    spec = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in net.state_dict().items()]
    assert spec == util.key_spec("pfenet")
    net.load_state_dict(util.wgen_state_dict("pfenet", seed=1259))        # the fixtures' weights load as they are


def test_constructor_reads_no_pretrained_file(monkeypatch):
    from pemp_amd.networks import pfenet as m

    def no_load(*a, **k):
        raise AssertionError("the constructor must not read a checkpoint")
    monkeypatch.setattr(torch, "load", no_load)
    net = m.ModelClass(5, None)
    assert net.shot == 5 and net.ppm_scales == [60, 30, 15, 8]


def test_entry_config_keys_match_the_reference():
    from pemp_amd.entry import pfenet as entry
    import contextlib
    import io
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        entry.ex.run_commandline(["pfenet", "print_config"])
    text = buf.getvalue()
    for key in ("tag", "shot", "query", "split", "seed", "ckpt", "exp_id", "loss", "sigma", "loss_coef", "p"):
        assert f"'{key}'" in text, key
    assert "'pfenet'" in text


def _episode(B=1, S=1, H=97, W=97, Q=1):
    return (torch.zeros(B, S, 3, H, W), torch.zeros(B, S, 2, H, W), torch.zeros(B, Q, 3, H, W))


@pytest.mark.parametrize("shape,err", [
    (dict(H=97, W=105), ValueError),          # non-square (pfenet.py:204,222,225)
    (dict(H=96, W=96), ValueError),           # (H - 1) % 8 != 0 (:164)
    (dict(Q=2), ValueError),                  # query != 1
    (dict(), RuntimeError),                   # CPU tensors: no CPU path
])
def test_bad_inputs_fail_before_any_launch(shape, err):
    net = _net().eval()
    sup, msk, qry = _episode(**shape)
    with pytest.raises(err):
        net(sup, msk, qry)


def test_train_mode_forward_is_not_implemented():
    net = _net().train()
    with pytest.raises(NotImplementedError, match="PFENet is an inference path here"):
        net(*_episode())
    from pemp_amd.entry import pfenet as entry
    with pytest.raises(NotImplementedError, match="PFENet is an inference path here"):
        entry.ex.run_commandline(["pfenet", "train", "with", "split=0"])


@pytest.mark.parametrize("name", ["pfenet_small", "pfenet_small5", "pfenet_full"])
def test_fixtures_are_not_degenerate(name):
    g = util.gold(name)
    seeds, shot, H = g["seeds"], int(g["shot"]), int(g["H"])
    assert g["sim_spread"].shape == (len(seeds), shot) and (g["sim_spread"] > 0.05).all()
    for k in range(4):
        p = g[f"prior_bin{k}"]
        assert p.shape == (len(seeds),) + ((60, 30, 15, 8)[k],) * 2
        assert p.min() >= 0.0 and p.max() <= 1.0 + 1e-6 and p.max() - p.min() > 0.05
    n = 0
    while f"o{n}_out_hw" in g:
        ho, wo = (int(v) for v in g[f"o{n}_out_hw"])
        am = np.unpackbits(g[f"o{n}_argmax_bits"])[:len(seeds) * ho * wo].reshape(len(seeds), ho, wo)
        for b in range(len(seeds)):
            assert set(np.unique(am[b])) == {0, 1}, (name, n, b)
        if H <= 97:
            assert (g[f"o{n}_logits"].argmax(1) == am).all()
        assert np.isfinite(float(g[f"o{n}_loss"]))
        n += 1
    assert n >= 1
    assert g["supp_vec"].shape == (len(seeds), 256) and (g["supp_vec"] >= 0).all()
    assert json.dumps(util.key_spec("pfenet"))        # the key spec the model is pinned to is readable
