"""RPMMs (networks/rpmms.py, entry/rpmms.py of the reference) without a GPU: the state_dict surface, the entry's configuration,
the checks that fail before any launch, the semantics of the EM's initial mu (``set_pmm_init`` / ``resample_pmm_init``) and the
reference-made fixtures (tests/golden/make_golden_rpmms.py) being usable."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests import util

KS = (1, 3, 6)
ROWS = {1: slice(0, 1), 3: slice(1, 4), 6: slice(4, 10)}


def _net(**cfg):
    from pemp_amd.networks import rpmms as m
    return m.RPMMs(None, **cfg) if cfg else m.RPMMs(None)


def test_state_dict_matches_the_reference_keys_shapes_and_dtypes():
    net = _net()
    spec = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in net.state_dict().items()]
    assert spec == util.key_spec("rpmms")
    assert len(spec) == 295
    keys = [k for k, _, _ in spec]
    for name in ("model_res.conv1.weight", "layer5.0.weight", "layer5.1.running_var", "layer55.0.bias", "layer56.0.weight",
                 "layer6.aspp_0.0.weight", "layer6.aspp_4.0.bias", "layer7.0.weight", "layer9.bias", "residule1.1.weight",
                 "residule3.3.bias"):
        assert name in keys, name
    assert "pmm_mu0" not in keys                                           # the EM's init is no checkpoint entry
    net.load_state_dict(util.wgen_state_dict("rpmms", seed=1259))         # the fixtures' weights load as they are
    assert net.residule1[1].weight.shape[1] == 258 and net.layer56[0].weight.shape[1] == 258


def test_constructor_reads_no_pretrained_file(monkeypatch):
    from pemp_amd.networks import rpmms as m

    def no_load(*a, **k):
        raise AssertionError("the constructor must not read a checkpoint")
    monkeypatch.setattr(torch, "load", no_load)
    net = m.ModelClass(None)
    assert net.num_pro_list == [1, 3, 6]
    assert m.net_ingredient.cfg == dict(dist_scalar=20, init_channels=3, out_channels=512, backbone="resnet50", protos=3,
                                        drop_rate=0.5)


def test_load_weights_keeps_the_aspp_key_fallback(tmp_path):
    """rpmms.py:328-340: a checkpoint that misses keys is completed key by key through the ``aspp`` -> ``layer6`` renaming."""
    import logging
    net = _net()
    sd = util.wgen_state_dict("rpmms", seed=1259)
    torch.save({"state_dict": sd}, tmp_path / "a.pth")
    net.load_weights(tmp_path / "a.pth", logging.getLogger("t"))
    assert torch.equal(net.layer9.bias.detach(), sd["layer9.bias"])
    broken = dict(sd)
    del broken["layer9.bias"]                                              # nothing the fallback can find: the error surfaces
    torch.save(broken, tmp_path / "b.pth")
    with pytest.raises(RuntimeError):
        net.load_weights(tmp_path / "b.pth", logging.getLogger("t"))


def test_entry_config_keys_match_the_reference():
    from pemp_amd.entry import rpmms as entry
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        entry.ex.run_commandline(["rpmms", "print_config"])
    text = buf.getvalue()
    for key in ("tag", "shot", "query", "split", "seed", "ckpt", "exp_id", "loss", "sigma", "loss_coef", "p", "dist_scalar",
                "init_channels", "out_channels", "backbone", "protos", "drop_rate"):
        assert f"'{key}'" in text, key
    assert "'rpmms'" in text


def _episode(B=1, S=1, H=97, W=97, Q=1):
    return (torch.zeros(B, S, 3, H, W), torch.zeros(B, S, 2, H, W), torch.zeros(B, Q, 3, H, W))


def test_bad_inputs_fail_before_any_launch():
    net = _net().eval()
    with pytest.raises(ValueError, match=r"rpmms\.py:129.*266-267"):
        net(*_episode(S=5))
    with pytest.raises(ValueError, match=r"rpmms\.py:129.*266-267"):
        net(*_episode(Q=2))
    with pytest.raises(ValueError, match=r"rpmms\.py:129"):
        net.lowres(*_episode(S=5))
    with pytest.raises(RuntimeError):                                       # CPU tensors: no CPU path
        net(*_episode())
    assert net.feature_hw(401, 401) == (51, 51) and net.feature_hw(97, 97) == (13, 13)
    from pemp_amd.entry import rpmms as entry
    with pytest.raises(ValueError, match="1-shot"):
        entry.ex.run_commandline(["rpmms", "test", "with", "split=0", "shot=5", "ckpt=wgen"])


def test_train_is_not_implemented():
    net = _net().train()
    with pytest.raises(NotImplementedError, match="RPMMs is an inference path here"):
        net(*_episode())
    with pytest.raises(NotImplementedError, match="RPMMs is an inference path here"):
        net.lowres(*_episode())
    from pemp_amd.entry import rpmms as entry
    with pytest.raises(NotImplementedError, match="RPMMs is an inference path here"):
        entry.ex.run_commandline(["rpmms", "train", "with", "split=0"])


def test_pmm_init_is_drawn_pinned_and_resampled_as_specified():
    net = _net()
    assert tuple(net.pmm_mu0.shape) == (10, 256) and net.pmm_mu0.dtype == torch.float32
    assert (net.pmm_mu0.norm(dim=1) - 1).abs().max().item() <= 1e-5       # unit rows from the constructor's draw
    assert not net.pmm_init_pinned
    # resample: the reference's draw (rpmms.py:41-43) for K = 1, 3, 6 in this order from one generator
    net.resample_pmm_init(torch.Generator().manual_seed(11))
    gen = torch.Generator().manual_seed(11)
    for k in KS:
        mu = torch.empty(1, 256, k).normal_(0, (2.0 / k) ** 0.5, generator=gen)
        mu = mu / (1e-6 + mu.norm(dim=1, keepdim=True))
        assert torch.equal(net.pmm_mu0[ROWS[k]], mu[0].t()), k              # the row layout: row 0 | rows 1..3 | rows 4..9
    assert (net.pmm_mu0.norm(dim=1) - 1).abs().max().item() <= 1e-5
    drawn = net.pmm_mu0.clone()
    net.step_pmm_init()                                                    # an evaluation step draws again
    assert not torch.equal(net.pmm_mu0, drawn)
    # pin: [256,K] and [1,256,K] both, and a pinned init survives a step
    g = util.gold("rpmms_small")
    net.set_pmm_init({1: torch.from_numpy(g["mu0_k1"]), 3: torch.from_numpy(g["mu0_k3"])[None], 6: g["mu0_k6"]})
    assert net.pmm_init_pinned
    for k in KS:
        assert np.array_equal(net.pmm_mu0[ROWS[k]].numpy(), g[f"mu0_k{k}"].T)
    pinned = net.pmm_mu0.clone()
    ptr = net.pmm_mu0.data_ptr()
    net.step_pmm_init()
    net.step_pmm_init()
    assert torch.equal(net.pmm_mu0, pinned) and net.pmm_init_pinned
    net.resample_pmm_init()                                                # only an explicit call ends it
    assert not net.pmm_init_pinned and not torch.equal(net.pmm_mu0, pinned)
    assert net.pmm_mu0.data_ptr() == ptr                                   # refilled in place: a captured graph keeps reading it
    with pytest.raises(ValueError):
        net.set_pmm_init({1: torch.zeros(256, 1), 3: torch.zeros(256, 3)})
    with pytest.raises(ValueError):
        net.set_pmm_init({1: torch.zeros(256, 1), 3: torch.zeros(256, 3), 6: torch.zeros(6, 256)})
    assert "pmm_mu0" not in net.state_dict()


@pytest.mark.parametrize("name", ["rpmms_small", "rpmms_full"])
def test_fixtures_are_not_degenerate(name):
    """The generator's conditions, restated on the stored data."""
    g = util.gold(name)
    seeds, H = g["seeds"], int(g["H"])
    B, h = len(seeds), (H - 1) // 8 + 1
    assert int(g["passes"]) == 3 and int(g["shot"]) == 1
    for k in KS:
        assert g[f"mu0_k{k}"].shape == (256, k)
        assert np.abs(np.linalg.norm(g[f"mu0_k{k}"].astype(np.float64), axis=0) - 1).max() <= 1e-5
        for side in ("f", "b"):
            mu = g[f"mu_{side}_k{k}"]
            assert mu.shape == (B, k, 256) and np.isfinite(mu).all()
            nrm = np.linalg.norm(mu.astype(np.float64), axis=2)
            # a row is a unit vector, or exactly 0: a component that attracted no pixel (one-hot assignments at kappa = 20) is
            # divided by 1e-6 + 0 and stays dead, in the reference as here
            assert (np.minimum(np.abs(nrm - 1), nrm) <= 1e-4).all() and (nrm.max(axis=1) > 0.5).all(), (k, side, nrm)
    for p in range(3):
        lg = g[f"p{p}_logits"]
        assert lg.shape == (B, 2, h, h) and np.isfinite(lg).all()
        assert float(g[f"f64_err_p{p}"]) <= util.LOGIT_TOL / 4             # the reference's own float32 error
        pm = g[f"p{p}_prob_s"]
        assert pm.shape[:2] == (B, 2) and np.abs(pm.sum(axis=1) - 1).max() <= 1e-5 and 0.02 < pm[:, 1].mean() < 0.98
        n = 0
        while f"o{n}_out_hw" in g:
            ho, wo = (int(v) for v in g[f"o{n}_out_hw"])
            am = np.unpackbits(g[f"p{p}_o{n}_argmax_bits"])[:B * ho * wo].reshape(B, ho, wo)
            for b in range(B):
                assert set(np.unique(am[b])) == {0, 1}, (name, p, n, b)     # both classes in every arg-max
            assert np.isfinite(float(g[f"p{p}_o{n}_loss"]))
            assert float(g[f"p{p}_o{n}_masked"]) <= 0.01                   # far inside assert_argmax_exact's 3 % cap
            n += 1
        assert n >= 1
        if p:
            assert np.abs(lg - g[f"p{p - 1}_logits"]).max() > 0.2          # every pass moves the logits
            assert float(g[f"p{p}_change"]) > 0.2
    assert g["layer5_s"].shape[0] == 2 * B and g["aspp_in_s"].shape[0] == B
