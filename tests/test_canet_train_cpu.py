"""CANet head training without a GPU: the reference-made train-step fixtures (tests/golden/make_golden_canet_train.py) are usable,
the torch restatement of the head (tests/canet_ref.py) reproduces them in float64, the flat parameter layout of a frozen CANet
holds the head only, the ``train_head`` command exists and trunk training is refused before any device work."""
import numpy as np
import pytest
import torch

from tests import canet_ref, util

STEP_CASES = ["canet_trainstep", "canet_trainstep5", "canet_trainstep_nh"]


def _net(**cfg):
    from pemp_amd.networks import canet as m
    return m.CaNet(None, **cfg) if cfg else m.CaNet(None)


@pytest.mark.parametrize("name", STEP_CASES)
def test_step_fixtures_are_not_degenerate(name):
    g, g64 = util.gold(name), util.gold(name + "_f64")
    B, shot, H = len(g["seeds"]), int(g["shot"]), int(g["H"])
    h = (H - 1) // 8 + 1
    p = float(g["p"])
    names = [str(n) for n in g["grad_names"]]
    assert [n for n, v in zip(names, g["grad_norms"]) if v >= 0] == list(canet_ref.HEAD)          # the 30 head tensors, in order
    assert all(n.startswith("encoder.") for n, v in zip(names, g["grad_norms"]) if v < 0)
    for v32, v64 in zip(g["grad_norms"], g64["grad_norms64"]):
        assert (v32 < 0) == (v64 < 0) and (v32 < 0 or (v32 > 0 and v64 > 0))                      # every trainable gradient is non-zero
    assert {k[len("grad__"):] for k in g.files if k.startswith("grad__")} == {k[len("g64__"):] for k in g64.files if k.startswith("g64__")}
    assert g["history"].shape == (B, 2, h, h) and g64["low64"].shape == (B, 2, h, h)
    if bool(g["use_history"]):
        assert g["history"].max() > 0 and float(g64["history_grad_norm64"]) > 0                   # the history channels get a gradient
    am = g64["low64"].argmax(1)
    for b in range(B):
        assert set(np.unique(am[b])) == {0, 1}
    for k in canet_ref.DROPS:
        u = g["draws__" + k]
        assert u.shape == ((B * (shot + 1) if k == "layer5.2" else B), 256) and u.dtype == np.float32
        assert np.abs(u - (1 - p)).min() > 1e-6                                                   # no draw on the keep threshold
    # no gradient-carrying support pre-activation of layer5 within the reference's own float32 error of zero (make_golden_canet_train.py)
    assert float(g["layer5_support_min_abs"]) > float(g["layer5_f32_error"]) > 0
    assert np.isfinite(float(g["loss"])) and abs(float(g["loss"]) - float(g64["loss64"])) < 1e-4


def test_trajectory_fixture_descends():
    t = util.gold("canet_trajectory")
    l32, l64 = t["losses32"], t["losses64"]
    assert l32.shape == l64.shape == (5,) and float(t["lr"]) == 1e-4
    assert l64[4] < 0.5 * l64[0] and np.abs(l32 - l64).max() < 1e-4


@pytest.mark.parametrize("name", STEP_CASES)
def test_restatement_reproduces_the_reference_step_in_float64(name):
    """tests/canet_ref.py on the oracle's eval-mode trunk against the reference's own float64 step: loss, low-resolution logits,
    every gradient norm and the sampled gradients.  Both sides are float64 evaluations of the same function in another op order:
    1e-9 relative."""
    g, sup, msk, qry, gt, hist, draws = canet_ref.fixture_inputs(name)
    g64 = util.gold(name + "_f64")
    B, S = sup.shape[:2]
    sd = canet_ref.fixture_state_dict(bool(g["use_history"]))
    cat23 = canet_ref.trunk_cat23(sd, sup, qry, torch.float64)
    loss, low, grads = canet_ref.head_step(cat23, msk, gt, sd, B, S, torch.float64, history=hist, draws=draws, p=float(g["p"]),
                                           use_history=bool(g["use_history"]))
    assert abs(loss - float(g64["loss64"])) <= 1e-9 * max(1.0, abs(loss))
    assert np.abs(low.numpy() - g64["low64"]).max() <= 1e-9 * np.abs(g64["low64"]).max()
    norms = {str(n): float(v) for n, v in zip(g["grad_names"], g64["grad_norms64"])}
    for k in canet_ref.HEAD:
        assert abs(float(grads[k].norm()) - norms[k]) <= 1e-8 * norms[k], k
    for key in [k for k in g64.files if k.startswith("g64__")]:
        got, ref = grads[key[len("g64__"):]], torch.from_numpy(g64[key])
        got = (got if got.numel() <= 40000 else got.reshape(-1)[::37]).reshape(ref.shape)
        assert float((got - ref).abs().max()) <= 1e-8 * float(ref.abs().max()), key


def test_flat_layout_of_a_frozen_canet_is_the_head():
    from pemp_amd.train_engine import flat_layout
    net = _net()
    net.maybe_fix_params()
    params, offs, n = flat_layout(net)
    named = {id(p): k for k, p in net.named_parameters()}
    assert [named[id(p)] for p in params] == list(canet_ref.HEAD) and len(params) == 30
    assert all(o % 4 == 0 for o in offs) and n >= sum(p.numel() for p in params)
    assert not any(p.requires_grad for k, p in net.named_parameters() if k.startswith("encoder."))


def test_train_head_command_is_registered():
    from pemp_amd.entry import canet as entry
    assert "train_head" in entry.ex.commands and "train" in entry.ex.commands


def test_trunk_training_is_rejected_before_any_device_work():
    from pemp_amd.train_canet import CANetHeadTrainEngine, CANetTrainer
    net = _net(init_channels=3, drop_rate=0.5, history=True, freeze_backbone=False)
    with pytest.raises(ValueError, match="trunk training"):
        CANetTrainer(net, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="trunk training"):
        CANetHeadTrainEngine(net, torch.device("cpu"))
    with pytest.raises(ValueError, match="eagerly"):
        CANetTrainer(_net(), device=torch.device("cpu"), use_graph=True)
