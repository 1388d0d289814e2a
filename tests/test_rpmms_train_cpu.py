"""RPMMs head training without a GPU: the trainer module imports, ``train_head`` exists and checks its arguments before any device
work, ``train`` still raises, an unfrozen trunk is refused, ``freeze_trunk`` freezes exactly the trunk, the reference-made
train-step fixtures (tests/golden/make_golden_rpmms_train.py) are usable and the torch restatement of the head
(tests/rpmms_ref.py) reproduces their float64 gradients."""
import numpy as np
import pytest
import torch

from tests import rpmms_ref, util

STEP_CASES = ["rpmms_trainstep", "rpmms_trainstep_p0"]


def _net():
    from pemp_amd.networks import rpmms as m
    return m.RPMMs(None)


def _run(*argv):
    from pemp_amd.entry import rpmms as e
    try:
        return e.ex.run_commandline(["prog", *argv])
    finally:
        for ing in e.INGREDIENTS[1:] + [e.net_ingredient, e.ex]:
            ing._updates.clear()
            ing._cfg = None


def test_trainer_module_imports():
    from pemp_amd import train_ops as T, train_rpmms
    assert issubclass(train_rpmms.RPMMsTrainer, train_rpmms.Stage1Trainer)
    assert train_rpmms.RPMMsHeadTrainEngine.aspp_drop_names == tuple(f"layer6.aspp_{i}.2" for i in range(5))
    # 10 columns x min(16, ceil(hw / 4)) pixel blocks x 9 taps x 256 channels per image
    assert T.rpmms_proto_bwd_work_floats(2, 13, 13) == 2 * 10 * 16 * 9 * 256 and T.rpmms_proto_bwd_work_floats(1, 1, 1) == 10 * 9 * 256


def test_train_head_command_checks_its_arguments():
    from pemp_amd.entry import rpmms as entry
    assert "train_head" in entry.ex.commands and "train" in entry.ex.commands
    with pytest.raises(ValueError, match="shot=1 query=1"):
        _run("train_head", "with", "split=0", "ckpt=wgen", "shot=5")
    with pytest.raises(ValueError, match="synthetic episodes only"):
        _run("train_head", "with", "split=0", "ckpt=wgen", "data.base_dir=/nowhere")
    with pytest.raises(NotImplementedError, match="RPMMs is an inference path here"):
        _run("train", "with", "split=0")


def test_an_unfrozen_trunk_is_refused_before_any_device_work():
    from pemp_amd.train_rpmms import RPMMsHeadTrainEngine, RPMMsTrainer
    net = _net()
    with pytest.raises(ValueError, match="trunk training is not built"):
        RPMMsTrainer(net, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="trunk training is not built"):
        RPMMsHeadTrainEngine(net, torch.device("cpu"))
    with pytest.raises(ValueError, match="eagerly"):
        RPMMsTrainer(_net().freeze_trunk(), device=torch.device("cpu"), use_graph=True)


def test_freeze_trunk_freezes_exactly_the_trunk():
    from pemp_amd.train_engine import flat_layout
    net = _net()
    assert any(p.requires_grad for p in net.model_res.parameters())
    assert net.freeze_trunk() is net
    for k, p in net.named_parameters():
        assert p.requires_grad == (not k.startswith("model_res.")), k
    assert net.layer5[1].weight.requires_grad and net.layer5[1].bias.requires_grad
    params, offs, n = flat_layout(net)
    named = {id(p): k for k, p in net.named_parameters()}
    assert [named[id(p)] for p in params] == list(rpmms_ref.HEAD) and len(params) == 34
    tail = [k for k in rpmms_ref.HEAD if k.startswith(("layer6.", "layer7.", "layer9.", "residule"))]
    assert list(rpmms_ref.HEAD[-len(tail):]) == tail                      # the per-pass tail is the end of the flat layout


@pytest.mark.parametrize("name", STEP_CASES)
def test_step_fixtures_load_and_name_every_head_parameter(name):
    g, g64 = util.gold(name), util.gold(name + "_f64")
    B, H, p = len(g["seeds"]), int(g["H"]), float(g["p"])
    h = (H - 1) // 8 + 1
    assert [int(s) for s in g["seeds"]] == [3, 4] and int(g["seed_pair"]) == 0 and H == 97 and p == (0.5 if name == "rpmms_trainstep" else 0.0)
    assert float(g["proto_err"]) <= float(g["proto_limit"])              # the seed condition of the generator
    # ... and its draw condition: a float32-sized difference of the trunk moves no sampled gradient by more than half of the
    # 3e-3 that util.check_gradients allows for switches (decided on the reference alone; p = 0 has no draws to choose)
    assert float(g["stable_limit"]) == 1.5e-3 and int(g["draw_seed"]) >= 78 and (p == 0 or float(g["stability"]) <= 1.5e-3)
    names = [str(n) for n in g["grad_names"]]
    assert [n for n, v in zip(names, g["grad_norms"]) if v >= 0] == list(rpmms_ref.HEAD)
    assert all(n.startswith("model_res.") for n, v in zip(names, g["grad_norms"]) if v < 0)
    for n, v32, v64 in zip(names, g["grad_norms"], g64["grad_norms64"]):
        assert (v32 < 0) == (v64 < 0) and (v32 < 0 or n in rpmms_ref.ZERO_GRAD or (v32 > 0 and v64 > 0)), n
    sampled = {k[len("grad__"):] for k in g.files if k.startswith("grad__")}
    assert sampled == {k[len("g64__"):] for k in g64.files if k.startswith("g64__")}
    assert {"layer55.0.weight", "layer56.0.weight", "residule1.1.weight", "layer5.1.weight", "layer9.weight"} <= sampled and len(sampled) >= 10
    assert float(g64["history_grad_norm64"]) > 0                          # the history channels of residule1.1 get a gradient
    for q in range(3):
        assert g[f"low32_p{q}"].shape == g64[f"low64_p{q}"].shape == (B, 2, h, h)
    for k, calls in rpmms_ref.DROP_CALLS.items():
        u = g["draws__" + k]
        assert u.shape == (calls, B, 256) and u.dtype == np.float32 and np.abs(u - (1 - p)).min() > 1e-6
    for K in rpmms_ref.KS:
        assert g[f"mu0_k{K}"].shape == (256, K) and g64[f"mu_f64_k{K}"].shape == (B, K, 256)
        np.testing.assert_allclose(np.linalg.norm(g[f"mu0_k{K}"], axis=0), 1.0, atol=1e-5)
    assert g["loss"].shape == g64["loss64"].shape == (3,) and np.abs(g["loss"] - g64["loss64"]).max() < 1e-4


def test_trajectory_fixture():
    t = util.gold("rpmms_trajectory")
    l32, l64 = t["losses32"], t["losses64"]
    assert l32.shape == l64.shape == (5, 3) and float(t["lr"]) == 1e-4 and [int(s) for s in t["seeds"]] == [3, 4]
    assert l64[4, 0] < l64[0, 0] and np.isfinite(l32).all()
    assert abs(l64[0, 0] - float(util.gold("rpmms_trainstep_p0_f64")["loss64"][0])) < 1e-9       # step 0 is the p = 0 step fixture


@pytest.mark.parametrize("name", STEP_CASES)
def test_restatement_reproduces_the_reference_step_in_float64(name):
    """tests/rpmms_ref.py on the oracle's train-mode trunk (two batches: supports, then queries) against the reference's own
    float64 step: prototypes, losses, low-resolution logits, every gradient norm and the sampled gradients.  Both sides are
    float64 evaluations of the same function in another op order; the EM's ten iterations and three chained passes amplify
    the last-bit differences, so the bound is taken from the two runs' own difference at the FIRST quantity both compute --
    the prototypes: a relative error ``e_mu`` there allows ``1e3 * e_mu + 1e-9`` downstream (three passes of ~20 layers)."""
    g, sup, msk, qry, gt, mu0, draws = rpmms_ref.fixture_inputs(name)
    g64 = util.gold(name + "_f64")
    sd = rpmms_ref.fixture_state_dict()
    cat_s = rpmms_ref.trunk_cat23(sd, sup.flatten(0, 1))
    cat_q = rpmms_ref.trunk_cat23(sd, qry.flatten(0, 1))
    ls, outs, grads, protos = rpmms_ref.head_step(cat_s, cat_q, msk, gt, sd, mu0, torch.float64, draws=draws, p=float(g["p"]))
    e_mu = max(float((protos[K][s] - torch.from_numpy(g64[f"mu_{'fb'[s]}64_k{K}"])).abs().max()) for K in rpmms_ref.KS for s in (0, 1))
    tol = 1e3 * e_mu + 1e-9
    print(f"{name}: |prototypes - reference float64| {e_mu:.2e} -> relative bound {tol:.2e}")
    assert e_mu <= 1e-9
    assert np.abs(np.array(ls) - g64["loss64"]).max() <= tol * max(1.0, abs(ls[0]))
    for q in range(3):
        assert np.abs(outs[q].numpy() - g64[f"low64_p{q}"]).max() <= tol * np.abs(g64[f"low64_p{q}"]).max(), q
    norms = {str(n): float(v) for n, v in zip(g["grad_names"], g64["grad_norms64"])}
    for k in rpmms_ref.HEAD:
        if k not in rpmms_ref.ZERO_GRAD:
            assert abs(float(grads[k].norm()) - norms[k]) <= tol * norms[k], k
    for key in [k for k in g64.files if k.startswith("g64__")]:
        got, ref = grads[key[len("g64__"):]], torch.from_numpy(g64[key])
        got = (got if got.numel() <= 40000 else got.reshape(-1)[::37]).reshape(ref.shape)
        assert float((got - ref).abs().max()) <= tol * float(ref.abs().max()), key
    assert float(grads["residule1.1.weight"][:, 256:258].norm()) > 0
