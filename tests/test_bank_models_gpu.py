"""Prototype banks through the models: ``segment(enroll(supports), queries)`` against ``forward`` on the same episodes, bit for
bit.  The claim is that of test_eval_protocol_gpu.py::test_batched_evaluation_gives_identical_metrics -- image rows are
independent in the conv GEMMs and the exact conv variants are bit-identical to each other -- plus the bank kernel's own
contract (tests/test_bank_ops_gpu.py), so supports encoded apart from their queries give the same prototypes and the same map.
Inputs are 97 x 97 (13 x 13 features), wgen weights."""
import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu
HW = (80, 120)


def _episodes(seeds, shot, dev, hw=HW):
    ts = [util.episode_tensors(s, shot, 97, hw, dev) for s in seeds]
    cat = lambda k: torch.cat([t[k] for t in ts])
    return cat("sup_img"), cat("sup_mask"), cat("qry_img"), cat("qry_mask")


def _make(kind, dev):
    from pemp_amd.networks import baseline, panet, pemp_stage1
    if kind == "stage1_rn50":
        net, sd = pemp_stage1.PEMPStage1(None), util.wgen_state_dict("stage1_rn50")
    elif kind == "stage1_vgg16":
        net, sd = pemp_stage1.PEMPStage1(None, backbone="vgg16"), util.wgen_state_dict("stage1_vgg16")
    elif kind == "stage1_map":
        net, sd = pemp_stage1.PEMPStage1(None, protos=0), util.wgen_state_dict("stage1_rn50")
        sd.pop("ctr")
    elif kind == "baseline_vgg16":
        net, sd = baseline.Baseline(None, backbone="vgg16"), util.wgen_state_dict("baseline_vgg16")
    elif kind == "baseline_rn50":
        net, sd = baseline.Baseline(None, backbone="resnet50"), util.wgen_state_dict("baseline_rn50")
    else:
        net, sd = panet.PANet(None, backbone="vgg16"), util.wgen_state_dict("panet_vgg16")
    net.load_state_dict(sd)
    return net.to(dev).eval()


_MODELS = {}


@pytest.fixture
def net_of(hip_lib, dev):
    """Models are shared by the tests of this module (their engines and arenas with them)."""
    def get(kind):
        if kind not in _MODELS:
            _MODELS[kind] = _make(kind, dev)
        return _MODELS[kind]
    yield get


@pytest.fixture(scope="module", autouse=True)
def _drop_models():
    yield
    _MODELS.clear()


@pytest.mark.parametrize("kind,shot,resp", [
    ("stage1_rn50", 1, True), ("stage1_rn50", 5, True), ("stage1_vgg16", 1, True), ("stage1_map", 2, True),
    ("baseline_vgg16", 1, False), ("baseline_rn50", 1, False), ("panet_vgg16", 1, False)])
def test_segment_of_enrolled_supports_equals_forward(net_of, dev, exact_eval_variants, kind, shot, resp):
    net = net_of(kind)
    B = 3
    sup, msk, qry, _ = _episodes((3, 11, 12), shot, dev)
    with torch.no_grad():
        if kind == "stage1_map":
            ref = net(sup, msk, qry, HW, ret_ind=True, protos=0)
        elif resp:
            ref = net(sup, msk, qry, HW, ret_ind=True)
        elif kind == "panet_vgg16":
            ref = net(sup, msk, qry, HW)[0]
        else:
            ref = net(sup, msk, qry, HW)
        ref_protos = net.__dict__["_last_protos"].clone()
        bank = net.enroll(sup, msk, labels=[7, 8, 9])
        got = net.segment(bank, qry[:, 0], index=list(range(B)), out_shape=HW, ret_ind=resp)
    assert len(bank) == B and bank.labels == [7, 8, 9] and bank.protos.shape == ref_protos.shape
    assert torch.equal(bank.protos, ref_protos), f"{kind}: prototypes differ, max |d| {(bank.protos - ref_protos).abs().max().item():.3e}"
    if resp:
        assert got[0].shape == (B, 2) + HW and got[1].shape == (B,) + HW and got[1].dtype == torch.int64
        assert torch.equal(got[0], ref[0]), f"{kind}: logits differ, max |d| {(got[0] - ref[0]).abs().max().item():.3e}"
        assert torch.equal(got[1], ref[1]), f"{kind}: response differs at {(got[1] != ref[1]).sum().item()} pixels"
    else:
        assert got.shape == (B, 2) + HW
        assert torch.equal(got, ref), f"{kind}: logits differ, max |d| {(got - ref).abs().max().item():.3e}"
        with pytest.raises(ValueError, match="ret_ind"):
            net.segment(bank, qry[:, 0], index=list(range(B)), ret_ind=True)
    # default output size: the query's own
    with torch.no_grad():
        full = net.segment(bank, qry[:1, 0], index=[0])
    assert full.shape == (1, 2, 97, 97)


def _compare(g, e, logits, tgt, ltol=util.LOGIT_TOL):
    """tests/test_models_gpu.py::_compare (its logits / arg-max / loss bounds; the bank path keeps no episode feature map)."""
    logits = logits.cpu()
    lref = torch.from_numpy(g[f"e{e}_logits_s7"])
    lerr = (logits[0, :, ::7, ::7] - lref).abs().max().item()
    assert lerr < ltol, f"logit err {lerr}"
    am = logits.argmax(1).numpy().astype(np.uint8)
    ref_bits = np.unpackbits(g[f"e{e}_argmax_bits"])[: am.size].reshape(am.shape)
    agree = 1.0 - util.assert_argmax_exact(logits, ref_bits, margin=2 * ltol, max_masked=0.02)
    print(f"|dlogit| {lerr:.2e}  pixels outside the margin {agree:.5f}")
    loss = torch.nn.functional.cross_entropy(logits, tgt.cpu(), ignore_index=255).item()
    assert abs(loss - float(g[f"e{e}_loss"])) < 2e-4
    return lerr, agree


@pytest.mark.parametrize("kind,fixture", [("stage1_rn50", "stage1_rn50_small"), ("stage1_rn50", "stage1_rn50_small5"),
                                          ("baseline_vgg16", "baseline_vgg16_small")])
def test_bank_path_matches_reference_golden(net_of, dev, kind, fixture):
    net = net_of(kind)
    g = util.gold(fixture)
    shot, H = int(g["shot"]), int(g["H"])
    for e, seed in enumerate(g["seeds"]):
        hw = tuple(int(v) for v in g[f"e{e}_out_hw"])
        t = util.episode_tensors(seed, shot, H, hw, dev)
        with torch.no_grad():
            out = net.segment(net.enroll(t["sup_img"], t["sup_mask"]), t["qry_img"][:, 0], index=[0], out_shape=hw)
        _compare(g, e, out, t["qry_mask"])


def test_all_classes_form_equals_indexed_calls(net_of, dev, exact_eval_variants):
    net = net_of("stage1_rn50")
    sup, msk, qry, _ = _episodes((3, 11, 12), 1, dev)
    q = qry[:2, 0]
    with torch.no_grad():
        bank = net.enroll(sup, msk)
        logits, resp = net.segment(bank, q, out_shape=HW, ret_ind=True)
        low, lresp = net.segment_lowres(bank, q, ret_ind=True)
        assert logits.shape == (2, 3, 2) + HW and resp.shape == (2, 3) + HW and low.shape == (2, 3, 2, 13, 13) and lresp.shape == (2, 3, 13, 13)
        for k in range(3):
            lk, rk = net.segment(bank, q, index=[k, k], out_shape=HW, ret_ind=True)
            assert torch.equal(logits[:, k], lk) and torch.equal(resp[:, k], rk), k
            pk, prk = net.segment_lowres(bank, q, index=[k, k], ret_ind=True)
            assert torch.equal(low[:, k], pk) and torch.equal(lresp[:, k], prk), k
        assert net.segment(bank, q, out_shape=HW).shape == (2, 3, 2) + HW


def test_graphed_segment_reads_the_bank_in_place(net_of, dev, exact_eval_variants):
    net = net_of("stage1_rn50")
    sup, msk, qry, _ = _episodes((3, 11, 12, 14), 1, dev)
    q = qry[:3, 0].contiguous()
    index = [2, 0, 1]
    with torch.no_grad():
        bank = net.enroll(sup[:3], msk[:3])
        other = net.enroll(sup[3:], msk[3:])
        eager = [t.clone() for t in net.segment_lowres(bank, q, index=index, ret_ind=True)]
        g0 = [t.clone() for t in net.segment_graphed(bank, q, index=index, ret_ind=True)]
        g1 = [t.clone() for t in net.segment_graphed(bank, q, index=index, ret_ind=True)]        # a replay
        n_graphs = len(net._engine["graphs"])
        assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(eager, g0, g1))
        # another index through the same graph (the static int32 buffer)
        e2 = net.segment_lowres(bank, q, index=[1, 1, 0], ret_ind=True)
        g2 = net.segment_graphed(bank, q, index=[1, 1, 0], ret_ind=True)
        assert torch.equal(e2[0], g2[0]) and torch.equal(e2[1], g2[1]) and not torch.equal(g2[0], eager[0])
        # new prototypes for class 1, in place: the same graph sees them
        ptr = bank.protos.data_ptr()
        bank.update(1, other)
        assert bank.protos.data_ptr() == ptr and torch.equal(bank.protos[1], other.protos[0])
        e3 = net.segment_lowres(bank, q, index=index, ret_ind=True)
        g3 = net.segment_graphed(bank, q, index=index, ret_ind=True)
        assert torch.equal(e3[0], g3[0]) and torch.equal(e3[1], g3[1])
        assert not torch.equal(e3[0][2], eager[0][2]) and torch.equal(e3[0][:2], eager[0][:2])      # query 2 meets class 1
        assert len(net._engine["graphs"]) == n_graphs
        # the all-classes form has a graph of its own
        ga = net.segment_graphed(bank, q)
        ea = net.segment_lowres(bank, q)
        assert ga[1] is None and torch.equal(ga[0], ea[0]) and len(net._engine["graphs"]) == n_graphs + 1


def test_enroll_into_an_existing_bank_is_in_place(net_of, dev, exact_eval_variants):
    for kind in ("stage1_rn50", "baseline_vgg16"):
        net = net_of(kind)
        sup, msk, _, _ = _episodes((3, 11, 12, 14), 1, dev)
        with torch.no_grad():
            bank = net.enroll(sup[:2], msk[:2], labels=[1, 2])
            fresh = net.enroll(sup[2:], msk[2:])
            ptr = bank.protos.data_ptr()
            assert net.enroll(sup[2:], msk[2:], labels=[3, 4], out=bank) is bank
        assert bank.protos.data_ptr() == ptr and torch.equal(bank.protos, fresh.protos) and bank.labels == [3, 4]
        with pytest.raises(ValueError, match="classes"):
            net.enroll(sup[:3], msk[:3], out=bank)
    # heads that condition on the query have no bank
    from pemp_amd.networks import pemp_stage2
    with pytest.raises(ValueError, match="prototype-matching"):
        pemp_stage2.PEMPStage2(1, 1, None).eval().enroll(sup[:1], msk[:1])
    # a bank travels: state_dict -> host -> a new bank on the device
    from pemp_amd.bank import PrototypeBank
    back = PrototypeBank.from_state_dict({k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in bank.state_dict().items()}, device=dev)
    assert back.protos.is_cuda and torch.equal(back.protos, bank.protos) and bank.to(dev) is bank and not bank.to("cpu").protos.is_cuda
