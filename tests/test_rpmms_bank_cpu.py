"""RPMMs support banks, the parts that need no GPU: the RPMMsBank container, the argument checks of the two C entries, the model's
refusals and the ``test_bank`` command's registration."""
import ctypes
import io

import pytest
import torch

from pemp_amd.bank import PFENetBank, PrototypeBank, RPMMsBank

C = 256


def _bank(k=3, c=C, labels=(1, 2, 3), seed=0, **kw):
    g = torch.Generator().manual_seed(seed)
    fields = dict(backbone="resnet50", precision="f32")
    fields.update(kw)
    return RPMMsBank(torch.randn(k, 2, 10, c, generator=g), torch.randn(k, 10, 9, c, generator=g), labels=labels, **fields)


def test_rpmms_bank_construction_and_validation():
    bank = _bank()
    assert len(bank) == 3 and (bank.family, bank.backbone, bank.precision, bank.C) == ("rpmms", "resnet50", "f32", C)
    assert bank.labels == [1, 2, 3] and "K=3" in repr(bank) and "rpmms" in repr(bank)
    assert bank.nbytes() == 112640                                  # (2 * 10 + 10 * 9) * 256 floats per class
    assert len(bank.tensors()) == 2 and bank.tensors()[0] is bank.mu and bank.tensors()[1] is bank.taps and bank.to("cpu") is bank
    mu, taps = (t.clone() for t in bank.tensors())
    mk = lambda **kw: RPMMsBank(kw.get("mu", mu), kw.get("taps", taps), "resnet50", "f32")
    for bad in (dict(mu=mu[0]), dict(mu=mu[:, :1]), dict(mu=mu[:, :, :9]), dict(mu=mu.double()), dict(mu=mu[:0]),
                dict(taps=taps[:2]), dict(taps=taps[:, :, :8]), dict(taps=taps[..., :128]), dict(taps=taps.double()),
                dict(taps=taps.to("meta"))):                        # the last one: two devices
        with pytest.raises(ValueError, match="RPMMsBank"):
            mk(**bad)
    with pytest.raises(ValueError, match="labels"):
        _bank(labels=(1, 2))
    assert _bank(labels=None).labels is None


def test_rpmms_bank_empty_like_holds_and_update():
    bank = _bank()
    keep = [t.clone() for t in bank.tensors()]
    one = _bank(k=1, labels=(9,), seed=2)
    empty = RPMMsBank.empty_like(one, 5, labels=[1, 2, 3, 4, 5])
    assert type(empty) is RPMMsBank and len(empty) == 5 and not empty.mu.any() and not empty.taps.any() and empty.holds(one)
    assert (empty.backbone, empty.precision, empty.C, empty.labels) == ("resnet50", "f32", C, [1, 2, 3, 4, 5])
    assert not empty.holds(_bank(k=1, c=128, labels=None)) and not empty.holds(PrototypeBank(torch.zeros(1, 2, 512), "baseline", "vgg16", "f32", 20))
    # update copies one class into the bank's own storage
    ptrs = [t.data_ptr() for t in bank.tensors()]
    assert bank.update(1, one) is bank and [t.data_ptr() for t in bank.tensors()] == ptrs
    assert torch.equal(bank.mu[1], one.mu[0]) and torch.equal(bank.taps[1], one.taps[0]) and bank.labels == [1, 9, 3]
    for k in (0, 2):
        assert torch.equal(bank.mu[k], keep[0][k]) and torch.equal(bank.taps[k], keep[1][k])
    bank.update(0, _bank(k=1, labels=None, seed=3))                 # a source without labels keeps the slot's label
    assert bank.labels == [1, 9, 3]
    bank.update(0, one, label=4)
    assert bank.labels == [4, 9, 3]
    with pytest.raises(ValueError, match="no labels"):
        _bank(labels=None).update(0, one)
    with pytest.raises(IndexError):
        bank.update(3, one)
    with pytest.raises(ValueError, match="one class"):
        bank.update(0, _bank(k=2, labels=None))
    for other in (torch.zeros(2, 10, C), PrototypeBank(torch.zeros(1, 2, 512), "baseline", "vgg16", "f32", 20)):
        with pytest.raises(TypeError, match="RPMMsBank"):
            bank.update(0, other)
    for field, kw in (("backbone", dict(backbone="resnet101")), ("precision", dict(precision="bf16")), ("C", dict(c=128))):
        with pytest.raises(ValueError, match=f"mismatch in {field}"):
            bank.update(0, _bank(k=1, labels=None, **kw))
        with pytest.raises(ValueError, match=f"mismatch in {field}"):
            bank.require_like(_bank(**kw), "test")
    bank.require_like(_bank(k=7, labels=None, seed=5), "test")     # K is not part of the likeness


def test_rpmms_bank_round_trips():
    bank = _bank()
    sd = bank.state_dict()
    assert all(isinstance(v, (torch.Tensor, int, float, str, list, type(None))) for v in sd.values())
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    loaded = torch.load(buf, weights_only=True)
    again = RPMMsBank.from_state_dict(loaded)
    assert all(torch.equal(a, b) and a.data_ptr() != b.data_ptr() for a, b in zip(again.tensors(), bank.tensors()))
    assert again.state_dict().keys() == sd.keys()
    for f in ("family", "backbone", "precision", "C", "labels"):
        assert getattr(again, f) == getattr(bank, f), f
    other = _bank(seed=1, labels=None)
    ptrs = [t.data_ptr() for t in other.tensors()]
    assert other.load_state_dict(loaded) is other
    assert [t.data_ptr() for t in other.tensors()] == ptrs and torch.equal(other.mu, bank.mu) and torch.equal(other.taps, bank.taps)
    assert other.labels == [1, 2, 3]
    with pytest.raises(ValueError, match="RPMMsBank"):
        other.load_state_dict(_bank(k=2, labels=None).state_dict())
    with pytest.raises(ValueError, match="family"):
        RPMMsBank.from_state_dict({**loaded, "family": "pfenet"})
    with pytest.raises(ValueError, match="RPMMsBank"):
        other.load_state_dict({**loaded, "family": "pfenet"})


def test_c_entries_validate_before_any_device_work(hip_lib):
    buf = (ctypes.c_float * 64)()                   # host memory: never dereferenced, only its address is looked at
    p = ctypes.cast(buf, ctypes.c_void_p)
    p = ctypes.c_void_p((p.value + 15) & ~15)
    off = ctypes.c_void_p(p.value + 4)
    err = hip_lib.pemp_last_error
    taps, l56 = hip_lib.pemp_rpmms_proto_taps_f32, hip_lib.pemp_rpmms_bank_l56_f32
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert taps(*args, 1, C, None) == -1 and b"null pointer" in err()
    assert taps(p, p, p, 0, C, None) == -1 and b"bad sizes" in err()
    assert taps(p, p, p, 1, 128, None) == -1 and b"C = 256" in err()
    for args in ((off, p, p), (p, off, p), (p, p, off)):
        assert taps(*args, 1, C, None) == -1 and b"16-byte aligned" in err()

    def call(qry=p, ldq=C, base=p, ldb=C, bias=p, mu=p, T=p, index=None, out=p, ldo=288, gstride=288 * 9, N=1, K=1, h=3, w=3, c=C, dil=2):
        return l56(qry, ldq, base, ldb, bias, mu, T, index, out, ldo, gstride, N, K, h, w, c, dil, None)
    for name in ("qry", "base", "bias", "mu", "T", "out"):
        assert call(**{name: None}) == -1 and b"null pointer" in err(), name
        assert call(**{name: off}) == -1 and b"16-byte aligned" in err(), name
    assert call(c=128) == -1 and b"C = 256" in err()
    assert call(ldo=257) == -1 and b"ldo >= C + 2" in err()
    assert call(ldo=256) == -1 and b"ldo >= C + 2" in err()
    for kw in (dict(ldq=258), dict(ldb=258), dict(ldo=262), dict(gstride=2), dict(ldq=128), dict(ldb=128)):
        assert call(**kw) == -1 and b"multiples of 4" in err(), kw
    for kw in (dict(N=0), dict(K=0), dict(N=300, K=300), dict(h=0), dict(dil=0)):
        assert call(**kw) == -1 and b"bad sizes" in err(), kw


def test_model_refusals_need_no_gpu():
    from pemp_amd.networks import rpmms
    net = rpmms.RPMMs(None)
    sup, msk = torch.zeros(2, 1, 3, 97, 97), torch.zeros(2, 1, 2, 97, 97)
    with pytest.raises(RuntimeError, match="eval"):
        net.train().enroll(sup, msk)
    net.eval()
    with pytest.raises(RuntimeError, match="GPU"):
        net.enroll(sup, msk)                                        # CPU inputs: no CPU path
    with pytest.raises(ValueError, match="1-shot"):
        net.enroll(torch.zeros(2, 2, 3, 97, 97), torch.zeros(2, 2, 2, 97, 97))
    with pytest.raises(ValueError, match="sup_mask"):
        net.enroll(sup, msk[:1])
    bank = _bank(k=2, labels=None)
    q = torch.zeros(1, 3, 97, 97)
    others = (PrototypeBank(torch.zeros(2, 2, 512), "baseline", "vgg16", "f32", 20),
              PFENetBank(torch.zeros(2, 1, 64, 2048), torch.zeros(2, 1, 64), torch.ones(2, 1, dtype=torch.int32), torch.zeros(2, 256), 169,
                         "resnet50v2", "f32"))
    for call in (net.segment, net.segment_lowres, net.segment_graphed):
        with pytest.raises(RuntimeError, match="GPU"):
            call(bank, q, index=[1])
        with pytest.raises(RuntimeError, match="GPU"):
            call(bank, torch.zeros(1, 3, 105, 97))                  # any size the trunk takes: the bank holds none
        with pytest.raises(ValueError, match="index values"):
            call(bank, q, index=[2])
        with pytest.raises(ValueError, match="ret_ind"):
            call(bank, q, ret_ind=True)
        with pytest.raises(ValueError, match="precision = "):
            call(_bank(k=2, labels=None, precision="bf16"), q)
        with pytest.raises(ValueError, match="qry_img"):
            call(bank, q[None])
        for other in others:
            with pytest.raises(TypeError, match="RPMMsBank"):
                call(other, q)
    with pytest.raises(RuntimeError, match="eval"):
        rpmms.RPMMs(None).train().segment(bank, q)
    for other in others:
        with pytest.raises(TypeError, match="RPMMsBank"):
            net.enroll(sup, msk, out=other)


def test_test_bank_command_is_registered():
    from pemp_amd.entry import rpmms
    assert "test_bank" in rpmms.ex.commands and "test" in rpmms.ex.commands

    def run(*argv):
        try:
            return rpmms.ex.run_commandline(["prog", *argv])
        finally:
            for ing in rpmms.ex.ingredients + [rpmms.ex]:
                ing._updates.clear()
                ing._cfg = None
    with pytest.raises(ValueError, match="split"):
        rpmms.ex.run("test_bank")                                   # split = -1: refused with test's own message, before any model
    with pytest.raises(ValueError, match="shot=1 query=1"):
        run("test_bank", "with", "split=0", "shot=5")
    with pytest.raises(ValueError, match="shot=1 query=1"):
        run("test_bank", "with", "split=0", "query=2")
    assert set(rpmms.ex.cfg) == {"tag", "shot", "query", "split", "seed", "ckpt", "exp_id", "loss", "sigma", "loss_coef",
                                 "trunk_precision", "p"}            # no configuration key of its own
    # the shared body keeps the other entries' result line
    import inspect
    from pemp_amd.entry import pemp_stage1
    sig = inspect.signature(pemp_stage1.run_test_bank)
    assert sig.parameters["evaluator"].default is None and sig.parameters["loss_label"].default == "Loss"
    assert issubclass(rpmms.BankEvaluator, pemp_stage1.BankEvaluator)
