"""PFENet support banks, the parts that need no GPU: the PFENetBank container, the argument checks of the ops wrappers and of the C
entries, the model's refusals, and the ``empty_like`` hook the enroll-once evaluator builds its bank with."""
import ctypes
import io

import pytest
import torch

from pemp_amd import _lib, ops
from pemp_amd.bank import PFENetBank, PrototypeBank


@pytest.fixture
def no_library(monkeypatch):
    """The checks under test come before the library is touched."""
    def load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", load)


def _bank(k=3, s=2, cap=128, c=64, hw=150, counts=None, labels=(1, 2, 3), seed=0, **kw):
    g = torch.Generator().manual_seed(seed)
    count = torch.full((k, s), 70, dtype=torch.int32) if counts is None else torch.tensor(counts, dtype=torch.int32)
    fields = dict(backbone="resnet50v2", precision="f32")
    fields.update(kw)
    return PFENetBank(torch.randn(k, s, cap, c, generator=g), torch.rand(k, s, cap, generator=g), count, torch.rand(k, 256, generator=g),
                      hw, labels=labels, **fields)


def test_pfenet_bank_construction_and_validation():
    bank = _bank()
    assert len(bank) == 3 and (bank.family, bank.S, bank.HW, bank.C, bank.cap) == ("pfenet", 2, 150, 64, 128)
    assert bank.labels == [1, 2, 3] and torch.equal(bank.count_host, bank.count) and bank.count_host is not bank.count
    assert "K=3" in repr(bank) and "cap=128" in repr(bank) and bank.nbytes() == (2 * 128 * 64 + 2 * 128 + 2 + 256) * 4
    assert len(bank.tensors()) == 4 and bank.to("cpu") is bank
    rows, norms, count, svec = (t.clone() for t in bank.tensors())
    mk = lambda **kw: PFENetBank(kw.get("rows", rows), kw.get("norms", norms), kw.get("count", count), kw.get("svec", svec),
                                 kw.get("hw", 150), "resnet50v2", "f32")
    for bad in (dict(rows=rows[:, :, :100]), dict(rows=rows[..., :48]), dict(rows=rows.double()), dict(rows=rows[0]),
                dict(norms=norms[:, :, :64]), dict(count=count.long()), dict(count=count[:2]), dict(svec=svec[:2]),
                dict(count=torch.zeros_like(count)), dict(count=torch.full_like(count, 129)), dict(hw=60)):
        with pytest.raises(ValueError, match="PFENetBank"):
            mk(**bad)
    with pytest.raises(ValueError, match="labels"):
        _bank(labels=(1, 2))


def test_pfenet_bank_round_trip_and_in_place_update():
    bank = _bank()
    sd = bank.state_dict()
    assert all(isinstance(v, (torch.Tensor, int, float, str, list, type(None))) for v in sd.values())
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    loaded = torch.load(buf, weights_only=True)
    again = PFENetBank.from_state_dict(loaded)
    assert all(torch.equal(a, b) for a, b in zip(again.tensors(), bank.tensors())) and again.state_dict().keys() == sd.keys()
    for f in ("family", "backbone", "precision", "S", "HW", "C", "cap", "labels"):
        assert getattr(again, f) == getattr(bank, f), f
    other = _bank(seed=1, labels=None)
    ptrs = [t.data_ptr() for t in other.tensors()]
    other.load_state_dict(loaded)
    assert [t.data_ptr() for t in other.tensors()] == ptrs and torch.equal(other.rows, bank.rows) and other.labels == [1, 2, 3]
    assert torch.equal(other.count_host, bank.count_host)
    with pytest.raises(ValueError):
        other.load_state_dict(_bank(k=2, labels=None).state_dict())
    with pytest.raises(ValueError, match="family"):
        PFENetBank.from_state_dict({**loaded, "family": "baseline"})
    # update copies one class into the bank's own storage; a source with another cap is fine as long as its rows fit
    ptrs = [t.data_ptr() for t in bank.tensors()]
    one = _bank(k=1, cap=64, counts=[[33, 64]], labels=(9,), seed=2)
    assert bank.update(1, one) is bank and [t.data_ptr() for t in bank.tensors()] == ptrs
    assert torch.equal(bank.rows[1, :, :64], one.rows[0]) and torch.equal(bank.norms[1, :, :64], one.norms[0])
    assert torch.equal(bank.rows[1, :, 64:], again.rows[1, :, 64:])                        # beyond the source's cap: untouched
    assert bank.count[1].tolist() == [33, 64] and bank.count_host[1].tolist() == [33, 64] and torch.equal(bank.svec[1], one.svec[0])
    assert bank.labels == [1, 9, 3]
    assert torch.equal(bank.rows[0], again.rows[0]) and torch.equal(bank.rows[2], again.rows[2]) and torch.equal(bank.count[0], again.count[0])
    wide = _bank(k=1, cap=192, counts=[[100, 5]], labels=None, seed=3)
    bank.update(0, wide)                                                                    # cap 192 into cap 128: 100 rows fit
    assert torch.equal(bank.rows[0], wide.rows[0, :, :128]) and bank.labels == [1, 9, 3]
    with pytest.raises(ValueError, match="needs 150 rows"):
        bank.update(0, _bank(k=1, cap=192, counts=[[150, 5]], labels=None))
    with pytest.raises(IndexError):
        bank.update(3, one)
    with pytest.raises(ValueError, match="one class"):
        bank.update(0, _bank(k=2, labels=None))
    with pytest.raises(TypeError):
        bank.update(0, torch.zeros(2, 128, 64))
    for field, kw in (("backbone", dict(backbone="resnet101")), ("precision", dict(precision="bf16")), ("S", dict(s=1)),
                      ("HW", dict(hw=128)), ("C", dict(c=32))):
        with pytest.raises(ValueError, match=f"mismatch in {field}"):
            bank.update(0, _bank(k=1, labels=None, **kw))
        with pytest.raises(ValueError, match=f"mismatch in {field}"):
            bank.require_like(_bank(**kw), "test")
    bank.require_like(_bank(cap=192, seed=5), "test")                                       # cap is not part of the likeness


def test_empty_like_builds_the_evaluators_banks():
    """What entry.pemp_stage1.BankEvaluator._enroll relies on.  For the prototype families the hook returns what the evaluator wrote
    by hand before: zeros [K,2p,c] with the one-class bank's fields and the split's labels."""
    one = PrototypeBank(torch.randn(1, 6, 512), "pemp_stage1", "resnet50", "f32", 20, labels=[3])
    bank = PrototypeBank.empty_like(one, 5, labels=[1, 2, 3, 4, 5])
    zeros = torch.zeros((5, 6, 512), dtype=torch.float32)
    hand = PrototypeBank(zeros, one.family, one.backbone, one.precision, one.dist_scalar, labels=[1, 2, 3, 4, 5])
    assert type(bank) is PrototypeBank and torch.equal(bank.protos, hand.protos) and bank.protos.dtype == torch.float32
    for f in ("family", "backbone", "precision", "p", "c", "dist_scalar", "labels"):
        assert getattr(bank, f) == getattr(hand, f), f
    assert bank.holds(one) and not bank.holds(PrototypeBank(torch.zeros(1, 2, 512), "pemp_stage1", "resnet50", "f32", 20))
    bank.update(2, one)
    assert torch.equal(bank.protos[2], one.protos[0]) and bank.labels == [1, 2, 3, 4, 5] and bank.tensors()[0] is bank.protos
    for family, bb, p in (("baseline", "vgg16", 1), ("panet", "vgg16", 1)):
        o = PrototypeBank(torch.randn(1, 2 * p, 512), family, bb, "f32", 20, labels=[1])
        e = PrototypeBank.empty_like(o, 5, labels=[1, 2, 3, 4, 5])
        assert (e.family, e.backbone, e.p, e.c, len(e)) == (family, bb, p, 512, 5) and not e.protos.any() and e.holds(o)
    # PFENet: slots of HW rounded up to 64 rows, each holding the one zero row of an empty mask
    pf = _bank(k=1, cap=64, hw=169, counts=[[40, 51]], labels=(4,))
    big = PFENetBank.empty_like(pf, 5, labels=[1, 2, 3, 4, 5])
    assert type(big) is PFENetBank and len(big) == 5 and (big.cap, big.S, big.HW, big.C) == (192, 2, 169, 64) and big.holds(pf)
    assert not big.rows.any() and not big.norms.any() and (big.count == 1).all() and (big.count_host == 1).all() and not big.svec.any()
    big.update(3, pf)
    assert big.labels == [1, 2, 3, 4, 5] and big.count_host[3].tolist() == [40, 51]
    assert not PFENetBank.empty_like(pf, 5, cap=64).holds(_bank(k=1, cap=128, hw=169, counts=[[100, 1]], labels=None))
    assert not big.holds(_bank(k=1, s=1, hw=169, labels=None))


def _store(k=3, s=1, cap=128, c=64):
    return torch.zeros(k, s, cap, c), torch.zeros(k, s, cap), torch.ones(k, s, dtype=torch.int32)


def test_ops_wrappers_check_their_arguments_before_the_library(no_library):
    q = torch.zeros(4, 9, 11, 64)
    rows, norms, count = _store()
    for bad in ([0, 3, 0, 0], [0, -1, 0, 0], [0, 1, 2], torch.tensor([0, 1, 2, 3]), torch.zeros(4, 1, dtype=torch.int64)):
        with pytest.raises(ValueError, match="index"):
            ops.prior_bank(q, rows, norms, count, index=bad)
    with pytest.raises(ValueError, match="CPU tensor"):
        ops.prior_bank(q, rows, norms, count, index=torch.zeros(4, dtype=torch.int32, device="meta"))
    with pytest.raises(ValueError, match="device index"):                # the launch wrapper wants the index on the device
        ops._prior_bank(q, rows, norms, count, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.prior_bank(q, *_store(cap=100))
    with pytest.raises(ValueError, match="C = 64"):
        ops.prior_bank(torch.zeros(4, 9, 11, 96), rows, norms, count)
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.prior_bank(torch.zeros(4, 9, 11, 48), *_store(c=48))
    with pytest.raises(ValueError, match="rows must be contiguous fp32"):
        ops.prior_bank(q, rows[..., ::2], norms, count)
    with pytest.raises(ValueError, match="norms"):
        ops.prior_bank(q, rows, norms[:, :, :64], count)
    with pytest.raises(ValueError, match="count"):
        ops.prior_bank(q, rows, norms, count.long())
    s, m = torch.zeros(3, 9, 11, 64), torch.zeros(3, 9, 11)
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.prior_bank_pack(s, m, 3, 1, cap=100)
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.prior_bank_pack(torch.zeros(3, 9, 11, 48), m, 3, 1)
    with pytest.raises(ValueError, match="mask"):
        ops.prior_bank_pack(s, m, 2, 1)
    with pytest.raises(ValueError, match="mask"):
        ops.prior_bank_pack(s, torch.zeros(3, 9, 12), 3, 1)
    with pytest.raises(ValueError, match="C=64"):
        ops.prior_bank_pack(torch.zeros(3, 9, 11, 96), m, 3, 1, rows=rows, norms=norms, count=count)
    with pytest.raises(ValueError, match="go together"):
        ops.prior_bank_pack(s, m, 3, 1, rows=rows)
    with pytest.raises(ValueError, match="mask"):
        ops.prior_bank_count(m.double(), 3, 1)
    with pytest.raises(ValueError, match="src"):
        ops.bank_gather_rows(torch.zeros(3, 256)[:, ::2], None, 4)
    with pytest.raises(ValueError, match="device index"):
        ops.bank_gather_rows(torch.zeros(3, 256), torch.zeros(4, dtype=torch.int64), 4)
    assert ops._round64(1) == 64 and ops._round64(64) == 64 and ops._round64(169) == 192 and ops._round64(2601) == 2624


def test_c_entries_validate_before_any_device_work(hip_lib):
    buf = (ctypes.c_float * 64)()                   # host memory: never dereferenced, only its address is looked at
    p = ctypes.cast(buf, ctypes.c_void_p)
    off = ctypes.c_void_p(p.value + 4)
    err = hip_lib.pemp_last_error
    pack, prior, gather = hip_lib.pemp_prior_bank_pack_f32, hip_lib.pemp_prior_bank_f32, hip_lib.pemp_bank_gather_rows_f32
    assert pack(p, 64, None, p, p, p, 1, 4, 64, 64, None) == -1 and b"null pointer" in err()
    assert pack(p, 64, p, p, None, p, 1, 4, 64, 64, None) == -1 and b"go together" in err()
    assert pack(None, 64, p, p, p, p, 1, 4, 64, 64, None) == -1 and b"go together" in err()
    assert pack(p, 64, p, p, p, p, 0, 4, 64, 64, None) == -1 and b"bad sizes" in err()
    assert pack(p, 64, p, p, p, p, 1, 4, 48, 64, None) == -1 and b"C % 32" in err()
    for cap in (0, 100, -64):
        assert pack(p, 64, p, p, p, p, 1, 4, 64, cap, None) == -1 and b"multiple of 64" in err()
    assert pack(p, 32, p, p, p, p, 1, 4, 64, 64, None) == -1 and b"16-byte aligned" in err()
    assert pack(off, 64, p, p, p, p, 1, 4, 64, 64, None) == -1 and b"16-byte aligned" in err()
    ok = (p, 64, p, p, p, None, p, p, 1 << 20)
    assert prior(None, 64, p, p, p, None, p, p, 1 << 20, 1, 1, 1, 4, 64, 64, None) == -1 and b"null pointer" in err()
    assert prior(*ok, 1, 1, 1, 4, 48, 64, None) == -1 and b"C % 32" in err()
    assert prior(*ok, 1, 1, 1, 4, 64, 100, None) == -1 and b"multiple of 64" in err()
    assert prior(*ok, 300, 300, 1, 4, 64, 64, None) == -1 and b"65535" in err()
    assert prior(off, 64, p, p, p, None, p, p, 1 << 20, 1, 1, 1, 4, 64, 64, None) == -1 and b"16-byte aligned" in err()
    assert prior(p, 64, p, p, p, None, p, p, 8, 1, 1, 1, 4, 64, 64, None) == -1 and b"workspace too small" in err()
    assert hip_lib.pemp_prior_bank_workspace_bytes(6, 5, 2601) == 6 * 5 * 2601 * 4
    assert gather(None, None, p, 1, 1, 4, None) == -1 and b"null pointer" in err()
    assert gather(p, None, p, 0, 1, 4, None) == -1 and b"bad sizes" in err()


def test_model_refusals_need_no_gpu():
    from pemp_amd.networks import canet, pemp_stage2, pfenet
    net = pfenet.PFENet(1, None)
    sup, msk = torch.zeros(2, 1, 3, 97, 97), torch.zeros(2, 1, 2, 97, 97)
    with pytest.raises(RuntimeError, match="eval"):
        net.train().enroll(sup, msk)
    net.eval()
    with pytest.raises(RuntimeError, match="GPU"):
        net.enroll(sup, msk)                                        # CPU inputs: no CPU path
    bank = _bank(k=2, s=1, cap=192, c=2048, hw=169, counts=[[5], [6]], labels=None)
    q = torch.zeros(1, 3, 97, 97)
    for call in (net.segment, net.segment_lowres, net.segment_graphed):
        with pytest.raises(RuntimeError, match="GPU"):
            call(bank, q, index=[1])
        with pytest.raises(ValueError, match="index values"):
            call(bank, q, index=[2])
        with pytest.raises(ValueError, match="ret_ind"):
            call(bank, q, ret_ind=True)
        with pytest.raises(ValueError, match="square"):
            call(bank, torch.zeros(1, 3, 97, 105))
        with pytest.raises(ValueError, match=r"\(H - 1\) % 8"):
            call(bank, torch.zeros(1, 3, 96, 96))
        with pytest.raises(ValueError, match="HW = 169"):
            call(bank, torch.zeros(1, 3, 105, 105))
        with pytest.raises(ValueError, match="S = 2"):
            call(_bank(k=2, s=2, cap=192, c=2048, hw=169, labels=None), q)
        with pytest.raises(ValueError, match="precision = "):
            call(_bank(k=2, s=1, cap=192, c=2048, hw=169, labels=None, precision="bf16"), q)
        with pytest.raises(TypeError, match="PFENetBank"):
            call(PrototypeBank(torch.zeros(2, 2, 512), "baseline", "vgg16", "f32", 20), q)
    with pytest.raises(RuntimeError, match="eval"):
        pfenet.PFENet(1, None).train().segment(bank, q)
    with pytest.raises(TypeError, match="PFENetBank"):
        net.enroll(sup, msk, out=PrototypeBank(torch.zeros(2, 2, 512), "baseline", "vgg16", "f32", 20))
    # the families whose whole head conditions on the query still have no bank
    with pytest.raises(ValueError, match="prototype-matching"):
        pemp_stage2.PEMPStage2(1, 1, None).eval().enroll(sup, msk)
    with pytest.raises(ValueError, match="prototype-matching"):
        canet.ModelClass(None).eval().enroll(sup, msk)


def test_test_bank_commands_are_registered():
    from pemp_amd.entry import baseline, panet, pemp_stage1, pfenet
    for entry in (pemp_stage1, baseline, panet, pfenet):
        assert "test_bank" in entry.ex.commands and "test" in entry.ex.commands
        with pytest.raises(ValueError, match="split"):
            entry.ex.run("test_bank")                          # split = -1: refused with test's own message, before any model
    assert set(pfenet.ex.cfg) == {"tag", "shot", "query", "split", "seed", "ckpt", "exp_id", "loss", "sigma", "loss_coef",
                                  "trunk_precision", "p"}      # no configuration key of its own
