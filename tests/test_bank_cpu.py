"""Prototype banks, the parts that need no GPU: argument checks of ops.cosine_bank_max and of the C entry, the PrototypeBank
container, the refusal of a mismatching bank, the test_bank commands."""
import ctypes
import io

import pytest
import torch

from pemp_amd import _lib, ops
from pemp_amd.bank import PrototypeBank


@pytest.fixture
def no_library(monkeypatch):
    """The checks under test come before the library is touched."""
    def load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", load)


def _feat(n=3, h=2, w=2, c=64):
    return torch.zeros(n, h, w, c)


def test_cosine_bank_max_refuses_bad_banks(no_library):
    q = _feat()
    for bad in (torch.zeros(6, 64), torch.zeros(2, 3, 64), torch.zeros(2, 6, 64, dtype=torch.float64),
                torch.zeros(2, 6, 128)[:, :, ::2], torch.zeros(0, 6, 64)):
        with pytest.raises(ValueError, match=r"bank must be contiguous fp32 \[K,2p,c\]"):
            ops.cosine_bank_max(q, bad, 20.0)
    with pytest.raises(ValueError, match="bank has c = 128, the features have c = 64"):
        ops.cosine_bank_max(q, torch.zeros(2, 6, 128), 20.0)


def test_cosine_bank_max_checks_the_index_on_the_host(no_library):
    q, bank = _feat(n=3), torch.zeros(4, 6, 64)
    for bad in ([0, 1], [0, 1, 2, 3], torch.tensor([0, 1]), torch.zeros(3, 1, dtype=torch.int64)):
        with pytest.raises(ValueError, match="index"):
            ops.cosine_bank_max(q, bank, 20.0, index=bad)
    for bad in ([0, -1, 2], [0, 4, 2], torch.tensor([0, 1, 4]), torch.tensor([-1, 0, 0], dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"index values must lie in 0\.\.3"):
            ops.cosine_bank_max(q, bank, 20.0, index=bad)
    with pytest.raises(ValueError, match="integers"):
        ops.cosine_bank_max(q, bank, 20.0, index=[0, 1.5, 2])
    with pytest.raises(ValueError, match="integers"):
        ops.cosine_bank_max(q, bank, 20.0, index=torch.tensor([0.0, 1.0, 2.0]))
    # a tensor that is not in host memory cannot be checked without a synchronisation: refused whatever it holds
    with pytest.raises(ValueError, match="CPU tensor"):
        ops.cosine_bank_max(q, bank, 20.0, index=torch.zeros(3, dtype=torch.int32, device="meta"))
    idx = ops.bank_index((2, 0, 3), 3, 4)
    assert idx.dtype == torch.int32 and idx.tolist() == [2, 0, 3] and not idx.is_cuda


def test_c_entry_validates_before_any_device_work(hip_lib):
    f = hip_lib.pemp_cosine_bank_max_f32
    buf = (ctypes.c_float * 64)()                   # host memory: never dereferenced, only its address is looked at
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert f(None, 64, p, None, p, None, 1, 1, 4, 64, 3, 20.0, None) == -1 and b"null pointer" in hip_lib.pemp_last_error()
    assert f(p, 64, None, None, p, None, 1, 1, 4, 64, 3, 20.0, None) == -1 and b"null pointer" in hip_lib.pemp_last_error()
    assert f(p, 64, p, None, None, None, 1, 1, 4, 64, 3, 20.0, None) == -1 and b"null pointer" in hip_lib.pemp_last_error()
    for N, K, n, c, pp, ldf in ((0, 1, 4, 64, 3, 64), (1, 0, 4, 64, 3, 64), (1, 1, 0, 64, 3, 64), (1, 1, 4, 64, 0, 64),
                                (1, 1, 4, 64, 9, 64)):
        assert f(p, ldf, p, None, p, None, N, K, n, c, pp, 20.0, None) == -1 and b"bad dims" in hip_lib.pemp_last_error()
    for c, ldf in ((62, 64), (576, 576), (64, 32), (64, 66)):
        assert f(p, ldf, p, None, p, None, 1, 1, 4, c, 3, 20.0, None) == -1 and b"multiple of 4" in hip_lib.pemp_last_error()
    assert f(p, 64, p, None, p, None, 70000, 1, 4, 64, 3, 20.0, None) == -1 and b"65535" in hip_lib.pemp_last_error()
    off = ctypes.c_void_p(p.value + 4)
    assert f(off, 64, p, None, p, None, 1, 1, 4, 64, 3, 20.0, None) == -1 and b"16-byte aligned" in hip_lib.pemp_last_error()
    assert hip_lib.pemp_abi_version() == 2


def _bank(k=3, p=3, c=8, labels=(1, 2, 3), seed=0):
    g = torch.Generator().manual_seed(seed)
    return PrototypeBank(torch.randn(k, 2 * p, c, generator=g), "pemp_stage1", "resnet50", "f32", 20, labels=labels)


def test_prototype_bank_round_trip_and_in_place_update():
    bank = _bank()
    assert len(bank) == 3 and (bank.p, bank.c, bank.dist_scalar) == (3, 8, 20.0) and bank.labels == [1, 2, 3]
    sd = bank.state_dict()
    assert all(isinstance(v, (torch.Tensor, int, float, str, list, type(None))) for v in sd.values())
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    loaded = torch.load(buf, weights_only=True)
    other = _bank(seed=1, labels=None)
    ptr = other.protos.data_ptr()
    other.load_state_dict(loaded)
    assert other.protos.data_ptr() == ptr and torch.equal(other.protos, bank.protos) and other.labels == [1, 2, 3]
    again = PrototypeBank.from_state_dict(loaded)
    assert torch.equal(again.protos, bank.protos) and again.state_dict().keys() == sd.keys()
    for f in ("family", "backbone", "precision", "p", "c", "dist_scalar", "labels"):
        assert getattr(again, f) == getattr(bank, f) == getattr(other, f)
    assert bank.to("cpu") is bank
    # update copies into the bank's own storage
    ptr = bank.protos.data_ptr()
    one = _bank(k=1, labels=(9,), seed=2)
    assert bank.update(1, one) is bank
    assert bank.protos.data_ptr() == ptr and torch.equal(bank.protos[1], one.protos[0]) and bank.labels == [1, 9, 3]
    assert torch.equal(bank.protos[0], again.protos[0]) and torch.equal(bank.protos[2], again.protos[2])
    row = torch.ones(6, 8)
    bank.update(2, row)
    assert bank.protos.data_ptr() == ptr and torch.equal(bank.protos[2], row) and bank.labels == [1, 9, 3]
    with pytest.raises(IndexError):
        bank.update(3, row)
    with pytest.raises(ValueError):
        bank.update(0, torch.ones(4, 8))
    with pytest.raises(ValueError, match="mismatch in family"):
        bank.update(0, PrototypeBank(torch.zeros(1, 6, 8), "baseline", "resnet50", "f32", 20))
    with pytest.raises(ValueError, match="one class"):
        bank.update(0, _bank(k=2, labels=None))
    with pytest.raises(ValueError):
        other.load_state_dict(_bank(k=2, labels=None).state_dict())
    with pytest.raises(ValueError):
        PrototypeBank(torch.zeros(2, 3, 8), "baseline", "vgg16", "f32", 20)
    with pytest.raises(ValueError):
        _bank(labels=(1, 2))


def test_segment_refuses_a_mismatching_bank():
    from pemp_amd.networks import baseline, panet, pemp_stage1
    net = pemp_stage1.PEMPStage1(None).eval()                # resnet50, protos = 3, c = 512
    q = torch.zeros(1, 3, 97, 97)
    good = dict(family="pemp_stage1", backbone="resnet50", precision="f32", dist_scalar=20)
    mk = lambda p=3, c=512, **kw: PrototypeBank(torch.zeros(2, 2 * p, c), **{**good, **kw})
    for bank, field in ((mk(family="baseline"), "family"), (mk(backbone="vgg16"), "backbone"), (mk(precision="bf16"), "precision"),
                        (mk(p=1), "p"), (mk(c=256), "c"), (mk(dist_scalar=10), "dist_scalar")):
        for call in (net.segment, net.segment_lowres, net.segment_graphed):
            with pytest.raises(ValueError, match=f"{field} = "):
                call(bank, q)
    with pytest.raises(TypeError):
        net.segment(torch.zeros(2, 6, 512), q)
    # a matching bank gets as far as the device check, and a bad index is refused before it
    with pytest.raises(ValueError, match="index values"):
        net.segment(mk(), q, index=[2])
    with pytest.raises(RuntimeError, match="GPU"):
        net.segment(mk(), q, index=[1])
    with pytest.raises(RuntimeError, match="eval"):
        pemp_stage1.PEMPStage1(None).train().segment(mk(), q)
    # Baseline / PANet: their own families, no response map
    b, pa = baseline.Baseline(None).eval(), panet.PANet(None).eval()
    bb = PrototypeBank(torch.zeros(2, 2, 512), "baseline", "vgg16", "f32", 20)
    with pytest.raises(ValueError, match="family"):
        pa.segment(bb, q)
    with pytest.raises(ValueError, match="ret_ind"):
        b.segment(bb, q, ret_ind=True)
    with pytest.raises(RuntimeError, match="GPU"):
        b.segment(bb, q)
    with pytest.raises(ValueError, match="family"):
        b.enroll(torch.zeros(2, 1, 3, 97, 97), torch.zeros(2, 1, 2, 97, 97), out=mk())


_KEYS = {"tag", "shot", "query", "split", "seed", "ckpt", "exp_id", "loss", "sigma"}


def test_test_bank_command_is_registered_and_adds_no_config_key():
    from pemp_amd.entry import baseline, panet, pemp_stage1
    for entry, extra in ((pemp_stage1, {"p"}), (baseline, set()), (panet, {"loss_coef", "p"})):
        assert "test_bank" in entry.ex.commands and "test" in entry.ex.commands
        assert set(entry.ex.cfg) == _KEYS | extra
        assert {i.name for i in entry.ex.ingredients} == {"net", "data", "tr", "te", "g", "d"}
        with pytest.raises(ValueError, match="split"):
            entry.ex.run("test_bank")                          # split = -1: refused with test's own message, before any model
    assert issubclass(pemp_stage1.BankEvaluator, pemp_stage1.Evaluator)


def test_synthetic_round_of_twelve_covers_every_validation_class():
    """What tests/test_bank_eval_gpu.py relies on: its 12-episode round (seed 5678, split 0) holds every validation class."""
    from pemp_amd.entry import pemp_stage1 as e
    data = e.SyntheticEpisodes(12, 5678, 1, split=0, height=33, width=33)
    data.reset_sampler()
    data.sample_tasks()
    assert {int(data.task(i)[2]) for i in range(12)} == set(e.get_val_labels(0))
