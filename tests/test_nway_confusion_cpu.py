"""The N-way confusion tail, the parts that need no GPU: the argument checks of the two C entries, the refusals of the wrappers and
of ``segment_confusion``, ``SemanticMetric`` against hand-written tables, ``slot_targets`` and the ``test_semantic`` commands."""
import ctypes
import os

import numpy as np
import pytest
import torch

from pemp_amd.bank import PrototypeBank


def test_the_library_exports_the_symbols(hip_lib):
    from pemp_amd import _lib
    for name in ("pemp_nway_confusion_workspace_bytes", "pemp_nway_confusion_f32", "pemp_nway_confusion_ragged_f32"):
        assert name in _lib.SYMBOLS and getattr(hip_lib, name) is not None
    header = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "pemp_hip.h")
    text = open(header).read()
    assert "size_t pemp_nway_confusion_workspace_bytes(int N, int K, int Ho, int Wo);" in text
    assert "int pemp_nway_confusion_f32(" in text and "int pemp_nway_confusion_ragged_f32(" in text
    # the blocks flush with integer atomics: no workspace at any size
    assert hip_lib.pemp_nway_confusion_workspace_bytes(25, 63, 513, 513) == 0
    assert hip_lib.pemp_abi_version() == 2                          # additions only


def test_c_entries_validate_before_any_device_work(hip_lib):
    from pemp_amd import _lib
    buf = (ctypes.c_float * 64)()                   # host memory: never dereferenced, only its address is looked at
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = hip_lib.pemp_last_error

    def fixed(pred=p, target=p, want=None, labels=None, conf=p, N=1, K=1, h=2, w=2, Ho=5, Wo=5):
        return hip_lib.pemp_nway_confusion_f32(pred, target, want, labels, conf, None, 0, N, K, h, w, Ho, Wo, None)
    for name in ("pred", "target", "conf"):
        assert fixed(**{name: None}) == -1 and b"null pointer" in err(), name
    for kw in (dict(N=0), dict(K=0), dict(h=0), dict(w=0), dict(Ho=0), dict(Wo=0), dict(N=-1), dict(N=70000),
               dict(Ho=1 << 16, Wo=1 << 16), dict(h=1 << 15, w=1 << 15)):
        assert fixed(**kw) == -1 and b"bad dims" in err(), kw
    for kw in (dict(K=64), dict(K=64, want=p, labels=p), dict(K=255)):
        assert fixed(**kw) == -1 and b"K <= 63" in err(), kw

    items = (_lib.TailItem * 2)()
    for it, (ho, wo) in zip(items, ((5, 5), (40, 24))):
        it.Ho, it.Wo = ho, wo
    assert hip_lib.pemp_tail_ragged_workspace_bytes(items, 2) > 0

    def ragged(pred=p, target=p, want=None, items_host=items, items_dev=p, N=2, K=1, h=2, w=2, labels=None, conf=p):
        return hip_lib.pemp_nway_confusion_ragged_f32(pred, target, want, items_host, items_dev, N, K, h, w, labels, conf, None, 0,
                                                      None)
    for name in ("pred", "target", "items_host", "items_dev", "conf"):
        assert ragged(**{name: None}) == -1 and b"null pointer" in err(), name
    for kw in (dict(N=0), dict(N=70000), dict(K=0), dict(h=0), dict(w=0)):
        assert ragged(**kw) == -1 and b"bad dims" in err(), kw
    assert ragged(K=64) == -1 and b"K <= 63" in err()
    fresh = (_lib.TailItem * 2)()                   # sizes filled in, never planned
    for it, (ho, wo) in zip(fresh, ((5, 5), (40, 24))):
        it.Ho, it.Wo = ho, wo
    assert ragged(items_host=fresh) == -1 and b"was not planned" in err()
    fresh[0].Ho = 0
    assert ragged(items_host=fresh) == -1 and b"has the size" in err()


def test_wrappers_refuse_on_the_host(hip_lib):
    from pemp_amd import _lib, ops
    pred = torch.zeros(2, 3, 2, 4, 4)
    tgt = torch.zeros(2, 9, 9, dtype=torch.int64)
    lst = [torch.zeros(9, 9, dtype=torch.int64), torch.zeros(1, 5, 7, dtype=torch.int64)]
    assert ops.CONFUSION_MAX_K == 63
    for call, good in ((ops.nway_confusion, tgt), (ops.nway_confusion_ragged, lst)):
        name = call.__name__
        with pytest.raises(ValueError, match=f"{name}: K = 64"):
            call(torch.zeros(2, 64, 2, 1, 1), good)
        for bad in (pred[0], pred.double(), pred.transpose(3, 4), torch.zeros(2, 3, 3, 4, 4), pred[:, :, :1]):
            with pytest.raises(ValueError, match=f"{name}: pred"):
                call(bad, good)
        # want: checked like nway_tail's, values outside 0..K-1 included
        for want in ([0, 3], [-1, 0], torch.tensor([0, 3]), [0], [0.5, 1], torch.zeros(2, 1, dtype=torch.int64)):
            with pytest.raises(ValueError):
                call(pred, good, want=want)
        # everything in order but the device: no CPU path (a RuntimeError)
        for want in (None, [2, 0]):
            with pytest.raises(_lib.PempHipError, match="no CPU path"):
                call(pred, good, want=want)
        assert issubclass(_lib.PempHipError, RuntimeError)
    for bad in (tgt.int(), tgt[:1], tgt.transpose(1, 2)[:, :, :8], tgt[0], None, lst):
        with pytest.raises(ValueError, match="nway_confusion: target"):
            ops.nway_confusion(pred, bad)
    for bad in (lst[:1], [lst[0], lst[1].int()], [lst[0], torch.zeros(2, 5, 7, dtype=torch.int64)], [lst[0], None], None):
        with pytest.raises(ValueError, match="nway_confusion_ragged"):
            ops.nway_confusion_ragged(pred, bad)


def test_segment_confusion_refusals_need_no_gpu():
    from pemp_amd.networks import canet, pemp_stage1, pemp_stage2
    net = pemp_stage1.PEMPStage1(None).eval()                # resnet50, protos = 3, c = 512
    q = torch.zeros(2, 3, 97, 97)
    tgt = torch.zeros(2, 97, 97, dtype=torch.int64)
    mk = lambda k=2, **kw: PrototypeBank(torch.zeros(k, 6, 512), **{**dict(family="pemp_stage1", backbone="resnet50", precision="f32",
                                                                          dist_scalar=20), **kw})
    for kw in (dict(), dict(graphed=True), dict(want_labels=True), dict(want=[1, 0])):
        with pytest.raises(RuntimeError, match="GPU"):
            net.segment_confusion(mk(), q, tgt, **kw)          # CPU inputs: no CPU path
    with pytest.raises(RuntimeError, match="GPU"):
        net.segment_confusion(mk(), q, [tgt[0], tgt[1, :50, :60]])
    with pytest.raises(RuntimeError, match="eval"):
        pemp_stage1.PEMPStage1(None).train().segment_confusion(mk(), q, tgt)
    # the existing checks of segment, under this call's name
    with pytest.raises(ValueError, match="segment_confusion.*family = "):
        net.segment_confusion(mk(family="baseline"), q, tgt)
    with pytest.raises(ValueError, match="qry_img"):
        net.segment_confusion(mk(), q[None], tgt)
    with pytest.raises(TypeError):
        net.segment_confusion(torch.zeros(2, 6, 512), q, tgt)
    # 4096 bins at the most, refused before the device check
    with pytest.raises(ValueError, match="64 classes"):
        net.segment_confusion(mk(64), q, tgt)
    with pytest.raises(RuntimeError, match="GPU"):
        net.segment_confusion(mk(63), q, tgt)
    for bad in (tgt.int(), tgt[:1], tgt[0], [tgt[0]]):
        with pytest.raises(ValueError, match="segment_confusion.*target"):
            net.segment_confusion(mk(), q, bad)
    for want in ([0, 2], [0], [-1, 0], [0.5, 1]):
        with pytest.raises(ValueError):
            net.segment_confusion(mk(), q, tgt, want=want)
    # the families whose whole head conditions on the query still have no bank
    with pytest.raises(ValueError, match="prototype-matching"):
        pemp_stage2.PEMPStage2(1, 1, None).eval().segment_confusion(mk(), q, tgt)
    with pytest.raises(ValueError, match="prototype-matching"):
        canet.ModelClass(None).eval().segment_confusion(mk(), q, tgt)


def test_semantic_metric_against_hand_written_tables():
    from pemp_amd.core.metrics import SemanticMetric
    m = SemanticMetric(3)
    #            p = 0  1  2  3
    a = np.array([[50, 2, 0, 0],         # t = 0
                  [3, 10, 1, 0],         # t = 1
                  [0, 4, 6, 0],          # t = 2
                  [0, 0, 0, 0]])         # t = 3: never a target and never predicted -> empty union
    m.update(a)
    iou = m.iou()
    # diag / (row + col - diag)
    want = [50 / (52 + 53 - 50), 10 / (14 + 16 - 10), 6 / (10 + 7 - 6)]
    assert np.allclose(iou[:3], want, rtol=0, atol=1e-15) and np.isnan(iou[3])
    r = m.result()
    assert r["mIoU"] == pytest.approx((want[1] + want[2]) / 2, abs=1e-15)            # class 3 left out, not counted as 0
    assert r["mIoU_bg"] == pytest.approx(sum(want) / 3, abs=1e-15)
    assert r["pixAcc"] == pytest.approx(66 / 76, abs=1e-15) and np.array_equal(r["iou"], iou, equal_nan=True)
    # tables add: a stack, a torch tensor, and the class that was empty shows up
    b = np.zeros((4, 4), np.int64)
    b[3, 3], b[0, 3] = 5, 5
    m.update(torch.from_numpy(np.stack([b, a])))
    assert np.array_equal(m.conf, 2 * a + b)
    assert m.iou()[3] == 0.5 and m.result()["mIoU"] == pytest.approx((want[1] + want[2] + 0.5) / 3, abs=1e-15)
    # nothing counted at all
    r0 = SemanticMetric(2).result()
    assert all(np.isnan(r0[k]) for k in ("mIoU", "mIoU_bg", "pixAcc")) and np.isnan(r0["iou"]).all()
    for bad in (np.zeros((3, 3), np.int64), np.zeros((4, 4))):
        with pytest.raises(ValueError, match="SemanticMetric"):
            m.update(bad)


def test_slot_targets_on_a_hand_made_id_map():
    from pemp_amd import ops
    ids = torch.tensor([[0, 7, 9, 255], [12, 9, 3, 0]], dtype=torch.uint8)
    want = torch.tensor([[0, 2, 1, 255], [0, 1, 0, 0]])                # bank slots: 9 -> 1, 7 -> 2; 12 and 3 are not enrolled
    got = ops.slot_targets(ids, [9, 7])
    assert got.dtype == torch.int64 and torch.equal(got, want)
    assert torch.equal(ops.slot_targets(ids.long(), (9, 7)), want) and torch.equal(ops.slot_targets(ids.int(), [9, 7]), want)
    assert torch.equal(ops.slot_targets(ids, []), torch.where(ids == 255, 255, 0))
    for bad in ([9, 9], [0, 7], [255], [7.5], [300]):
        with pytest.raises(ValueError, match="bank_labels"):
            ops.slot_targets(ids, bad)
    with pytest.raises(ValueError, match="target_ids"):
        ops.slot_targets(ids.float(), [9, 7])


def test_test_semantic_commands_are_registered():
    from pemp_amd.entry import baseline, panet, pemp_stage1, pfenet, rpmms
    for entry in (pemp_stage1, baseline, panet, pfenet, rpmms):
        assert {"test_semantic", "test_nway", "test_bank", "test"} <= set(entry.ex.commands)
        with pytest.raises(ValueError, match="Argument `split` is required"):
            entry.ex.run("test_semantic")                      # split = -1: refused with test's own message, before any model
    e = pemp_stage1
    assert e.SemanticEvaluator.__mro__[1:4] == (e.SemanticMixin, e.NWayMixin, e.BankEvaluator)
    assert rpmms.SemanticEvaluator.__mro__[1:4] == (e.SemanticMixin, e.NWayMixin, rpmms.BankEvaluator)
    assert rpmms.SemanticEvaluator._enroll is rpmms.BankEvaluator._enroll
    assert e.SemanticEvaluator._episodes is e.NWayMixin._episodes
