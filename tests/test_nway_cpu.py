"""The N-way label map, the parts that need no GPU: the argument checks of the C entry, the refusals of ``segment_labels`` and the
``test_nway`` command's registration."""
import ctypes

import pytest
import torch

from pemp_amd.bank import PrototypeBank


def test_the_library_exports_both_symbols(hip_lib):
    from pemp_amd import _lib
    for name in ("pemp_nway_tail_workspace_bytes", "pemp_nway_tail_f32"):
        assert name in _lib.SYMBOLS and getattr(hip_lib, name) is not None
    text = open(util_header()).read()
    assert "size_t pemp_nway_tail_workspace_bytes(int N, int Ho, int Wo);" in text and "int pemp_nway_tail_f32(" in text
    # the partial sums of eval_tail: [N][blocks][8] doubles, blocks = ceil(Ho * Wo / 1024) capped at 256
    ws = hip_lib.pemp_nway_tail_workspace_bytes
    assert ws(1, 1, 1) == 64 and ws(3, 401, 401) == 3 * 158 * 64 and ws(1, 520, 521) == 256 * 64
    assert ws(3, 401, 401) == hip_lib.pemp_eval_tail_workspace_bytes(3, 401, 401)
    assert hip_lib.pemp_abi_version() == 2                          # additions only


def util_header():
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "pemp_hip.h")


def test_c_entry_validates_before_any_device_work(hip_lib):
    buf = (ctypes.c_float * 64)()                   # host memory: never dereferenced, only its address is looked at
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = hip_lib.pemp_last_error
    f = hip_lib.pemp_nway_tail_f32

    def call(pred=p, target=None, want=None, labels=p, margin=None, stats=None, ws=p, ws_bytes=1 << 20, N=1, K=1, h=2, w=2, Ho=5,
             Wo=5):
        return f(pred, target, want, labels, margin, stats, ws, ws_bytes, N, K, h, w, Ho, Wo, None)
    for name in ("pred", "labels", "ws"):
        assert call(**{name: None}) == -1 and b"null pointer" in err(), name
    for kw in (dict(target=p), dict(want=p), dict(stats=p), dict(target=p, want=p), dict(target=p, stats=p), dict(want=p, stats=p)):
        assert call(**kw) == -1 and b"come together" in err(), kw
    for kw in (dict(N=0), dict(K=0), dict(h=0), dict(w=0), dict(Ho=0), dict(Wo=0), dict(N=-1), dict(N=70000),
               dict(Ho=1 << 16, Wo=1 << 16)):
        assert call(**kw) == -1 and b"bad dims" in err(), kw
    assert call(K=256) == -1 and b"K <= 255" in err()
    assert call(K=256, target=p, want=p, stats=p) == -1 and b"K <= 255" in err()
    need = hip_lib.pemp_nway_tail_workspace_bytes(2, 401, 401)
    for kw in (dict(), dict(target=p, want=p, stats=p)):
        assert call(N=2, Ho=401, Wo=401, ws_bytes=need - 1, **kw) == -1 and b"workspace too small" in err(), kw
    assert call(ws_bytes=0) == -1 and b"workspace too small" in err()


def test_nway_tail_wrapper_refuses_host_tensors(hip_lib):
    from pemp_amd import _lib, ops
    with pytest.raises(_lib.PempHipError, match="no CPU path"):
        ops.nway_tail(torch.zeros(1, 2, 2, 3, 3), (5, 5))
    with pytest.raises(ValueError, match="K = 256"):
        ops.nway_tail(torch.zeros(1, 256, 2, 1, 1), (5, 5))
    with pytest.raises(ValueError, match="come together"):
        ops.nway_tail(torch.zeros(1, 2, 2, 3, 3), target=torch.zeros(1, 5, 5, dtype=torch.int64))
    with pytest.raises(ValueError, match="index values"):
        ops.nway_tail(torch.zeros(1, 2, 2, 3, 3), target=torch.zeros(1, 5, 5, dtype=torch.int64), want=[2])


def test_segment_labels_refusals_need_no_gpu():
    from pemp_amd.networks import canet, pemp_stage1, pemp_stage2
    net = pemp_stage1.PEMPStage1(None).eval()                # resnet50, protos = 3, c = 512
    q = torch.zeros(1, 3, 97, 97)
    mk = lambda k=2, **kw: PrototypeBank(torch.zeros(k, 6, 512), **{**dict(family="pemp_stage1", backbone="resnet50", precision="f32",
                                                                          dist_scalar=20), **kw})
    for kw in (dict(), dict(graphed=True), dict(want_margin=True), dict(out_shape=(50, 60))):
        with pytest.raises(RuntimeError, match="GPU"):
            net.segment_labels(mk(), q, **kw)                  # CPU inputs: no CPU path
    with pytest.raises(RuntimeError, match="eval"):
        pemp_stage1.PEMPStage1(None).train().segment_labels(mk(), q)
    # the existing checks of segment, under this call's name
    with pytest.raises(ValueError, match="segment_labels.*family = "):
        net.segment_labels(mk(family="baseline"), q)
    with pytest.raises(ValueError, match="qry_img"):
        net.segment_labels(mk(), q[None])
    with pytest.raises(TypeError):
        net.segment_labels(torch.zeros(2, 6, 512), q)
    # uint8 labels with 0 for no class: 255 classes at the most, refused before the device check
    with pytest.raises(ValueError, match="256 classes"):
        net.segment_labels(mk(256), q)
    with pytest.raises(RuntimeError, match="GPU"):
        net.segment_labels(mk(255), q)
    # the families whose whole head conditions on the query still have no bank
    with pytest.raises(ValueError, match="prototype-matching"):
        pemp_stage2.PEMPStage2(1, 1, None).eval().segment_labels(mk(), q)
    with pytest.raises(ValueError, match="prototype-matching"):
        canet.ModelClass(None).eval().segment_labels(mk(), q)


def test_test_nway_commands_are_registered():
    from pemp_amd.entry import baseline, panet, pemp_stage1, pfenet, rpmms
    for entry in (pemp_stage1, baseline, panet, pfenet, rpmms):
        assert {"test_nway", "test_bank", "test"} <= set(entry.ex.commands)
        with pytest.raises(ValueError, match="Argument `split` is required"):
            entry.ex.run("test_nway")                          # split = -1: refused with test's own message, before any model
    # the evaluators: the mixin in front of each entry's own BankEvaluator, so RPMMs keeps its _enroll
    assert pemp_stage1.NWayEvaluator.__mro__[1:3] == (pemp_stage1.NWayMixin, pemp_stage1.BankEvaluator)
    assert rpmms.NWayEvaluator.__mro__[1:3] == (pemp_stage1.NWayMixin, rpmms.BankEvaluator)
    assert rpmms.NWayEvaluator._enroll is rpmms.BankEvaluator._enroll
    assert rpmms.NWayEvaluator._episodes is pemp_stage1.NWayMixin._episodes


def test_a_round_that_misses_a_class_is_refused_before_any_query():
    """The walk enrolls first and raises when a validation class never occurs; nothing is segmented."""
    from pemp_amd.entry import pemp_stage1 as e

    class Ev(e.NWayEvaluator):
        def __init__(self):                                  # no model, no device: the walk alone
            self._labels, self.splitk, self.enrolled = [1, 2, 3, 4, 5], None, []

        def _enroll(self, slot, cls, sup_img, sup_mask):
            self.enrolled.append((slot, cls))

    class Data:
        def __init__(self, classes):
            self.classes = classes

        def __len__(self):
            return len(self.classes)

        def task(self, i):
            return (f"sup{i}", f"msk{i}", f"qry{i}"), f"lab{i}", torch.tensor([self.classes[i]])
    ev = Ev()
    with pytest.raises(ValueError, match=r"validation classes \[3, 5\]"):
        next(ev._episodes(Data([1, 2, 2, 4, 1]), range(5)))
    assert ev.enrolled == [(0, 1), (1, 2), (3, 4)]
    ev = Ev()
    got = list(ev._episodes(Data([2, 2, 1, 3, 5, 4, 1, 3]), range(1, 8, 2)))         # a rank's shard
    assert ev.enrolled == [(1, 2), (0, 1), (2, 3), (4, 5), (3, 4)]                     # first tasks, in the walk's order
    assert [(g[0], g[1], int(g[2])) for g in got] == [(("qry1", 1), "lab1", 2), (("qry3", 2), "lab3", 3), (("qry5", 3), "lab5", 4),
                                                      (("qry7", 2), "lab7", 3)]
    with pytest.raises(ValueError, match="not a validation class"):
        next(Ev()._episodes(Data([1, 9]), range(2)))
