"""The ragged tails, the parts that need no GPU: the host-side planner against its formula, the argument checks of the two C
entries, and the refusals of ``ops.eval_tail_ragged`` / ``ops.nway_tail_ragged`` / ``segment_labels`` that come before any
device work."""
import ctypes
import os

import pytest
import torch

from pemp_amd.bank import PrototypeBank

SIZES = [(1, 1), (32, 32), (25, 41), (263, 257), (520, 510)]
NBLK = [1, 1, 2, 67, 256]


def _items(sizes):
    from pemp_amd import _lib
    items = (_lib.TailItem * len(sizes))()
    for it, (ho, wo) in zip(items, sizes):
        it.Ho, it.Wo = ho, wo
    return items


def test_the_library_exports_the_three_symbols(hip_lib):
    from pemp_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "pemp_hip.h")).read()
    for name in ("pemp_tail_ragged_workspace_bytes", "pemp_eval_tail_ragged_f32", "pemp_nway_tail_ragged_f32"):
        assert name in _lib.SYMBOLS and getattr(hip_lib, name) is not None and name + "(" in header
    assert "} pemp_tail_item;" in header
    assert ctypes.sizeof(_lib.TailItem) == 24                      # int32 Ho, Wo, nblk, part_off; int64 pix_off
    assert hip_lib.pemp_abi_version() == 2                         # additions only


def test_planner_fills_the_planned_fields_by_the_formula(hip_lib):
    plan = hip_lib.pemp_tail_ragged_workspace_bytes
    items = _items(SIZES)
    nbytes = plan(items, len(SIZES))
    assert [it.nblk for it in items] == NBLK
    for it, (ho, wo) in zip(items, SIZES):                         # tail_blocks: ceil(Ho * Wo / 1024) in 1..256
        assert it.nblk == min(max(-(-ho * wo // 1024), 1), 256) and (it.Ho, it.Wo) == (ho, wo)
        assert it.nblk * 64 == hip_lib.pemp_eval_tail_workspace_bytes(1, ho, wo)
    pix = blk = 0
    for it, (ho, wo) in zip(items, SIZES):                         # running sums: pixels, and rows of partials
        assert (it.pix_off, it.part_off) == (pix, blk)
        pix, blk = pix + ho * wo, blk + it.nblk
    assert nbytes == sum(NBLK) * 8 * 8                             # [8] doubles per block, nothing between the images
    # the order is the caller's: permuted sizes give permuted block counts and their own running sums
    perm = [3, 0, 4, 2, 1]
    items = _items([SIZES[i] for i in perm])
    assert plan(items, 5) == nbytes and [it.nblk for it in items] == [NBLK[i] for i in perm]
    assert [it.pix_off for it in items] == [0, 263 * 257, 263 * 257 + 1, 263 * 257 + 1 + 520 * 510, 263 * 257 + 1 + 520 * 510 + 1025]
    # equal sizes: the fixed-size tail's workspace
    assert plan(_items([(401, 401)] * 3), 3) == hip_lib.pemp_eval_tail_workspace_bytes(3, 401, 401)


def test_planner_refuses_bad_items(hip_lib):
    plan, err = hip_lib.pemp_tail_ragged_workspace_bytes, hip_lib.pemp_last_error
    assert plan(None, 3) == 0 and b"bad arguments" in err()
    for n in (0, -1, 70000):
        assert plan(_items([(5, 5)]), n) == 0 and b"bad arguments" in err(), n
    for bad in ((0, 5), (5, 0), (-1, 5), (5, -3), (1 << 16, 1 << 16)):
        assert plan(_items([(5, 5), bad]), 2) == 0 and b"item 1 has the size" in err(), bad


def test_c_entries_validate_before_any_device_work(hip_lib):
    buf = (ctypes.c_float * 64)()                   # host memory: never dereferenced, only its address is looked at
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = hip_lib.pemp_last_error
    planned = _items([(5, 5), (401, 401)])
    need = hip_lib.pemp_tail_ragged_workspace_bytes(planned, 2)
    assert need == (1 + 158) * 64

    def ev(pred=p, target=None, items=planned, items_dev=p, B=2, h=2, w=2, out=p, stats=None, ws=p, ws_bytes=1 << 20):
        return hip_lib.pemp_eval_tail_ragged_f32(pred, target, items, items_dev, B, h, w, out, stats, ws, ws_bytes, None)

    def nw(pred=p, target=None, want=None, items=planned, items_dev=p, N=2, K=1, h=2, w=2, labels=p, margin=None, stats=None, ws=p,
           ws_bytes=1 << 20):
        return hip_lib.pemp_nway_tail_ragged_f32(pred, target, want, items, items_dev, N, K, h, w, labels, margin, stats, ws,
                                                 ws_bytes, None)
    for name in ("pred", "items", "items_dev", "out", "ws"):
        assert ev(**{name: None}) == -1 and b"eval_tail_ragged: null pointer" in err(), name
    for name in ("pred", "items", "items_dev", "labels", "ws"):
        assert nw(**{name: None}) == -1 and b"nway_tail_ragged: null pointer" in err(), name
    for kw in (dict(target=p), dict(stats=p)):
        assert ev(**kw) == -1 and b"come together" in err(), kw
    for kw in (dict(target=p), dict(want=p), dict(stats=p), dict(target=p, want=p), dict(target=p, stats=p), dict(want=p, stats=p)):
        assert nw(**kw) == -1 and b"come together" in err(), kw
    for kw in (dict(B=0), dict(B=-1), dict(B=70000), dict(h=0), dict(w=0)):
        assert ev(**kw) == -1 and b"bad dims" in err(), kw
    for kw in (dict(N=0), dict(N=-1), dict(N=70000), dict(K=0), dict(h=0), dict(w=0)):
        assert nw(**kw) == -1 and b"bad dims" in err(), kw
    assert nw(K=256) == -1 and b"K <= 255" in err()
    assert nw(K=256, target=p, want=p, stats=p) == -1 and b"K <= 255" in err()
    # an item with a size below 1, and items that did not go through the planner
    for bad in ((0, 5), (5, 0), (-2, 5)):
        items = _items([(5, 5), bad])
        assert ev(items=items) == -1 and b"item 1 has the size" in err(), bad
        assert nw(items=items) == -1 and b"item 1 has the size" in err(), bad
    raw = _items([(5, 5), (401, 401)])
    assert ev(items=raw) == -1 and b"item 0 was not planned" in err()
    assert nw(items=raw) == -1 and b"item 0 was not planned" in err()
    moved = _items([(5, 5), (401, 401)])
    hip_lib.pemp_tail_ragged_workspace_bytes(moved, 2)
    moved[1].pix_off += 1
    assert ev(items=moved) == -1 and b"item 1 was not planned" in err()
    # a workspace one byte short, with and without statistics
    for kw in (dict(), dict(target=p, stats=p)):
        assert ev(ws_bytes=need - 1, **kw) == -1 and b"workspace too small" in err(), kw
    for kw in (dict(), dict(target=p, want=p, stats=p)):
        assert nw(ws_bytes=need - 1, **kw) == -1 and b"workspace too small" in err(), kw
    assert ev(ws_bytes=0) == -1 and nw(ws_bytes=0) == -1 and b"workspace too small" in err()


def _tgt(*hw):
    return torch.zeros(*hw, dtype=torch.int64)


def test_eval_tail_ragged_refusals_need_no_gpu(hip_lib):
    from pemp_amd import _lib, ops
    pred = torch.zeros(2, 2, 3, 3)
    call = ops.eval_tail_ragged
    for bad in (torch.zeros(2, 3, 3), torch.zeros(2, 3, 3, 3), torch.zeros(2, 2, 3, 6)[..., ::2], pred.double(), torch.zeros(2, 1, 2, 3, 3)):
        with pytest.raises(ValueError, match="pred must be contiguous fp32"):
            call(bad, sizes=[(5, 5), (4, 6)])
    with pytest.raises(ValueError, match="either sizes or targets"):
        call(pred)
    with pytest.raises(ValueError, match="either sizes or targets"):
        call(pred, [_tgt(5, 5), _tgt(4, 6)], sizes=[(5, 5), (4, 6)])
    with pytest.raises(ValueError, match="1 sizes for 2 images"):
        call(pred, sizes=[(5, 5)])
    with pytest.raises(ValueError, match="3 targets for 2 images"):
        call(pred, [_tgt(5, 5)] * 3)
    for bad in (torch.zeros(5, 5, dtype=torch.int32), torch.zeros(5, 5), _tgt(2, 5, 5), _tgt(5), _tgt(1, 1, 5, 5)):
        with pytest.raises(ValueError, match="target 1 must be an int64 tensor"):
            call(pred, [_tgt(5, 5), bad])
    for bad in ((0, 5), (5, 0), (-1, 4)):
        with pytest.raises(ValueError, match="image 1 has the size"):
            call(pred, sizes=[(5, 5), bad])
    with pytest.raises(ValueError, match="image 0 has the size"):
        call(pred, [_tgt(0, 5), _tgt(5, 5)])
    with pytest.raises(ValueError, match="pair"):
        call(pred, sizes=[(5, 5), (5, 5, 5)])
    # the good calls reach the device check: there is no CPU path
    for kw in (dict(sizes=[(5, 5), (4, 6)]), dict(targets=[_tgt(5, 5), _tgt(1, 4, 6)])):
        with pytest.raises(_lib.PempHipError, match="no CPU path"):
            call(pred, **kw)


def test_nway_tail_ragged_refusals_need_no_gpu(hip_lib):
    from pemp_amd import _lib, ops
    pred = torch.zeros(2, 3, 2, 3, 3)
    call = ops.nway_tail_ragged
    for bad in (torch.zeros(2, 2, 3, 3), torch.zeros(2, 3, 3, 3, 3), torch.zeros(2, 3, 2, 3, 6)[..., ::2], pred.double()):
        with pytest.raises(ValueError, match="pred must be contiguous fp32"):
            call(bad, [(5, 5), (4, 6)])
    with pytest.raises(ValueError, match="K = 256"):
        call(torch.zeros(1, 256, 2, 1, 1), [(5, 5)])
    with pytest.raises(ValueError, match="either sizes or targets"):
        call(pred)
    with pytest.raises(ValueError, match="either sizes or targets"):
        call(pred, [(5, 5), (4, 6)], targets=[_tgt(5, 5), _tgt(4, 6)], want=[0, 1])
    with pytest.raises(ValueError, match="come together"):
        call(pred, targets=[_tgt(5, 5), _tgt(4, 6)])
    with pytest.raises(ValueError, match="come together"):
        call(pred, [(5, 5), (4, 6)], want=[0, 1])
    with pytest.raises(ValueError, match="index values"):
        call(pred, targets=[_tgt(5, 5), _tgt(4, 6)], want=[0, 3])                 # bank_index's check
    with pytest.raises(ValueError, match="1 entries for 2 queries"):
        call(pred, targets=[_tgt(5, 5), _tgt(4, 6)], want=[0])
    with pytest.raises(ValueError, match="3 sizes for 2 images"):
        call(pred, [(5, 5)] * 3)
    with pytest.raises(ValueError, match="1 targets for 2 images"):
        call(pred, targets=[_tgt(5, 5)], want=[0, 1])
    with pytest.raises(ValueError, match="target 0 must be an int64 tensor"):
        call(pred, targets=[torch.zeros(5, 5, dtype=torch.uint8), _tgt(4, 6)], want=[0, 1])
    with pytest.raises(ValueError, match="image 1 has the size"):
        call(pred, [(5, 5), (4, 0)])
    for kw in (dict(sizes=[(5, 5), (4, 6)]), dict(sizes=[(5, 5), (4, 6)], want_margin=True),
               dict(targets=[_tgt(5, 5), _tgt(1, 4, 6)], want=[2, 0])):
        with pytest.raises(_lib.PempHipError, match="no CPU path"):
            call(pred, **kw)


def test_segment_labels_refuses_a_wrong_number_of_shapes_without_a_gpu():
    from pemp_amd.networks import pemp_stage1
    net = pemp_stage1.PEMPStage1(None).eval()                # resnet50, protos = 3, c = 512
    q = torch.zeros(3, 3, 97, 97)
    bank = PrototypeBank(torch.zeros(2, 6, 512), family="pemp_stage1", backbone="resnet50", precision="f32", dist_scalar=20)
    for shapes in ([(50, 60)], [(50, 60), (40, 40)], [(50, 60)] * 4, [], [(50, 60), (40, 40), (0, 40)], [(50, 60), (40, 40), (30, 30, 30)]):
        for kw in (dict(), dict(want_margin=True), dict(graphed=True)):
            with pytest.raises(ValueError, match="segment_labels: out_shape"):
                net.segment_labels(bank, q, out_shape=shapes, **kw)
    # the right number reaches the device check, as a single pair (tuple, list or torch.Size) and None still do
    for shapes in ([(50, 60), (40, 40), (97, 97)], [[50, 60], [40, 40], torch.Size([97, 97])], (50, 60), [50, 60], torch.Size([50, 60]), None):
        with pytest.raises(RuntimeError, match="GPU"):
            net.segment_labels(bank, q, out_shape=shapes)


def test_the_evaluators_keep_one_copy_of_the_per_size_loop():
    """``PEMP_RAGGED_TAIL=0`` is served by ``ops.tail_rows`` alone: the evaluators hold no loop over label sizes."""
    import inspect
    from pemp_amd import ops
    from pemp_amd.entry import canet, pemp_stage1
    assert isinstance(ops.RAGGED_TAIL, bool)
    for mod in (canet, pemp_stage1):
        src = inspect.getsource(mod)
        assert "by_size" not in src and "index_select" not in src and "ops.tail_rows(" in src
    for cls in (pemp_stage1.Evaluator, pemp_stage1.BankEvaluator, pemp_stage1.NWayEvaluator, canet.Evaluator):
        assert not hasattr(cls, "_tail_by_size") and not hasattr(cls, "_nway_by_size")
    assert inspect.getsource(ops).count("by_size = {}") == 1
