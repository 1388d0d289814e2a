"""``ops.nway_confusion`` / ``ops.nway_confusion_ragged``: the label map of ``ops.nway_tail`` counted against a target.  The
reference is ``torch.bincount`` on the CPU over (target, labels of ``ops.nway_tail``); every comparison is exact integer
equality.  The logits are small integers (tests/test_nway_ops_gpu.py::_int_logits), so that ties between classes occur."""
import pytest
import torch

from tests.test_nway_ops_gpu import _int_logits

pytestmark = pytest.mark.gpu

#: (N, K, h, w, Ho, Wo)
SHAPES = [(2, 1, 3, 5, 7, 9),
          (3, 3, 4, 4, 33, 33),            # 1089 pixels: two blocks, 1024 + 65
          (2, 5, 13, 13, 97, 97),
          (1, 20, 5, 5, 40, 24),
          (1, 63, 3, 3, 17, 19)]           # 4096 bins
_IDS = ["x".join(str(v) for v in s) for s in SHAPES]
RAGGED_SIZES = [(1, 1), (7, 9), (33, 33), (513, 513), (40, 24)]


def bincount_tables(target, labels, K):
    """conf [N,K+1,K+1] on the CPU: pixels per (target class, label), targets outside 0..K left out."""
    out = []
    for t, p in zip(target.cpu().flatten(1), labels.cpu().flatten(1).long()):
        keep = (t >= 0) & (t <= K)
        out.append(torch.bincount(t[keep] * (K + 1) + p[keep], minlength=(K + 1) ** 2).view(K + 1, K + 1))
    return torch.stack(out)


_CASES = {}


@pytest.fixture
def case(hip_lib, dev, request):
    """Per shape, computed once and left unchanged: integer logits, a target in 0..K with some 255, a binary target with some 255,
    wanted slots, ``nway_tail``'s labels and the CPU tables."""
    from pemp_amd import ops
    shape = request.param
    if shape not in _CASES:
        N, K, h, w, Ho, Wo = shape
        g = torch.Generator().manual_seed(2000 + sum(shape))
        pred = _int_logits((N, K, 2, h, w), g).to(dev)
        target = torch.randint(0, K + 1, (N, Ho, Wo), generator=g)
        target[torch.rand((N, Ho, Wo), generator=g) < 0.1] = 255
        binary = torch.randint(0, 2, (N, Ho, Wo), generator=g)
        binary[torch.rand((N, Ho, Wo), generator=g) < 0.1] = 255
        want = torch.randint(0, K, (N,), generator=g)
        labels = ops.nway_tail(pred, (Ho, Wo))[0]
        _CASES[shape] = dict(shape=shape, pred=pred, target=target.to(dev), binary=binary.to(dev), want=want, labels=labels,
                             conf=bincount_tables(target, labels, K))
    return _CASES[shape]


@pytest.fixture(scope="module", autouse=True)
def _drop_cases():
    yield
    _CASES.clear()


@pytest.mark.parametrize("case", SHAPES, ids=_IDS, indirect=True)
def test_conf_is_the_bincount_of_target_and_nway_tail_labels(case, dev):
    from pemp_amd import ops
    N, K, h, w, Ho, Wo = case["shape"]
    conf, none = ops.nway_confusion(case["pred"], case["target"])
    assert none is None and conf.dtype == torch.int64 and conf.shape == (N, K + 1, K + 1) and conf.device.type == "cuda"
    assert torch.equal(conf.cpu(), case["conf"]), (conf.cpu() - case["conf"]).abs().sum().item()
    counted = (case["target"] != 255).flatten(1).sum(1)
    assert torch.equal(conf.sum(dim=(1, 2)), counted)
    # with the labels: nway_tail's bit for bit, and the same table
    conf2, labels = ops.nway_confusion(case["pred"], case["target"], want_labels=True)
    assert labels.dtype == torch.uint8 and torch.equal(labels, case["labels"]) and torch.equal(conf2, conf)
    # the case is no trivial one: every target class and every label occurs
    if case["shape"] == SHAPES[2]:
        assert (case["conf"].sum(0) > 0).all() and (case["conf"].sum(1) > 0).all()


@pytest.mark.parametrize("case", SHAPES, ids=_IDS, indirect=True)
def test_lifted_mode_recovers_the_rows_of_nway_tail(case, dev):
    from pemp_amd import ops
    N, K, h, w, Ho, Wo = case["shape"]
    pred, binary, want = case["pred"], case["binary"], case["want"]
    _, _, stats = ops.nway_tail(pred, target=binary, want=want)
    stats = stats.cpu()
    for w2 in (want, want.tolist(), want.to(torch.int32).to(dev)):
        conf, labels = ops.nway_confusion(pred, binary, want=w2, want_labels=True)
        assert torch.equal(labels, case["labels"])
        conf = conf.cpu()
        for n in range(N):
            c, s = conf[n], int(want[n]) + 1
            # the lifted target only has the rows 0 and want + 1
            assert int(c.sum()) == int(c[0].sum() + c[s].sum())
            n_valid = c.sum()
            tp_fg = c[s, s]
            fp_fg = c[:, s].sum() - tp_fg
            fn_fg = c[s].sum() - tp_fg
            # the binary image [label == want + 1]: its background is every other label
            tp_bg = c[0].sum() - c[0, s]
            fp_bg = c[s].sum() - c[s, s]                     # predicted not-s on a target of s
            fn_bg = c[0, s]                                  # predicted s on a background target
            row = torch.stack([n_valid, tp_bg, fp_bg, fn_bg, tp_fg, fp_fg, fn_fg]).double()
            assert torch.equal(row, stats[n, 1:]), (n, row.tolist(), stats[n].tolist())
    # the same table from the target lifted by hand
    lifted = torch.where(binary == 1, (want.to(dev) + 1).view(N, 1, 1), binary)
    assert torch.equal(ops.nway_confusion(pred, lifted)[0].cpu(), conf)


def test_ignored_values_never_reach_the_table(hip_lib, dev):
    from pemp_amd import ops
    N, K, h, w, Ho, Wo = 2, 3, 4, 4, 33, 33
    g = torch.Generator().manual_seed(11)
    pred = _int_logits((N, K, 2, h, w), g).to(dev)
    target = torch.randint(0, K + 1, (N, Ho, Wo), generator=g)
    hole = torch.rand((N, Ho, Wo), generator=g) < 0.3
    target[hole] = 255
    base = ops.nway_confusion(pred, target.to(dev))[0]
    assert int(base.sum()) == int((~hole).sum()) and int(hole.sum()) > 0
    for other in (254, K + 1, -1, -255, 1 << 32, (1 << 32) + 1, -(1 << 40)):       # the last three: no truncation to 32 bits
        t2 = target.clone()
        t2[hole] = other
        assert torch.equal(ops.nway_confusion(pred, t2.to(dev))[0], base), other
    zero = ops.nway_confusion(pred, torch.full((N, Ho, Wo), 255, dtype=torch.int64, device=dev))[0]
    assert zero.shape == (N, K + 1, K + 1) and not zero.any()
    # lifted: anything but 0 / 1 is ignored, 255 among them
    binary = torch.randint(0, 2, (N, Ho, Wo), generator=g)
    b255 = binary.clone()
    b255[hole] = 255
    lifted = ops.nway_confusion(pred, b255.to(dev), want=[2, 0])[0]
    assert int(lifted.sum()) == int((~hole).sum())
    for other in (254, 2, -1):
        b2 = binary.clone()
        b2[hole] = other
        assert torch.equal(ops.nway_confusion(pred, b2.to(dev), want=[2, 0])[0], lifted), other
    assert not ops.nway_confusion(pred, torch.full((N, Ho, Wo), 255, dtype=torch.int64, device=dev), want=[2, 0])[0].any()


def test_one_hot_bin(hip_lib, dev):
    """513 x 513 = 263169 pixels, more than the 256 blocks x 1024 of a full grid: the cap of 256 blocks binds and some threads
    walk a fifth pixel.  All pixels in one bin: the register count of (0,0), then the worst case of the LDS atomics."""
    from pemp_amd import ops
    K, h, w, S = 3, 5, 5, 513
    # background logit above foreground in every class: nobody claims
    pred = torch.stack([torch.ones(1, K, h, w), torch.zeros(1, K, h, w)], 2).contiguous().to(dev)
    conf, labels = ops.nway_confusion(pred, torch.zeros(1, S, S, dtype=torch.int64, device=dev), want_labels=True)
    want = torch.zeros(1, K + 1, K + 1, dtype=torch.int64)
    want[0, 0, 0] = 263169
    assert S * S == 263169 and torch.equal(conf.cpu(), want) and not labels.any()
    # class 2 (slot 1) claims by the largest margin everywhere
    pred = torch.zeros(1, K, 2, h, w)
    pred[0, :, 1] = torch.tensor([1.0, 3.0, 2.0]).view(K, 1, 1)
    conf, labels = ops.nway_confusion(pred.to(dev), torch.full((1, S, S), 2, dtype=torch.int64, device=dev), want_labels=True)
    want = torch.zeros(1, K + 1, K + 1, dtype=torch.int64)
    want[0, 2, 2] = 263169
    assert torch.equal(conf.cpu(), want) and (labels == 2).all()


def test_ragged_equals_the_fixed_size_call_per_image(hip_lib, dev):
    from pemp_amd import ops
    K, h, w = 5, 6, 7
    n = len(RAGGED_SIZES)
    g = torch.Generator().manual_seed(23)
    pred = _int_logits((n, K, 2, h, w), g).to(dev)
    targets, binaries = [], []
    for ho, wo in RAGGED_SIZES:
        t = torch.randint(0, K + 1, (ho, wo), generator=g)
        b = torch.randint(0, 2, (ho, wo), generator=g)
        if ho * wo > 1:
            t[torch.rand((ho, wo), generator=g) < 0.1] = 255
            b[torch.rand((ho, wo), generator=g) < 0.1] = 255
        targets.append(t)
        binaries.append(b)
    want = [4, 0, 2, 1, 3]
    alone = [ops.nway_confusion(pred[i:i + 1], t[None].to(dev), want_labels=True) for i, t in enumerate(targets)]
    alone_b = [ops.nway_confusion(pred[i:i + 1], b[None].to(dev), want=[want[i]])[0] for i, b in enumerate(binaries)]
    # the big image against the CPU once more (its table is the only one here that the block cap shapes)
    assert torch.equal(alone[3][0].cpu(), bincount_tables(targets[3][None], alone[3][1], K))
    for tl in (targets, [t.to(dev) for t in targets], [t[None] for t in targets]):          # host, device, [1,Ho,Wo]
        conf, none = ops.nway_confusion_ragged(pred, tl)
        assert none is None and conf.shape == (n, K + 1, K + 1) and conf.dtype == torch.int64
        for i in range(n):
            assert torch.equal(conf[i], alone[i][0][0]), i
    conf, labels = ops.nway_confusion_ragged(pred, targets, want_labels=True)
    assert len(labels) == n and torch.equal(conf, torch.cat([a[0] for a in alone]))
    for i, (ho, wo) in enumerate(RAGGED_SIZES):
        assert labels[i].shape == (ho, wo) and torch.equal(labels[i], alone[i][1][0])
    tail_labels = ops.nway_tail_ragged(pred, RAGGED_SIZES)[0]
    assert all(torch.equal(a, b) for a, b in zip(labels, tail_labels))
    packed = ops.nway_confusion_ragged(pred, targets, want_labels=True, views=False)[1]
    assert packed.shape == (sum(ho * wo for ho, wo in RAGGED_SIZES),) and torch.equal(packed, torch.cat([l.flatten() for l in labels]))
    # lifted
    conf = ops.nway_confusion_ragged(pred, binaries, want=want)[0]
    assert torch.equal(conf, torch.cat(alone_b))
    assert torch.equal(ops.nway_confusion_ragged(pred, binaries, want=torch.tensor(want, dtype=torch.int32, device=dev))[0], conf)


def test_batch_and_repetition(hip_lib, dev):
    from pemp_amd import ops
    N, K, h, w, Ho, Wo = 5, 5, 13, 13, 97, 97
    g = torch.Generator().manual_seed(31)
    pred = _int_logits((N, K, 2, h, w), g).to(dev)
    target = torch.randint(0, K + 1, (N, Ho, Wo), generator=g)
    target[torch.rand((N, Ho, Wo), generator=g) < 0.1] = 255
    target = target.to(dev)
    conf = ops.nway_confusion(pred, target)[0]
    for i in range(N):
        assert torch.equal(ops.nway_confusion(pred[i:i + 1], target[i:i + 1])[0][0], conf[i]), i
    cache = {}
    for _ in range(2):
        assert torch.equal(ops.nway_confusion(pred, target, ws_cache=cache)[0], conf)
    # the entry overwrites conf: a table is not added to what the allocator hands back
    assert torch.equal(ops.nway_confusion(pred, target)[0], conf)


def test_wrapper_refusals_on_device_tensors(hip_lib, dev):
    from pemp_amd import ops
    pred = torch.zeros(2, 3, 2, 4, 4, device=dev)
    tgt = torch.zeros(2, 9, 9, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="K = 64"):
        ops.nway_confusion(torch.zeros(1, 64, 2, 1, 1, device=dev), tgt[:1])
    for bad in (tgt.int(), tgt[:1], tgt.transpose(1, 2)[:, :, :8], tgt[0]):
        with pytest.raises(ValueError, match="target"):
            ops.nway_confusion(pred, bad)
    for bad in (torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(3, dtype=torch.int32, device=dev)):
        with pytest.raises(ValueError, match="device want"):
            ops.nway_confusion(pred, tgt, want=bad)
        with pytest.raises(ValueError, match="device want"):
            ops.nway_confusion_ragged(pred, [tgt[0], tgt[1]], want=bad)
    for want in ([0, 3], [-1, 0], [0]):
        with pytest.raises(ValueError):
            ops.nway_confusion(pred, tgt, want=want)
    conf, labels = ops.nway_confusion(pred, tgt, want=[2, 0])                  # and the good call goes through
    assert labels is None and conf[:, 0, 0].tolist() == [81, 81] and int(conf.sum()) == 162
