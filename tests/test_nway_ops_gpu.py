"""``ops.nway_tail``: the K binary maps of an all-classes bank call fused into one label map, against a torch restatement of the
rule on the upsampled logits ``ops.upsample_bilinear_ac`` gives -- the kernel shares that kernel's interpolation
helper, so every comparison of labels, margins and counts is exact."""
import pytest
import torch

pytestmark = pytest.mark.gpu

#: (N, K, h, w, Ho, Wo)
SHAPES = [(1, 1, 1, 1, 1, 1),              # output size 1: scale 0
          (2, 1, 13, 13, 97, 97),          # K = 1
          (1, 3, 3, 5, 7, 9),              # not square
          (2, 5, 13, 13, 97, 101),         # row length = 1 mod 4
          (1, 20, 7, 7, 33, 33),           # K = 20
          (1, 255, 2, 2, 5, 5),            # K at the uint8 limit
          (3, 4, 51, 51, 401, 401),        # the workload's own size
          (1, 2, 9, 9, 520, 521)]          # more pixels than the 256 x 1024 of a full grid: the grid-stride loop's second pass
_IDS = ["x".join(str(v) for v in s) for s in SHAPES]


def rule(up):
    """The rule on upsampled logits ``up`` [N,K,2,Ho,Wo]: an explicit walk over k upward with a strict > (torch.max's tie order is
    unspecified).  -> (labels uint8, margin fp32, claims bool [N,K,Ho,Wo])."""
    N, K = up.shape[:2]
    labels = torch.zeros((N,) + tuple(up.shape[-2:]), dtype=torch.uint8, device=up.device)
    best = torch.zeros(labels.shape, dtype=torch.float32, device=up.device)
    top = torch.full(labels.shape, float("-inf"), dtype=torch.float32, device=up.device)
    claims = []
    for k in range(K):
        l0, l1 = up[:, k, 0], up[:, k, 1]
        m = l1 - l0                                            # one fp32 subtraction
        claim = l1 > l0
        take = claim & ((labels == 0) | (m > best))
        labels = torch.where(take, torch.full_like(labels, k + 1), labels)
        best = torch.where(take, m, best)
        top = torch.where(m > top, m, top)
        claims.append(claim)
    return labels, torch.where(labels > 0, best, top), torch.stack(claims, 1)


def upsampled(pred, out_hw):
    from pemp_amd import ops
    N, K, _, h, w = pred.shape
    return ops.upsample_bilinear_ac(pred.view(N * K, 2, h, w), out_hw).view(N, K, 2, *out_hw)


_CASES = {}


@pytest.fixture
def case(hip_lib, dev, request):
    """Per shape, computed once and left unchanged: randn logits, a {0, 1} target with a band of 255, wanted slots and the
    restatement's answer."""
    shape = request.param
    if shape not in _CASES:
        N, K, h, w, Ho, Wo = shape
        g = torch.Generator().manual_seed(1000 + sum(shape))
        pred = torch.randn(N, K, 2, h, w, generator=g).to(dev)
        target = torch.randint(0, 2, (N, Ho, Wo), generator=g)
        target[:, Ho // 3:Ho // 3 + max(1, Ho // 8), :] = 255
        if Ho == 1:
            target[:] = 1                                       # one pixel: keep it valid
        want = torch.randint(0, K, (N,), generator=g)
        labels, margin, claims = rule(upsampled(pred, (Ho, Wo)))
        _CASES[shape] = dict(shape=shape, pred=pred, target=target.to(dev), want=want, labels=labels, margin=margin, claims=claims)
    return _CASES[shape]


@pytest.fixture(scope="module", autouse=True)
def _drop_cases():
    yield
    _CASES.clear()


@pytest.mark.parametrize("case", SHAPES, ids=_IDS, indirect=True)
def test_labels_and_margin_equal_the_restatement(case, dev):
    from pemp_amd import ops
    N, K, h, w, Ho, Wo = case["shape"]
    labels, margin, stats = ops.nway_tail(case["pred"], (Ho, Wo), want_margin=True)
    assert stats is None and labels.dtype == torch.uint8 and labels.shape == (N, Ho, Wo) and margin.shape == (N, Ho, Wo)
    assert torch.equal(labels, case["labels"]), f"{(labels != case['labels']).sum().item()} labels differ"
    assert torch.equal(margin, case["margin"])
    assert int(labels.max()) <= K
    # a pixel is 0 iff every one of the K binary maps says background
    assert torch.equal(labels == 0, ~case["claims"].any(dim=1))
    assert ((margin > 0) == (labels > 0)).all()
    # without the margin: the same labels; a workspace cache changes nothing
    cache = {}
    for _ in range(2):
        l2, none, _ = ops.nway_tail(case["pred"], (Ho, Wo), ws_cache=cache)
        assert none is None and torch.equal(l2, labels)
    assert len(cache) == 1


@pytest.mark.parametrize("case", SHAPES, ids=_IDS, indirect=True)
def test_one_class_is_the_binary_tail(case, dev):
    """With K = 1 the label map is eval_tail's arg-max image, here for the first class of every shape."""
    from pemp_amd import ops
    N, K, h, w, Ho, Wo = case["shape"]
    one = case["pred"][:, :1].contiguous()
    labels, _, _ = ops.nway_tail(one, (Ho, Wo))
    am, _, _ = ops.eval_tail(one[:, 0], None, out_hw=(Ho, Wo))
    assert torch.equal(labels, am)
    if K == 1:
        assert torch.equal(case["labels"], am)


@pytest.mark.parametrize("case", SHAPES, ids=_IDS, indirect=True)
def test_statistics_rows(case, dev):
    from pemp_amd import ops
    N, K, h, w, Ho, Wo = case["shape"]
    pred, target, want = case["pred"], case["target"], case["want"]
    labels, none, stats = ops.nway_tail(pred, target=target, want=want)
    assert none is None and stats.shape == (N, 8) and stats.dtype == torch.float64
    assert torch.equal(labels, case["labels"])                  # the labels do not depend on the target
    own = pred[torch.arange(N), want.to(dev)].contiguous()      # [N,2,h,w]: every query's wanted class
    _, ref, _ = ops.eval_tail(own, target)
    stats, ref = stats.cpu(), ref.cpu()
    valid = target != 255
    am = labels == (want.to(dev) + 1).view(N, 1, 1).to(torch.uint8)
    counts = []
    for j, img in ((0, ~am), (1, am)):
        counts += [(img & (target == j) & valid), (img & (target != j) & valid), (~img & (target == j) & valid)]
    counts = torch.stack([c.flatten(1).sum(1) for c in counts], 1).cpu()
    print("stats", stats.tolist(), "eval_tail on the wanted class", ref.tolist())
    assert torch.equal(stats[:, 2:], counts.double())
    assert torch.equal(stats[:, 1], valid.flatten(1).sum(1).double().cpu()) and torch.equal(stats[:, 1], ref[:, 1])
    # the per-pixel CE terms are those of eval_tail (one device function) and non-negative; either order of summing n of them
    # in float64 is within (n - 1) u sum(x) of the true sum, u = 2^-53
    bound = 2.0 * stats[:, 1] * 2.0 ** -53 * ref[:, 0]
    assert ((stats[:, 0] - ref[:, 0]).abs() <= bound).all(), (stats[:, 0] - ref[:, 0]).abs().tolist()
    assert (stats[:, 0] > 0).all()
    # under competition the wanted class can only lose foreground pixels against its own binary map
    assert (stats[:, 5] + stats[:, 6] <= ref[:, 5] + ref[:, 6]).all()
    # want as a CPU tensor of another integer type, a Python list and a device int32 tensor: the same rows
    for w2 in (want.to(torch.int16), want.tolist(), want.to(torch.int32).to(dev)):
        l2, _, s2 = ops.nway_tail(pred, target=target, want=w2)
        assert torch.equal(l2, labels) and torch.equal(s2.cpu(), stats)


def _int_logits(shape, gen, lo=-4, hi=5):
    return torch.randint(lo, hi, shape, generator=gen).float()


@pytest.mark.parametrize("shape", [(2, 5, 13, 13, 97, 101), (1, 255, 2, 2, 5, 5)], ids=["2x5", "1x255"])
def test_ties(hip_lib, dev, shape):
    from pemp_amd import ops
    N, K, h, w, Ho, Wo = shape
    g = torch.Generator().manual_seed(7)
    # all classes identical: equal margins everywhere, the lowest slot wins wherever there is a claim
    one = _int_logits((N, 1, 2, h, w), g)
    pred = one.expand(N, K, 2, h, w).contiguous().to(dev)
    labels, margin, _ = ops.nway_tail(pred, (Ho, Wo), want_margin=True)
    am, _, _ = ops.eval_tail(pred[:, 0].contiguous(), None, out_hw=(Ho, Wo))
    assert torch.equal(labels, am) and (h * w < 100 or 0 < int(am.sum()) < am.numel())
    ref = rule(upsampled(pred, (Ho, Wo)))
    assert torch.equal(labels, ref[0]) and torch.equal(margin, ref[1])
    # foreground logit == background logit in every class: a tie is background
    pred = _int_logits((N, K, 1, h, w), g).expand(N, K, 2, h, w).contiguous().to(dev)
    labels, margin, _ = ops.nway_tail(pred, (Ho, Wo), want_margin=True)
    assert not labels.any() and not margin.any()
    # every margin negative: no label, and the margin is the largest of the K
    bg = _int_logits((N, K, h, w), g)
    gap = torch.randint(1, 6, (N, K, h, w), generator=g).float()
    pred = torch.stack([bg, bg - gap], 2).contiguous().to(dev)
    labels, margin, _ = ops.nway_tail(pred, (Ho, Wo), want_margin=True)
    up = upsampled(pred, (Ho, Wo))
    m = up[:, :, 1] - up[:, :, 0]
    assert not labels.any() and (m < 0).all() and torch.equal(margin, m.max(dim=1).values)
    # two classes with the same planes, hence equal positive margins, among classes that do not claim: the lower slot
    pred = torch.stack([bg, bg - gap], 2)
    pred[:, 1, 1] = pred[:, 1, 0] + 3
    pred[:, K - 1] = pred[:, 1]
    pred = pred.contiguous().to(dev)
    labels, margin, _ = ops.nway_tail(pred, (Ho, Wo), want_margin=True)
    ref = rule(upsampled(pred, (Ho, Wo)))
    assert torch.equal(labels, ref[0]) and torch.equal(margin, ref[1])
    assert (labels == 2).all() and (margin > 2.9).all()


@pytest.mark.parametrize("case", [SHAPES[3], SHAPES[4]], ids=[_IDS[3], _IDS[4]], indirect=True)
def test_permuting_the_classes_permutes_the_labels(case, dev):
    from pemp_amd import ops
    N, K, h, w, Ho, Wo = case["shape"]
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(3)).to(dev)
    labels, margin, _ = ops.nway_tail(case["pred"][:, perm].contiguous(), (Ho, Wo), want_margin=True)
    # new slot j holds old class perm[j]: an old label v > 0 becomes 1 + the j with perm[j] == v - 1
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(K, device=dev)
    table = torch.cat([torch.zeros(1, dtype=torch.long, device=dev), inv + 1])
    want = table[case["labels"].long()].to(torch.uint8)
    # where two classes tie in the margin the lower slot wins, which a permutation changes: compare the tie-free pixels
    up = upsampled(case["pred"], (Ho, Wo))
    m = (up[:, :, 1] - up[:, :, 0]).sort(dim=1).values
    free = (m[:, 1:] != m[:, :-1]).all(dim=1)
    assert free.float().mean() > 0.99
    assert torch.equal(labels[free], want[free]) and torch.equal(margin[free], case["margin"][free])


def test_wrapper_refusals(hip_lib, dev):
    from pemp_amd import ops
    pred = torch.zeros(2, 3, 2, 4, 4, device=dev)
    tgt = torch.zeros(2, 9, 9, dtype=torch.int64, device=dev)
    for bad in (pred[0], pred.double(), pred.transpose(3, 4), torch.zeros(2, 3, 3, 4, 4, device=dev), pred[:, :, :1],
                torch.zeros(1, 256, 2, 1, 1, device=dev)):
        with pytest.raises(ValueError, match="nway_tail"):
            ops.nway_tail(bad, (9, 9))
    with pytest.raises(ValueError, match="K = 256"):
        ops.nway_tail(torch.zeros(1, 256, 2, 1, 1, device=dev), (9, 9))
    for want in ([0, 3], [-1, 0], torch.tensor([0, 3]), [0], [0.5, 1]):
        with pytest.raises(ValueError):
            ops.nway_tail(pred, target=tgt, want=want)
    with pytest.raises(ValueError, match="come together"):
        ops.nway_tail(pred, target=tgt)
    with pytest.raises(ValueError, match="come together"):
        ops.nway_tail(pred, (9, 9), want=[0, 1])
    with pytest.raises(ValueError, match="out_hw"):
        ops.nway_tail(pred)
    with pytest.raises(ValueError, match="out_hw"):
        ops.nway_tail(pred, (9, 8), target=tgt, want=[0, 1])
    for bad in (tgt.int(), tgt[:1], tgt.transpose(1, 2)[:, :, :8], tgt[0]):
        with pytest.raises(ValueError, match="target"):
            ops.nway_tail(pred, target=bad, want=[0, 1])
    for bad in (torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(3, dtype=torch.int32, device=dev)):
        with pytest.raises(ValueError, match="device want"):
            ops.nway_tail(pred, target=tgt, want=bad)
    labels, margin, stats = ops.nway_tail(pred, target=tgt, want=[2, 0])       # and the good call goes through
    assert not labels.any() and margin is None and stats.shape == (2, 8)
