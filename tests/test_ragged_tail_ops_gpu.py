"""``ops.eval_tail_ragged`` / ``ops.nway_tail_ragged``: one launch pair for a batch whose images each have their own output
size.  The yardstick is the fixed-size tail run on each image alone (``ops.eval_tail``, ``ops.nway_tail``, which the suite holds
to the oracle); every comparison is ``torch.equal``: the ragged kernels walk an image with the same blocks, the same pixel
body and the same order of sums."""
import pytest
import torch

pytestmark = pytest.mark.gpu

#: one batch: the smallest image; a non-square size, its transpose, and the size again; 1023 and 1024 pixels (the last counts
#: with one block) and 1025 (the first with two); 67 blocks (the final sum wraps its 64 lanes); the 256-block clamp with a
#: grid-stride loop of more than four rounds
SIZES = [(1, 1), (17, 23), (23, 17), (17, 23), (33, 31), (32, 32), (25, 41), (263, 257), (520, 510)]
PERM = [8, 3, 0, 6, 1, 7, 5, 2, 4]
LOW = [(13, 13), (7, 11)]
B = len(SIZES)
ALL_IGNORED = 2                             # this image's target is 255 everywhere: n_valid = 0
TIES = 4                                    # this image's two planes are equal on half of their rows: exact ties

_REF = {}


def _data(hw, dev):
    """Per low-resolution size, made once and left unchanged: predictions, targets, and the fixed-size tails' answers per image."""
    if hw in _REF:
        return _REF[hw]
    from pemp_amd import ops
    h, w = hw
    g = torch.Generator().manual_seed(97 * h + w)
    pred = torch.randn(B, 2, h, w, generator=g)
    pred[TIES, 1, : h // 2 + 1] = pred[TIES, 0, : h // 2 + 1]
    targets = []
    for i, (ho, wo) in enumerate(SIZES):
        t = torch.randint(0, 2, (ho, wo), generator=g)
        t[torch.rand(ho, wo, generator=g) < 0.1] = 255
        if i == ALL_IGNORED:
            t[:] = 255
        targets.append(t)
    nway = {}
    for K in (1, 3):
        p5 = torch.randn(B, K, 2, h, w, generator=g)
        p5[TIES, :, 1, : h // 2 + 1] = p5[TIES, :, 0, : h // 2 + 1]
        nway[K] = dict(pred=p5.to(dev), want=[int(v) for v in torch.randint(0, K, (B,), generator=g)])
    d = dict(pred=pred.to(dev), targets=targets, targets_dev=[t.to(dev) for t in targets], nway=nway)
    d["eval"] = [ops.eval_tail(d["pred"][i:i + 1], d["targets_dev"][i][None]) for i in range(B)]
    d["argmax"] = [ops.eval_tail(d["pred"][i:i + 1], None, out_hw=SIZES[i])[0] for i in range(B)]
    for K, c in nway.items():
        c["scored"] = [ops.nway_tail(c["pred"][i:i + 1], target=d["targets_dev"][i][None], want=[c["want"][i]], want_margin=True)
                       for i in range(B)]
        c["plain"] = [ops.nway_tail(c["pred"][i:i + 1], SIZES[i])[0] for i in range(B)]
    _REF[hw] = d
    return d


@pytest.fixture(scope="module", autouse=True)
def _drop():
    yield
    _REF.clear()


_ORDERS = {"given": list(range(B)), "permuted": PERM}
_GRID = [(hw, o) for hw in LOW for o in _ORDERS]
_IDS = [f"{hw[0]}x{hw[1]}-{o}" for hw, o in _GRID]


@pytest.mark.parametrize("hw,order", _GRID, ids=_IDS)
def test_eval_tail_ragged_is_the_fixed_size_tail_per_image(hip_lib, dev, hw, order):
    from pemp_amd import ops
    d, idx = _data(hw, dev), _ORDERS[order]
    pred = d["pred"][idx].contiguous()
    # device targets as [Ho,Wo] (one concatenation); host targets as [1,Ho,Wo] (each uploaded into its place)
    for targets in ([d["targets_dev"][i] for i in idx], [d["targets"][i][None] for i in idx]):
        am_list, stats, packed = ops.eval_tail_ragged(pred, targets)
        assert stats.shape == (B, 8) and stats.dtype == torch.float64 and packed.dtype == torch.uint8
        assert packed.numel() == sum(ho * wo for ho, wo in SIZES) and len(am_list) == B
        off = 0
        for j, i in enumerate(idx):
            am, st, _ = d["eval"][i]
            assert tuple(am_list[j].shape) == SIZES[i] and am_list[j].data_ptr() == packed.data_ptr() + off      # a view
            assert torch.equal(am_list[j], am[0]), (j, i, SIZES[i])
            assert torch.equal(stats[j], st[0]), (j, i, SIZES[i], stats[j].tolist(), st[0].tolist())
            off += SIZES[i][0] * SIZES[i][1]
        assert float(stats[idx.index(ALL_IGNORED), 1]) == 0.0 and float(stats[idx.index(ALL_IGNORED), 0]) == 0.0
        assert float(stats[idx.index(8), 1]) > 200000                      # the large image really was counted
    # sizes alone: arg-max only
    am_list, stats, packed = ops.eval_tail_ragged(pred, sizes=[SIZES[i] for i in idx])
    assert stats is None
    for j, i in enumerate(idx):
        assert torch.equal(am_list[j], d["argmax"][i][0]) and torch.equal(am_list[j], d["eval"][i][0][0]), (j, i)
    ties = am_list[idx.index(TIES)]
    assert int(ties[0].sum()) == 0                                          # equal logits: background


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("hw,order", _GRID, ids=_IDS)
def test_nway_tail_ragged_is_the_fixed_size_tail_per_image(hip_lib, dev, hw, order, K):
    from pemp_amd import ops
    d, idx = _data(hw, dev), _ORDERS[order]
    c = d["nway"][K]
    pred = c["pred"][idx].contiguous()
    targets = [d["targets_dev"][i] for i in idx]
    want = [c["want"][i] for i in idx]
    labels, margin, stats = ops.nway_tail_ragged(pred, targets=targets, want=want, want_margin=True)
    for j, i in enumerate(idx):
        l1, m1, s1 = c["scored"][i]
        assert torch.equal(labels[j], l1[0]) and tuple(labels[j].shape) == SIZES[i], (j, i)
        assert torch.equal(margin[j], m1[0]) and margin[j].dtype == torch.float32, (j, i)
        assert torch.equal(stats[j], s1[0]), (j, i, stats[j].tolist(), s1[0].tolist())
    # without the margin; a device int32 want gives what the Python list gives; host targets
    l2, none, s2 = ops.nway_tail_ragged(pred, targets=[d["targets"][i][None] for i in idx],
                                        want=torch.tensor(want, dtype=torch.int32, device=dev))
    assert none is None and torch.equal(s2, stats) and all(torch.equal(a, b) for a, b in zip(l2, labels))
    # without a target: labels only
    l3, none, s3 = ops.nway_tail_ragged(pred, [SIZES[i] for i in idx])
    assert none is None and s3 is None
    for j, i in enumerate(idx):
        assert torch.equal(l3[j], c["plain"][i][0]) and torch.equal(l3[j], labels[j]), (j, i)
    l4, m4, _ = ops.nway_tail_ragged(pred, [SIZES[i] for i in idx], want_margin=True)
    assert all(torch.equal(a, b) for a, b in zip(m4, margin)) and all(torch.equal(a, b) for a, b in zip(l4, labels))
    assert int(labels[idx.index(TIES)][0].sum()) == 0                      # equal logits: nobody claims the tied rows


def test_a_reused_workspace_serves_another_size_mix_of_the_same_batch_size(hip_lib, dev):
    from pemp_amd import ops
    d = _data(LOW[0], dev)
    cache = {}
    small = [0, 1, 2, 3, 4, 5, 6, 0, 1]                                    # nine small images first: a small workspace
    mixes = [small, list(range(B)), small, PERM, list(range(B))]
    seen = []
    for idx in mixes:
        pred = d["pred"][idx].contiguous()
        am_list, stats, _ = ops.eval_tail_ragged(pred, [d["targets_dev"][i] for i in idx], ws_cache=cache)
        for j, i in enumerate(idx):
            assert torch.equal(am_list[j], d["eval"][i][0][0]) and torch.equal(stats[j], d["eval"][i][1][0]), (idx, j)
        c = d["nway"][3]
        labels, _, st = ops.nway_tail_ragged(c["pred"][idx].contiguous(), targets=[d["targets_dev"][i] for i in idx],
                                             want=[c["want"][i] for i in idx], ws_cache=cache)
        for j, i in enumerate(idx):
            assert torch.equal(labels[j], c["scored"][i][0][0]) and torch.equal(st[j], c["scored"][i][2][0]), (idx, j)
        seen.append(cache[("tail_ragged", B)].numel())
    # one workspace per batch size, grown to the largest mix and kept: not one per size combination
    assert list(cache) == [("tail_ragged", B)] and seen[1] > seen[0] and seen[1:] == [seen[1]] * 4
