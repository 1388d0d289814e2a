"""Row pruning in ResNetEngine.forward (engine.PRUNE_ROWS, DESIGN.md "Row pruning"): layer1's last block computes only the rows that
layer2's stride-2 1x1 convs read -- conv2 at stride 2, conv3 with the block input as a stride-2 residual (ops.conv2d
residual_stride=2), layer2's block 0 at stride 1 on the compact tensor.  Every output row is the same dot product through the same
split, so every comparison here is torch.equal.

 * switch on against switch off on random weights: 2 images of 49 x 49 (layer1 grid 13, odd) and of 61 x 61 (grid 16, even);
 * a stage named in ``stage_outs`` is produced in full; ResNetCMEngine (whose cm_reduce reads the whole map) does not change;
 * a one-image pass equals the batched pass;
 * the launch list, through a recording stand-in for the library handle: position 9 (layer1 block 2's conv2 in a [3, ...] trunk, as
   in the benchmark's trace) runs at stride 2, position 10 carries the flag, positions 11 and 13 run at stride 1."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = {49: 13, 61: 16}         # image side -> layer1's grid


def _randomise(prm, seed):
    g = torch.Generator().manual_seed(seed)
    for m in prm.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
            m.weight.data.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
            m.bias.data.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
    return prm


@pytest.fixture(scope="module")
def trunk_params(dev):
    from pemp_amd.networks import backbones
    torch.manual_seed(9)
    return _randomise(backbones.ResNetParams(3, [3, 2, 2]), 9).to(dev).eval()


@pytest.fixture
def clean_picks():
    from pemp_amd import ops
    saved = dict(ops._TILE_CACHE)
    yield ops
    ops._TILE_CACHE.clear()
    ops._TILE_CACHE.update(saved)


def _images(dev, n, side, seed=3):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(n, 3, side, side, generator=g, device=dev)


def _forward(engine, prm, dev, images, prune, monkeypatch, stage_outs=None):
    """A fresh engine and arena per arm: no buffer of one arm is read by the other."""
    monkeypatch.setattr(engine, "PRUNE_ROWS", prune)
    arena = engine.Arena(dev)
    eng = engine.ResNetEngine(prm, arena)
    out = eng.forward(engine.pack_episode(arena, (images,)), stage_outs=stage_outs)
    torch.cuda.synchronize()
    return eng, arena, out


@pytest.mark.parametrize("side", sorted(SIZES))
def test_pruned_forward_equals_the_full_one_bit_for_bit(hip_lib, dev, trunk_params, clean_picks, monkeypatch, side):
    from pemp_amd import engine, ops
    assert engine.SPLIT3
    stem = ops.conv_out_size(side, 7, 2, 3, 1)
    grid = ops._pool_out(stem, 3, 2, 1, True)
    assert grid == SIZES[side]
    images = _images(dev, 2, side)
    eng, arena, full = _forward(engine, trunk_params, dev, images, False, monkeypatch)
    assert not any(eng._prunes(si) for si in range(3))
    eng, arena, pruned = _forward(engine, trunk_params, dev, images, True, monkeypatch)
    assert [eng._prunes(si) for si in range(3)] == [True, False, False]            # layer3 is dilated, not strided
    half = (grid - 1) // 2 + 1
    assert tuple(full.shape) == tuple(pruned.shape) == (2, half, half, 1024)
    assert bool(full.abs().sum() > 0) and torch.equal(full, pruned)
    # the pruned arm never made layer1's full last output: its block buffers of that size are those of blocks 0 and 1 only
    compact = [k for k in arena.bufs if k[0] == ("blk", (0, 0)) and k[1] == (2, half, half, 256)]
    assert len(compact) == 1, list(arena.bufs)


def test_a_stage_that_is_asked_for_is_produced_in_full(hip_lib, dev, trunk_params, clean_picks, monkeypatch):
    from pemp_amd import engine
    images = _images(dev, 2, 49)
    outs = {}
    for prune in (False, True):
        keep = torch.full((2, 13, 13, 256), float("nan"), device=dev)
        eng, _, last = _forward(engine, trunk_params, dev, images, prune, monkeypatch, stage_outs={0: keep})
        assert not eng._prunes(0, {0: keep})
        outs[prune] = (keep, last.clone())
    assert not bool(torch.isnan(outs[True][0]).any())
    assert torch.equal(outs[True][0], outs[False][0]) and torch.equal(outs[True][1], outs[False][1])
    # ... and it is what the pruned trunk gathers from
    _, _, pruned = _forward(engine, trunk_params, dev, images, True, monkeypatch)
    assert torch.equal(pruned, outs[True][1])


def test_one_image_equals_the_batched_pass(hip_lib, dev, trunk_params, clean_picks, monkeypatch):
    from pemp_amd import engine
    images = _images(dev, 2, 61)
    _, _, both = _forward(engine, trunk_params, dev, images, True, monkeypatch)
    for i in range(2):
        _, _, one = _forward(engine, trunk_params, dev, images[i:i + 1], True, monkeypatch)
        assert torch.equal(one[0], both[i]), i


def test_the_cm_trunk_is_left_alone(hip_lib, dev, clean_picks, monkeypatch):
    from pemp_amd import engine
    from pemp_amd.networks import backbones
    torch.manual_seed(10)
    prm = _randomise(backbones.ResNetCMParams(4, [2, 1, 1], shot_query=2), 10).to(dev).eval()
    images = _images(dev, 2, 49, seed=4)
    prior = (torch.rand(2, 49, 49, generator=torch.Generator(device=dev).manual_seed(5), device=dev) > 0.5).float()
    outs = {}
    for prune in (False, True):
        monkeypatch.setattr(engine, "PRUNE_ROWS", prune)
        arena = engine.Arena(dev)
        eng = engine.ResNetCMEngine(prm, arena)
        eng.group, eng.n_groups = torch.zeros(2, dtype=torch.int32, device=dev), 1
        outs[prune] = eng.forward(engine.pack_episode(arena, (images,), (prior,)), prior).clone()
        last = [k[1] for k in arena.bufs if k[0] == ("blk", (0, 1))]                       # layer1's last block: never compact
        assert last == [(2, 13, 13, 256)], list(arena.bufs)
    assert bool(outs[True].abs().sum() > 0) and torch.equal(outs[True], outs[False])


class _Recorder:
    """Stand-in for the library handle: notes the descriptor of every pemp_conv2d_nhwc_f32 call, in order."""

    def __init__(self, lib):
        self._lib, self.convs = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "pemp_conv2d_nhwc_f32":
            return fn

        def noted(*a):
            d = a[0]._obj
            self.convs.append({f: getattr(d, f) for f, _ in d._fields_})
            return fn(*a)
        return noted


def test_the_launch_list(hip_lib, dev, trunk_params, clean_picks, monkeypatch):
    from pemp_amd import _lib, engine
    monkeypatch.setattr(engine, "GROUP_MAX_ROWS", 0)                 # conv1 and the downsample conv one by one, as on the full step
    images = _images(dev, 2, 49)
    lists = {}
    real = _lib.load()
    for prune in (False, True):
        rec = _Recorder(real)
        monkeypatch.setattr(_lib, "load", lambda rec=rec: rec)
        _forward(engine, trunk_params, dev, images, prune, monkeypatch)
        lists[prune] = rec.convs
    monkeypatch.setattr(_lib, "load", lambda: real)
    full, pruned = lists[False], lists[True]
    S2 = _lib.CONV_RES_S2
    assert len(full) == len(pruned) == 1 + 4 + 3 + 3 + 4 + 3 + 4 + 3          # the fused stem, then the bottlenecks' convs
    assert not any(d["flags"] & S2 for d in full)
    geom = lambda d: (d["KH"], d["stride"], d["H"], d["Ho"], d["Cin"], d["Cout"])
    assert geom(full[9]) == (3, 1, 13, 13, 64, 64) and geom(pruned[9]) == (3, 2, 13, 7, 64, 64)
    assert geom(full[10]) == (1, 1, 13, 13, 64, 256) and geom(pruned[10]) == (1, 1, 7, 7, 64, 256)
    assert pruned[10]["flags"] & S2 and not pruned[10]["flags"] & (_lib.CONV_RES_HEVEN | _lib.CONV_RES_WEVEN)      # 13: odd
    assert [i for i, d in enumerate(pruned) if d["flags"] & S2] == [10]
    for pos in (11, 13):                                             # layer2 block 0: conv1 and the downsample conv
        assert geom(full[pos])[:4] == (1, 2, 13, 7) and geom(pruned[pos])[:4] == (1, 1, 7, 7), pos
    untiled = lambda d: {k: v for k, v in d.items() if k != "tile"}
    for pos in set(range(len(full))) - {9, 10, 11, 13}:
        assert untiled(full[pos]) == untiled(pruned[pos]), pos
