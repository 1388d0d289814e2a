"""Pre-split activations on the device (conv_dma2.hip A3, tile ids 146 / 149; conv_common.h conv_store_split3), bit for bit:

 * producer: a conv with ``out_split3`` writes exactly the reference split (tests/test_conv_split3_presplit_cpu.py: presplit) of what
   the same id writes as fp32, on every unsplit id, and nothing behind its buffer;
 * consumer: ids 146 / 149 on the pre-split tensor equal id 43 on the fp32 tensor -- plain, dilated, strided, padding that is not the
   dilation's with a padding vector; one, two and eight K chunks; tails; a launch whose blocks walk several tiles; every epilogue;
 * the chain producer -> consumer equals the fp32 pair, eager and from a graph replay;
 * the six piece probes of the fuzz tests are exact on the new ids;
 * a ResNet bottleneck and the purifier's p0 -> p3 give the same bits with the hand-over on and off, and no pick crosses over."""
import pytest
import torch
import torch.nn as nn

from tests import test_conv_split3_fuzz_cpu as A
from tests.test_conv_split3_presplit_cpu import presplit, unsplit

pytestmark = pytest.mark.gpu

NEW = (146, 149)
PRODUCERS = (41, 42, 43, 44, 46, 47, 49)
SENTINEL = -3.0


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _params(ops, w, stride, pad, dil, scale=None, shift=None, relu=False):
    packed, kpad = ops.pack_conv_weight(w)
    packed = packed.contiguous()
    co, ci, kh, kw = w.shape
    return ops.ConvParams(packed, scale, shift, ci, co, kh, kw, stride, pad, dil, kpad, False, relu, ops.pack_split3(packed))


def _rand(dev, seed, *shape):
    return torch.randn(*shape, generator=torch.Generator(device=dev).manual_seed(seed), device=dev)


def _activations(dev, seed, N, H, W, cin, padv):
    """fp32 x with its padding vector right behind it, and the same two pre-split in one bf16 buffer."""
    M = N * H * W
    buf = _rand(dev, seed, M + 4, cin)
    x, pv = buf[:M].view(N, H, W, cin), (buf[M] if padv else None)
    sbuf = torch.zeros((M + 4) * cin * 3, dtype=torch.bfloat16, device=dev)
    xs = sbuf[:M * cin * 3].view(N, H, W, cin // 32, 3, 32)
    xs.copy_(presplit(x))
    pvs = None
    if padv:
        pvs = sbuf[M * cin * 3:(M + 1) * cin * 3].view(cin // 32, 3, 32)
        pvs.copy_(presplit(pv.view(1, 1, 1, cin)).view(cin // 32, 3, 32))
    assert torch.equal(_bits(unsplit(xs)), _bits(x))
    return x, pv, xs, pvs


# ---- producer -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("nhw", [(2, 9, 13), (5, 9, 29)], ids=["M234", "M1305"])
@pytest.mark.parametrize("cin,cout", [(64, 64), (96, 128)])
def test_producer_writes_the_split_of_its_own_fp32_output(hip_lib, dev, cin, cout, nhw, relu):
    from pemp_amd import ops
    N, H, W = nhw
    M = N * H * W
    x = _rand(dev, 5 + cin, N, H, W, cin)
    w = _rand(dev, 6 + cin, cout, cin, 1, 1) / cin ** 0.5
    prm = _params(ops, w, 1, 0, 1, _rand(dev, 7, cout).abs() + 0.5, _rand(dev, 8, cout), relu)
    ran = 0
    for tile in PRODUCERS:
        if cout % ops._tile_bn(tile):
            continue
        y = ops.conv2d(x, prm, tile=tile)
        assert bool((y < 0).any()) != relu and bool(y.abs().sum() > 0)
        buf = torch.full((M * cout * 3 + 256,), SENTINEL, dtype=torch.bfloat16, device=dev)
        out = buf[:M * cout * 3].view(ops.split3_shape(N, H, W, cout))
        assert ops.conv2d(x, prm, tile=tile, out=out, out_split3=True) is out
        bad = _bits(out) != _bits(presplit(y))
        assert not bool(bad.any()), (tile, int(bad.sum()), bad.nonzero()[:4].tolist())
        assert torch.equal(_bits(unsplit(out)), _bits(y)), tile
        assert bool((buf[M * cout * 3:] == SENTINEL).all()), tile
        ran += 1
    assert ran >= (7 if cout % 128 == 0 else 3)


def test_producer_with_a_per_image_shift(hip_lib, dev):
    from pemp_amd import ops
    N, H, W, cin, cout = 3, 7, 11, 64, 128
    x, w = _rand(dev, 1, N, H, W, cin), _rand(dev, 2, cout, cin, 1, 1) / 8
    prm = _params(ops, w, 1, 0, 1, relu=True)
    kw = dict(shift_override=_rand(dev, 3, N, cout), per_image_shift=True)
    for tile in (43, 46):
        y = ops.conv2d(x, prm, tile=tile, **kw)
        out = ops.conv2d(x, prm, tile=tile, out_split3=True, **kw)
        assert torch.equal(_bits(out), _bits(presplit(y))), tile


# ---- consumer -------------------------------------------------------------------------------------------------------------------
# (k, stride, pad, dil, padding vector) and the input sizes that give M = 234 and M = 1305 output rows
GEOMS = {
    "3x3": ((3, 1, 1, 1, False), {234: (2, 9, 13), 1305: (5, 9, 29)}),
    "3x3-dil2": ((3, 1, 2, 2, False), {234: (2, 9, 13), 1305: (5, 9, 29)}),
    "3x3-stride2": ((3, 2, 1, 1, False), {234: (2, 17, 25), 1305: (5, 17, 57)}),
    "3x3-dil6-pad4-padv": ((3, 1, 4, 6, True), {234: (2, 13, 17), 1305: (5, 13, 33)}),
}


def _consumer_check(ops, dev, x, pv, xs, pvs, prm, want_rows=None, **kw):
    want = ops.conv2d(x, prm, tile=43, pad_value=pv, **kw)
    if want_rows is not None:
        assert want.shape[0] * want.shape[1] * want.shape[2] == want_rows
    assert bool(want.abs().sum() > 0)
    for tile in NEW:
        for again in range(2):
            got = torch.full_like(want, float("nan"))
            ops.conv2d(xs, prm, tile=tile, out=got, pad_value=pvs, x_split3=True, **kw)
            bad = got != want
            assert not bool(bad.any()), (tile, again, int(bad.sum()), bad.nonzero()[:4].tolist())


@pytest.mark.parametrize("M", [234, 1305])
@pytest.mark.parametrize("cout", [128, 256])
@pytest.mark.parametrize("cin", [32, 64, 256])
@pytest.mark.parametrize("geom", sorted(GEOMS))
def test_consumer_equals_id_43_on_the_fp32_tensor(hip_lib, dev, geom, cin, cout, M):
    from pemp_amd import ops
    (k, s, p, d, padv), sizes = GEOMS[geom]
    N, H, W = sizes[M]
    x, pv, xs, pvs = _activations(dev, 3 + cin + M, N, H, W, cin, padv)
    w = _rand(dev, 4 + cin + cout, cout, cin, k, k) / (cin * k * k) ** 0.5
    _consumer_check(ops, dev, x, pv, xs, pvs, _params(ops, w, s, p, d), want_rows=M)


def test_consumer_blocks_walk_several_tiles(hip_lib, dev):
    """test_conv_split3_persist_gpu.py's smallest-Cin multi-tap LARGE shape: several times more tiles than resident blocks."""
    from pemp_amd import ops
    N, H, W, cin, cout, k, dil = 20, 51, 51, 32, 1024, 3, 2
    tiles = -(-N * H * W // 256) * (cout // 128)
    assert tiles >= 3 * torch.cuda.get_device_properties(dev).multi_processor_count          # one 144 KiB block per CU
    x, pv, xs, pvs = _activations(dev, 9, N, H, W, cin, True)
    w = _rand(dev, 10, cout, cin, k, k) / (cin * k * k) ** 0.5
    _consumer_check(ops, dev, x, None, xs, None, _params(ops, w, 1, dil, dil))
    _consumer_check(ops, dev, x, pv, xs, pvs, _params(ops, w, 1, dil, dil, relu=True))


@pytest.mark.parametrize("nhw", [(2, 9, 13), (5, 9, 29)], ids=["M234", "M1305"])
def test_consumer_epilogues(hip_lib, dev, nhw):
    from pemp_amd import ops
    N, H, W = nhw
    cin, cout = 64, 256
    x, pv, xs, pvs = _activations(dev, 21, N, H, W, cin, False)
    w = _rand(dev, 22, cout, cin, 3, 3) / (cin * 9) ** 0.5
    scale, shift, res = _rand(dev, 23, cout), _rand(dev, 24, cout), _rand(dev, 25, N, H, W, cout)
    _consumer_check(ops, dev, x, pv, xs, pvs, _params(ops, w, 1, 1, 1, scale, shift, relu=True), residual=res)
    _consumer_check(ops, dev, x, pv, xs, pvs, _params(ops, w, 1, 1, 1, scale, shift))
    _consumer_check(ops, dev, x, pv, xs, pvs, _params(ops, w, 1, 1, 1, None, shift, relu=True))
    # a consumer that is itself a producer
    prm = _params(ops, w, 1, 1, 1, scale, shift, relu=True)
    want = presplit(ops.conv2d(x, prm, tile=43))
    for tile in NEW:
        got = ops.conv2d(xs, prm, tile=tile, x_split3=True, out_split3=True)
        assert torch.equal(_bits(got), _bits(want)), tile


# ---- chain ----------------------------------------------------------------------------------------------------------------------
def test_chain_equals_the_fp32_pair_eager_and_replayed(hip_lib, dev):
    from pemp_amd import ops
    N, H, W, cin, mid = 5, 9, 29, 96, 128
    x = _rand(dev, 31, N, H, W, cin)
    c1 = _params(ops, _rand(dev, 32, mid, cin, 1, 1) / cin ** 0.5, 1, 0, 1, _rand(dev, 33, mid), _rand(dev, 34, mid), relu=True)
    c2 = _params(ops, _rand(dev, 35, mid, mid, 3, 3) / (mid * 9) ** 0.5, 1, 2, 2, _rand(dev, 36, mid), _rand(dev, 37, mid), relu=True)
    want = ops.conv2d(ops.conv2d(x, c1, tile=43), c2, tile=43)
    assert bool(want.abs().sum() > 0)
    y1s = torch.zeros(ops.split3_shape(N, H, W, mid), dtype=torch.bfloat16, device=dev)
    for t1, t2 in ((43, 146), (46, 149), (49, 149)):
        got = torch.full_like(want, float("nan"))
        ops.conv2d(ops.conv2d(x, c1, tile=t1, out=y1s, out_split3=True), c2, tile=t2, out=got, x_split3=True)
        assert torch.equal(got, want), (t1, t2)
    got = torch.full_like(want, float("nan"))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.conv2d(ops.conv2d(x, c1, tile=46, out=y1s, out_split3=True), c2, tile=149, out=got, x_split3=True)
    y1s.zero_()
    got.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got, want)


# ---- piece probes ---------------------------------------------------------------------------------------------------------------
DILATED = A.PROBE_GEOMS[1]
assert DILATED[4] == 3 and DILATED[7] == 2 and DILATED[8]          # the dilated 3x3 with a padding value


@pytest.mark.parametrize("probe", [(pq, DILATED) for pq in A.PRODUCTS], ids=A.probe_id)
def test_new_ids_are_exact_on_the_piece_probes(hip_lib, dev, probe):
    from pemp_amd import ops
    q = A.probe_problem(probe)
    ref = A.conv_f64(q["x"], q["w"], q["stride"], q["pad"], q["dil"], q["pv"])
    want = ref.float().to(dev)
    assert torch.equal(want.double().cpu(), ref)
    N, H, W, cin = q["x"].shape
    M = N * H * W
    sbuf = torch.zeros((M + 4) * cin * 3, dtype=torch.bfloat16)
    sbuf[:M * cin * 3] = presplit(q["x"]).reshape(-1)                 # split on the CPU: the reference split itself
    sbuf[M * cin * 3:(M + 1) * cin * 3] = presplit(q["pv"].view(1, 1, 1, cin)).reshape(-1)
    sbuf = sbuf.to(dev)
    xs, pvs = sbuf[:M * cin * 3].view(N, H, W, cin // 32, 3, 32), sbuf[M * cin * 3:(M + 1) * cin * 3].view(cin // 32, 3, 32)
    prm = _params(ops, q["w"].to(dev), q["stride"], q["pad"], q["dil"])
    for tile in NEW:
        for again in range(2):
            y = torch.full_like(want, float("nan"))
            ops.conv2d(xs, prm, tile=tile, out=y, pad_value=pvs, x_split3=True)
            bad = y != want
            assert not bool(bad.any()), (A.probe_id(probe), tile, again, int(bad.sum()), bad.nonzero()[:4].tolist(), (y - want)[bad][:4].tolist())


# ---- engine ---------------------------------------------------------------------------------------------------------------------
class _Bottleneck(nn.Module):
    def __init__(self, cin, mid, dil):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(cin, mid, 1, bias=False), nn.BatchNorm2d(mid)
        self.conv2, self.bn2 = nn.Conv2d(mid, mid, 3, padding=dil, dilation=dil, bias=False), nn.BatchNorm2d(mid)
        self.conv3, self.bn3 = nn.Conv2d(mid, cin, 1, bias=False), nn.BatchNorm2d(cin)
        self.downsample = None
        for bn in (self.bn1, self.bn2, self.bn3):
            bn.running_mean.normal_(0, 0.1)
            bn.running_var.uniform_(0.5, 1.5)


class _Identity:
    def forward(self, y):
        return y


def _engines(dev):
    """-> [(name, forward(x) -> result)]: one layer3-like bottleneck (256 wide, dilation 2) and the purifier's p0 -> p3."""
    from pemp_amd import engine
    torch.manual_seed(5)
    trunk = engine._BottleneckTrunk()
    trunk.arena = engine.Arena(dev)
    bp = engine._BlockPlan(_Bottleneck(512, 256, 2).to(dev).eval())
    pur = engine.PurifierEngine.__new__(engine.PurifierEngine)
    pur.arena = engine.Arena(dev)
    pur.p0 = engine.conv_params(nn.Conv2d(512, 256, 3, padding=1).to(dev), None, relu=True)
    pur.p3 = engine.conv_params(nn.Conv2d(256, 256, 3, padding=1).to(dev), None, relu=True)
    pur.aspp = _Identity()
    return [("block", trunk.arena, lambda x: trunk._block(x, bp, "t")), ("purifier", pur.arena, pur.forward)]


def test_engine_results_do_not_depend_on_the_hand_over(hip_lib, dev, monkeypatch):
    from pemp_amd import engine, ops
    assert engine.SPLIT3
    monkeypatch.setattr(engine, "PRESPLIT_MIN_TILES", 0)          # 2178 rows are 18 tiles: below the engines' own threshold
    x = _rand(dev, 41, 2, 33, 33, 512)
    saved = dict(ops._TILE_CACHE)
    picks = {}
    try:
        for name, arena, fwd in _engines(dev):
            outs = {}
            for on in (True, False):
                monkeypatch.setattr(ops, "SPLIT3_PRESPLIT", on)
                ops._TILE_CACHE.clear()
                before = set(arena.bufs)
                monkeypatch.setattr(ops, "PICK_HOOK", lambda kind, cands, key: cands[-1])      # every pick is made and remembered
                outs[on] = fwd(x).clone()
                monkeypatch.setattr(ops, "PICK_HOOK", None)
                assert torch.equal(fwd(x), outs[on])                                            # ... and replayed
                picks[name, on] = dict(ops._TILE_CACHE)
                split_bufs = [k for k in set(arena.bufs) - before if k[2] == torch.bfloat16]      # the pre-split intermediate
                assert bool(split_bufs) == on, (name, on, list(arena.bufs))
            assert bool(outs[True].abs().sum() > 0) and torch.equal(outs[True], outs[False]), name
        for (name, on), cache in picks.items():
            pre = {k: t for k, t in cache.items() if t in ops.SPLIT3_PRESPLIT_TILES}
            assert bool(pre) == on, (name, on, cache)
            other = picks[name, not on]
            # a pick made on one path sits under a key the other path never asks for
            assert all(k not in other for k in pre), (name, on)
            assert all(146 in k[14:] for k in pre) and all(146 not in k[14:] for k in cache if k not in pre), (name, on, cache)
    finally:
        ops._TILE_CACHE.clear()
        ops._TILE_CACHE.update(saved)
