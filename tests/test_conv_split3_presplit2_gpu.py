"""Pre-split hand-over, second round, on the device -- bit for bit:

 * persistent producers: ids 47 / 49 (conv_dma2_s3po_kernel) and 149 (conv_dma2_a3po_kernel) with ``out_split3`` write the reference
   split (tests/test_conv_split3_presplit_cpu.py: presplit) of what id 43 writes as fp32 -- twice, into a sentinel-filled buffer, and
   nothing behind it; one launch whose blocks walk several tiles;
 * dual output: ids 146 / 149 with ``also_split3`` write the fp32 tensor of id 43 -- as a channel window of a wider buffer -- and its
   split, and leave the spare rows behind both alone; the entry refuses what the header says it refuses;
 * chain: p3 with both outputs feeds three dilated 3x3 convs with their own padding vectors (split copy) and a 1x1 (fp32 copy):
   the concatenated result equals the fp32 path's, eager and from a graph replayed over poisoned buffers;
 * engine: stage-1 ``lowres`` gives the same outputs with the hand-over on and off, and the new path is taken when it is on."""
import pytest
import torch

from tests import util
from tests.test_conv_split3_presplit_cpu import presplit, unsplit
from tests.test_conv_split3_presplit2_cpu import library_refusals
from tests.test_conv_split3_presplit_gpu import SENTINEL, _activations, _bits, _params, _rand

pytestmark = pytest.mark.gpu

SIZES = {234: (2, 9, 13), 1305: (5, 9, 29)}


def _split_sentinel(dev, M, cout, spare=256):
    buf = torch.full((M * cout * 3 + spare,), SENTINEL, dtype=torch.bfloat16, device=dev)
    return buf, buf[:M * cout * 3]


# ---- persistent producers ---------------------------------------------------------------------------------------------------------
def _producer_check(ops, dev, x, xs, prm, tiles, **kw):
    """``out_split3`` on each of ``tiles`` (149 reads ``xs``) against the split of id 43's fp32 output on ``x``."""
    y = ops.conv2d(x, prm, tile=43, **kw)
    N, H, W, cout = y.shape
    M = N * H * W
    assert bool(y.abs().sum() > 0) and bool((y < 0).any()) != prm.relu
    want = _bits(presplit(y))
    for tile in tiles:
        for again in range(2):
            buf, body = _split_sentinel(dev, M, cout)
            out = body.view(ops.split3_shape(N, H, W, cout))
            src = xs if tile == 149 else x
            assert ops.conv2d(src, prm, tile=tile, out=out, out_split3=True, x_split3=tile == 149, **kw) is out
            bad = _bits(out) != want
            assert not bool(bad.any()), (tile, again, int(bad.sum()), bad.nonzero()[:4].tolist())
            assert torch.equal(_bits(unsplit(out)), _bits(y)), (tile, again)
            assert bool((buf[M * cout * 3:] == SENTINEL).all()), (tile, again)


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("M", sorted(SIZES))
@pytest.mark.parametrize("cout", [128, 256])
@pytest.mark.parametrize("cin", [32, 64, 256])
def test_persistent_producers_write_the_split_of_id_43(hip_lib, dev, cin, cout, M, relu):
    from pemp_amd import ops
    N, H, W = SIZES[M]
    x, _, xs, _ = _activations(dev, 50 + cin + M, N, H, W, cin, False)
    w3 = _rand(dev, 51 + cin + cout, cout, cin, 3, 3) / (cin * 9) ** 0.5
    scale, shift = _rand(dev, 52, cout).abs() + 0.5, _rand(dev, 53, cout)
    _producer_check(ops, dev, x, xs, _params(ops, w3, 1, 1, 1, scale, shift, relu), (47, 49, 149))
    # the layer the engines run this way: a 1x1 conv (no pre-split input form)
    w1 = _rand(dev, 54 + cin + cout, cout, cin, 1, 1) / cin ** 0.5
    _producer_check(ops, dev, x, None, _params(ops, w1, 1, 0, 1, scale, shift, relu), (47, 49))


def test_persistent_producers_with_a_per_image_shift(hip_lib, dev):
    from pemp_amd import ops
    N, H, W, cin, cout = 5, 9, 29, 64, 128
    x = _rand(dev, 55, N, H, W, cin)
    prm = _params(ops, _rand(dev, 56, cout, cin, 1, 1) / 8, 1, 0, 1, _rand(dev, 57, cout), None, relu=True)
    _producer_check(ops, dev, x, None, prm, (47, 49), shift_override=_rand(dev, 58, N, cout), per_image_shift=True)


def test_persistent_producers_walk_several_tiles(hip_lib, dev):
    """tests/test_conv_split3_presplit_gpu.py's LARGE shape: several times more tiles than resident blocks, a padding vector."""
    from pemp_amd import ops
    N, H, W, cin, cout, k, dil = 20, 51, 51, 32, 1024, 3, 2
    tiles = -(-N * H * W // 256) * (cout // 128)
    assert tiles >= 3 * torch.cuda.get_device_properties(dev).multi_processor_count
    x, pv, xs, pvs = _activations(dev, 59, N, H, W, cin, True)
    prm = _params(ops, _rand(dev, 60, cout, cin, k, k) / (cin * k * k) ** 0.5, 1, dil, dil, _rand(dev, 61, cout), _rand(dev, 62, cout), relu=True)
    M = N * H * W
    want = _bits(presplit(ops.conv2d(x, prm, tile=43, pad_value=pv)))
    for tile in (47, 49, 149):
        buf, body = _split_sentinel(dev, M, cout)
        out = body.view(ops.split3_shape(N, H, W, cout))
        ops.conv2d(xs if tile == 149 else x, prm, tile=tile, out=out, out_split3=True, x_split3=tile == 149, pad_value=pvs if tile == 149 else pv)
        assert torch.equal(_bits(out), want), tile
        assert bool((buf[M * cout * 3:] == SENTINEL).all()), tile


def test_the_persistent_ids_are_offered_to_a_producer_pick(hip_lib, dev, monkeypatch):
    from pemp_amd import ops
    x = _rand(dev, 63, 2, 9, 13, 64)
    prm = _params(ops, _rand(dev, 64, 128, 64, 1, 1) / 8, 1, 0, 1)
    seen = {}
    saved = dict(ops._TILE_CACHE)
    monkeypatch.setattr(ops, "PICK_HOOK", lambda kind, cands, key: seen.setdefault(key, list(cands))[-1])
    try:
        ops._TILE_CACHE.clear()
        plain = ops.conv2d(x, prm)
        split = ops.conv2d(x, prm, out_split3=True)
        (k_plain, c_plain), (k_split, c_split) = sorted(seen.items(), key=lambda kc: len(kc[0]))
        assert c_split == list(ops.SPLIT3_TILES) and {47, 49} <= set(c_split)
        # a key of its own, and not the one picks were remembered under while 47 / 49 ran as 43 / 46 and were not offered
        assert k_split[:len(k_plain)] == k_plain and k_split[len(k_plain):] == (17,)
        assert ops._TILE_CACHE[k_split] == 49
        assert torch.equal(_bits(split), _bits(presplit(plain)))
    finally:
        ops._TILE_CACHE.clear()
        ops._TILE_CACHE.update(saved)


# ---- dual output ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padv", [False, True], ids=["zeros", "padv"])
@pytest.mark.parametrize("M", sorted(SIZES))
def test_dual_output_writes_id_43s_tensor_and_its_split(hip_lib, dev, M, padv):
    from pemp_amd import ops
    N, H, W = SIZES[M]
    cin, cout, wide, off, spare = 64, 128, 384, 128, 8
    x, pv, xs, pvs = _activations(dev, 70 + M, N, H, W, cin, padv)
    prm = _params(ops, _rand(dev, 71, cout, cin, 3, 3) / (cin * 9) ** 0.5, 1, 1, 1, _rand(dev, 72, cout), _rand(dev, 73, cout), relu=True)
    want = ops.conv2d(x, prm, tile=43, pad_value=pv)
    assert bool(want.abs().sum() > 0)
    want_s = _bits(presplit(want))
    for tile in (146, 149):
        for again in range(2):
            ybuf = torch.full((M + spare, wide), SENTINEL, device=dev)
            y = ybuf[:M, off:off + cout].view(N, H, W, cout)              # a channel window: ldy != Cout
            sbuf = torch.full((M + spare, cout // 32, 3, 32), SENTINEL, dtype=torch.bfloat16, device=dev)
            ys = sbuf[:M].view(ops.split3_shape(N, H, W, cout))
            assert ops.conv2d(xs, prm, tile=tile, out=y, pad_value=pvs, x_split3=True, also_split3=ys) is y
            assert torch.equal(_bits(y), _bits(want)), (tile, again)
            assert torch.equal(_bits(ys), want_s), (tile, again)
            assert bool((ybuf[M:] == SENTINEL).all()) and bool((ybuf[:M, :off] == SENTINEL).all()) and bool((ybuf[:M, off + cout:] == SENTINEL).all())
            assert bool((sbuf[M:] == SENTINEL).all()), (tile, again)


def test_dual_output_refusals(hip_lib, dev):
    from pemp_amd import ops
    for what, rc in library_refusals(hip_lib):
        assert rc == -1, what
    # overlapping outputs of real tensors
    N, H, W, cin, cout = 2, 9, 13, 64, 128
    x, _, xs, _ = _activations(dev, 74, N, H, W, cin, False)
    prm = _params(ops, _rand(dev, 75, cout, cin, 3, 3) / 24, 1, 1, 1)
    from pemp_amd._lib import PempHipError
    M = N * H * W
    raw = torch.zeros(M * cout * 3, dtype=torch.bfloat16, device=dev)
    ys = raw.view(ops.split3_shape(N, H, W, cout))
    y = raw.view(torch.float32)[:M * cout].view(N, H, W, cout)          # the first two thirds of the same bytes
    for tile in (146, 149):
        with pytest.raises(PempHipError):
            ops.conv2d(xs, prm, tile=tile, out=y, x_split3=True, also_split3=ys)
    assert not bool(raw.view(torch.int16).any())                        # nothing was launched


# ---- chain ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nhw", [(5, 9, 29), (2, 13, 17)], ids=["M1305", "M442"])
def test_aspp_chain_equals_the_fp32_path_eager_and_replayed(hip_lib, dev, nhw):
    from pemp_amd import ops
    N, H, W = nhw
    M, cin, c, midc, dils = N * H * W, 64, 128, 128, (6, 12, 18)
    x, _, xs, _ = _activations(dev, 80 + M, N, H, W, cin, False)
    p3 = _params(ops, _rand(dev, 81, c, cin, 3, 3) / (cin * 9) ** 0.5, 1, 1, 1, None, _rand(dev, 82, c), relu=True)
    b1 = _params(ops, _rand(dev, 83, midc, c, 1, 1) / c ** 0.5, 1, 0, 1, None, _rand(dev, 84, midc))
    bd = [_params(ops, _rand(dev, 85 + d, midc, c, 3, 3) / (c * 9) ** 0.5, 1, d, d, None, _rand(dev, 86 + d, midc)) for d in dils]
    pvecs = [_rand(dev, 87 + d, c) for d in dils]                       # one padding vector per branch

    # the fp32 path: p3 -> y (+ the vectors in the spare rows behind it) -> four branches into the concat buffer
    flat = torch.zeros(M + 8, c, device=dev)
    for i, v in enumerate(pvecs):
        flat[M + i].copy_(v)
    y = flat[:M].view(N, H, W, c)
    want = torch.zeros(N, H, W, 4 * midc, device=dev)
    ops.conv2d(x, p3, tile=43, out=y)
    ops.conv2d(y, b1, tile=43, out=want[..., :midc])
    for i, p in enumerate(bd):
        ops.conv2d(y, p, tile=43, out=want[..., (i + 1) * midc:(i + 2) * midc], pad_value=flat[M + i])
    assert all(bool(want[..., i * midc:(i + 1) * midc].abs().sum() > 0) for i in range(4))
    y_want = y.clone()

    # the new path: p3 writes both forms, the dilated branches read the split one with split vectors behind it
    flat2 = torch.zeros(M + 8, c, device=dev)
    y2 = flat2[:M].view(N, H, W, c)
    flat_s = torch.zeros(M + 8, c // 32, 3, 32, dtype=torch.bfloat16, device=dev)
    ys = flat_s[:M].view(ops.split3_shape(N, H, W, c))
    for i, v in enumerate(pvecs):
        flat_s[M + i].copy_(ops.pack_split3(v.view(1, c))[0])
        assert torch.equal(_bits(flat_s[M + i]), _bits(presplit(v.view(1, 1, 1, c)).view(c // 32, 3, 32)))
    got = torch.zeros_like(want)

    def run(t_p3, t_br):
        ops.conv2d(xs, p3, tile=t_p3, out=y2, x_split3=True, also_split3=ys)
        ops.conv2d(y2, b1, tile=43, out=got[..., :midc])
        for i, p in enumerate(bd):
            ops.conv2d(ys, p, tile=t_br, out=got[..., (i + 1) * midc:(i + 2) * midc], pad_value=flat_s[M + i], x_split3=True)

    def poison():
        flat2[:M].fill_(float("nan"))
        flat_s[:M].fill_(float("nan"))
        got.fill_(float("nan"))

    for t_p3, t_br in ((146, 146), (149, 149), (146, 149)):
        poison()
        run(t_p3, t_br)
        assert torch.equal(_bits(y2), _bits(y_want)) and torch.equal(_bits(ys), _bits(presplit(y_want))), (t_p3, t_br)
        assert torch.equal(_bits(got), _bits(want)), (t_p3, t_br)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(149, 149)
    poison()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(ys), _bits(presplit(y_want)))


# ---- engine -----------------------------------------------------------------------------------------------------------------------
def test_stage1_lowres_does_not_depend_on_the_hand_over(hip_lib, dev, monkeypatch):
    from pemp_amd import engine, ops, synth
    from pemp_amd.networks import pemp_stage1 as m
    assert engine.SPLIT3 and engine.PRESPLIT_ASPP
    monkeypatch.setattr(engine, "PRESPLIT_MIN_TILES", 0)          # two 97 x 97 episodes: a few tiles, below the engines' own threshold
    net = m.ModelClass(None)
    net.load_state_dict(util.wgen_state_dict("stage1_rn50"))
    net = net.to(dev).eval()
    b = synth.make_batch([4321, 4322], shot=1, height=97, width=97, out_hw=(97, 97))
    t = lambda k_: torch.from_numpy(b[k_]).to(dev)
    sup, msk, qry = t("sup_img"), t("sup_mask"), t("qry_img")
    calls = []
    conv2d = ops.conv2d

    def spy(x, p, **kw):
        calls.append((bool(kw.get("x_split3")), bool(kw.get("out_split3")), kw.get("also_split3") is not None, p.kh * p.kw))
        return conv2d(x, p, **kw)

    monkeypatch.setattr(ops, "conv2d", spy)
    saved = dict(ops._TILE_CACHE)
    outs = {}
    try:
        with torch.no_grad():
            for on in (True, False):
                monkeypatch.setattr(ops, "SPLIT3_PRESPLIT", on)
                ops._TILE_CACHE.clear()
                del calls[:]
                outs[on] = [o.clone() for o in net.lowres(sup, msk, qry) if o is not None]
                also = [i for i, c in enumerate(calls) if c[2]]
                if on:      # p3 wrote both forms once; behind it the three dilated branches, and nothing else, read the split one
                    assert len(also) == 1 and calls[also[0]][0], calls
                    assert [c[3] for c in calls[also[0] + 1:] if c[0]] == [9, 9, 9], calls
                else:
                    assert not also and not any(c[0] or c[1] for c in calls), calls
    finally:
        ops._TILE_CACHE.clear()
        ops._TILE_CACHE.update(saved)
    assert len(outs[True]) == len(outs[False]) and bool(outs[True][0].abs().sum() > 0)
    for a, c in zip(outs[True], outs[False]):
        assert torch.equal(a, c)
