"""The row-stage forms of the pre-split 3x3 convs on the device (conv_row3.hip, tile ids 246 / 249), bit for bit:

 * ids 246 / 249 equal id 146 on the same pre-split tensor and id 43 on the fp32 tensor -- one partial tile, tiles that start mid-row and
   cross image boundaries, the headline geometries (many tiles), a stage close to the capacity limit; with and without affine /
   ReLU; into a channel window of a wider buffer, nothing else written; every launch twice;
 * exact edge probes: one non-zero pixel on an image's border, weights that select one tap, integer values -- every id gives the
   float64 result exactly, so a leak across a row or image boundary shows as a wrong integer;
 * what the entry refuses is refused on the device as on the CPU, and ops.conv2d keeps such a call on 146 / 149."""
import pytest
import torch

from tests.test_conv_row3_cpu import library_refusals
from tests.test_conv_split3_presplit_cpu import presplit
from tests.test_conv_split3_presplit_gpu import _params, _rand

pytestmark = pytest.mark.gpu

ROW3 = (246, 249)
SENTINEL = -3.0
# (N, H, W, Cin, Cout, d)
CASES = [(1, 7, 9, 32, 128, 1),        # one partial tile, one chunk
         (3, 11, 17, 64, 128, 1),      # tiles that start mid-row and cross image boundaries, M tail
         (2, 51, 51, 256, 256, 2),     # the headline geometry (layer3 conv2): 21 row tiles
         (2, 51, 51, 128, 128, 1),     # layer2's
         (2, 30, 40, 96, 256, 3)]      # 283 of 288 stage rows


def _ids(c):
    return "x".join(map(str, c[:3])) + f"-{c[3]}-{c[4]}-d{c[5]}"


@pytest.mark.parametrize("epi", ["plain", "affine", "relu", "affine-relu"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_equals_id_146_and_id_43(hip_lib, dev, case, epi):
    from pemp_amd import ops
    N, H, W, cin, cout, d = case
    assert ops.row3_stage_rows(W, d) <= ops.ROW3_STAGE_ROWS
    x = _rand(dev, 3 + cin + W, N, H, W, cin)
    xs = presplit(x)
    w = _rand(dev, 4 + cin + cout, cout, cin, 3, 3) / (cin * 9) ** 0.5
    affine, relu = "affine" in epi, "relu" in epi
    prm = _params(ops, w, 1, d, d, _rand(dev, 5, cout) if affine else None, _rand(dev, 6, cout) if affine else None, relu)
    want = ops.conv2d(x, prm, tile=43)
    assert bool(want.abs().sum() > 0) and bool((want < 0).any()) != relu
    assert torch.equal(ops.conv2d(xs, prm, tile=146, x_split3=True), want)
    for tile in ROW3:
        for again in range(2):
            got = torch.full_like(want, float("nan"))
            ops.conv2d(xs, prm, tile=tile, out=got, x_split3=True)
            bad = got != want
            assert not bool(bad.any()), (tile, again, int(bad.sum()), bad.nonzero()[:4].tolist())


def test_persistent_blocks_walk_several_tiles(hip_lib, dev):
    """test_conv_split3_presplit_gpu.py's LARGE shape: several times more tiles than resident blocks, so that every block of id 249
    exchanges its offsets and runs the tile-to-tile hand-over (the cases above have fewer tiles than the chip has CUs)."""
    from pemp_amd import ops
    N, H, W, cin, cout, d = 20, 51, 51, 32, 1024, 2
    assert -(-N * H * W // 256) * (cout // 128) >= 3 * torch.cuda.get_device_properties(dev).multi_processor_count
    x = _rand(dev, 9, N, H, W, cin)
    xs = presplit(x)
    prm = _params(ops, _rand(dev, 10, cout, cin, 3, 3) / (cin * 9) ** 0.5, 1, d, d, _rand(dev, 11, cout), _rand(dev, 12, cout), True)
    want = ops.conv2d(xs, prm, tile=146, x_split3=True)
    assert bool(want.abs().sum() > 0)
    for tile in ROW3 * 2:
        got = torch.full_like(want, float("nan"))
        ops.conv2d(xs, prm, tile=tile, out=got, x_split3=True)
        bad = got != want
        assert not bool(bad.any()), (tile, int(bad.sum()), bad.nonzero()[:4].tolist())


@pytest.mark.parametrize("case", [CASES[1], CASES[4]], ids=_ids)
def test_channel_window_of_a_wider_buffer(hip_lib, dev, case):
    from pemp_amd import ops
    N, H, W, cin, cout, d = case
    x = _rand(dev, 11, N, H, W, cin)
    xs = presplit(x)
    prm = _params(ops, _rand(dev, 12, cout, cin, 3, 3) / (cin * 9) ** 0.5, 1, d, d, _rand(dev, 13, cout), _rand(dev, 14, cout), True)
    want = ops.conv2d(x, prm, tile=43)
    M, ld, c0 = N * H * W, cout + 96, 32
    for tile in ROW3 * 2:
        buf = torch.full((M * ld + 1024,), SENTINEL, device=dev)
        wide = buf[:M * ld].view(N, H, W, ld)
        ops.conv2d(xs, prm, tile=tile, out=wide[..., c0:c0 + cout], x_split3=True)
        assert torch.equal(wide[..., c0:c0 + cout], want), tile
        assert bool((wide[..., :c0] == SENTINEL).all()) and bool((wide[..., c0 + cout:] == SENTINEL).all()) and bool((buf[M * ld:] == SENTINEL).all())


@pytest.mark.parametrize("d", [1, 2])
def test_edge_probes_are_exact_on_every_id(hip_lib, dev, d):
    """One non-zero pixel, one tap: out[n, h, w, co] = x[n, h + (kh - 1) d, w + (kw - 1) d, :] . w[co, :, kh, kw] where that pixel is
    the probe, zero elsewhere -- integers below 2^24, values that need all three bf16 pieces."""
    from pemp_amd import ops
    N, H, W, cin, cout = 2, 6, {1: 9, 2: 19}[d], 32, 128        # the narrowest maps whose stage fits: the most row boundaries per tile
    assert ops.row3_stage_rows(W, d) <= ops.ROW3_STAGE_ROWS < ops.row3_stage_rows(W - 1, d)
    c = torch.arange(cin)
    pix = torch.where(c % 2 == 0, torch.tensor(65793.0), (c % 7 + 1).float())         # 65793 = 2^16 + 2^8 + 1: h, m and l
    wv = ((torch.arange(cout)[:, None] + c[None, :]) % 5 - 2).float()                   # [cout, cin]
    assert float((wv.abs() @ pix).max()) < 2 ** 24
    # column 0, column W - 1, the first and the last row of an image -- of the first and of the second image (an image boundary
    # is a row boundary: the last row of image 0 sits against the first row of image 1)
    probes = [(0, 2, 0), (0, 3, W - 1), (0, 0, 3), (0, H - 1, 3), (1, 0, 0), (0, H - 1, W - 1), (1, 0, W - 1), (0, H - 1, 0), (1, H - 1, W - 1)]
    for n, h, wc in probes:
        x = torch.zeros(N, H, W, cin)
        x[n, h, wc] = pix
        xd, xs = x.to(dev), presplit(x).to(dev)
        for kh in range(3):
            for kw in range(3):
                w = torch.zeros(cout, cin, 3, 3)
                w[:, :, kh, kw] = wv
                ref = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), padding=d, dilation=d).permute(0, 2, 3, 1)
                want = ref.float()
                assert torch.equal(want.double(), ref)
                hh, ww = h - (kh - 1) * d, wc - (kw - 1) * d                            # the one output pixel that sees the probe
                assert int((want.abs().sum(-1) > 0).sum()) == int(0 <= hh < H and 0 <= ww < W)
                want = want.to(dev)
                prm = _params(ops, w.to(dev), 1, d, d)
                for tile in (43, 146, 149) + ROW3:
                    got = torch.full_like(want, float("nan"))
                    if tile == 43:
                        ops.conv2d(xd, prm, tile=tile, out=got)
                    else:
                        ops.conv2d(xs, prm, tile=tile, out=got, x_split3=True)
                    bad = got != want
                    assert not bool(bad.any()), ((n, h, wc), (kh, kw), tile, bad.nonzero()[:4].tolist(), got[bad][:4].tolist())


def test_refusals_on_the_device_and_the_fall_back(hip_lib, dev, monkeypatch):
    from pemp_amd import ops
    monkeypatch.setattr(ops, "SPLIT3_ROW3", True)
    for tile in ROW3:
        for what, rc, msg in library_refusals(hip_lib, tile):
            assert rc == -1 and msg, (tile, what, rc, msg)
    # a geometry that needs more than 288 stage rows: the id is an error, a call that names no id runs 146 / 149
    N, H, W, cin, cout, d = 2, 20, 13, 64, 128, 2
    assert ops.row3_stage_rows(W, d) > ops.ROW3_STAGE_ROWS
    x = _rand(dev, 21, N, H, W, cin)
    xs = presplit(x)
    prm = _params(ops, _rand(dev, 22, cout, cin, 3, 3) / (cin * 9) ** 0.5, 1, d, d)
    want = ops.conv2d(x, prm, tile=43)
    for tile in ROW3:
        with pytest.raises(Exception, match="unsupported"):
            ops.conv2d(xs, prm, tile=tile, x_split3=True)
    saved = dict(ops._TILE_CACHE)
    try:
        for least in (1 << 30, 0):                       # the default id; a timing-based pick
            ops._TILE_CACHE.clear()
            monkeypatch.setattr(ops, "_tunes", lambda rows, least=least: rows >= least)
            assert torch.equal(ops.conv2d(xs, prm, x_split3=True), want)
            assert all(t in ops.SPLIT3_PRESPLIT_TILES for t in ops._TILE_CACHE.values()) and all(k[-1] != 246 for k in ops._TILE_CACHE)
        # ... and where the id applies, a timing-based pick is made among 146 / 149 / 246 / 249 under a key of its own
        N, H, W, cin, cout, d = CASES[1]
        x = _rand(dev, 23, N, H, W, cin)
        prm = _params(ops, _rand(dev, 24, cout, cin, 3, 3) / (cin * 9) ** 0.5, 1, d, d)
        ops._TILE_CACHE.clear()
        assert torch.equal(ops.conv2d(presplit(x), prm, x_split3=True), ops.conv2d(x, prm, tile=43))
        (key, tile), = ops._TILE_CACHE.items()
        assert key[-1] == 246 and tile in ops.SPLIT3_PRESPLIT_TILES + ops.SPLIT3_ROW3_TILES
    finally:
        ops._TILE_CACHE.clear()
        ops._TILE_CACHE.update(saved)
