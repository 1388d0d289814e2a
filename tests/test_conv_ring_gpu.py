"""The three-deep activation ring of the long-K 1x1 convs on the device (conv_ring.hip, tile id 349), bit for bit:

 * the fp32 output equals id 43's on the same inputs (torch.equal), the pre-split output equals the producer of id 49 byte for byte:
   K = 128 (four K steps: the ring just fills), 160, 256, 1024; Cout = 128, 256, 512; M = 40 (one partial tile), 256, 257, and a
   launch with several times more tiles than resident blocks (every block walks three or more tiles: the offsets exchanged under
   the last steps, the counted wait past the stores); stride 1 and 2; an input that is a channel window (ldx > Cin); affine, ReLU,
   a per-image shift; every launch twice;
 * an output that is a channel window of a wider buffer (ldy > Cout): the neighbouring channels and the guard rows behind M keep
   their bytes, and so do the rows behind a pre-split output;
 * what the entry refuses is refused on the device as on the CPU, and a call that names no id picks among candidates that include
   the id under a key of its own."""
import pytest
import torch

from tests.test_conv_ring_cpu import RING, library_refusals
from tests.test_conv_split3_presplit_gpu import _bits, _params, _rand

pytestmark = pytest.mark.gpu

SENTINEL = -3.0
# (N, H, W, Cin, Cout, stride, channels of the buffer x is a window of)
CASES = [(1, 5, 8, 128, 128, 1, 128),          # M = 40: one partial tile; four K steps
         (1, 16, 16, 160, 256, 1, 160),        # M = 256: one full row tile; five K steps
         (1, 1, 257, 256, 512, 1, 256),        # M = 257: a second row tile with one row
         (2, 13, 11, 1024, 128, 1, 1024),      # K = 1024, M = 286
         (3, 17, 19, 128, 256, 2, 128),        # stride 2: M = 3 x 9 x 10 = 270
         (2, 21, 15, 256, 128, 2, 320),        # stride 2, ldx > Cin
         (1, 16, 17, 160, 512, 1, 224)]        # ldx > Cin, M = 272
EPIS = ["plain", "affine", "relu", "affine-relu", "per-image", "per-image-relu"]


def _ids(c):
    return "x".join(map(str, c[:3])) + f"-{c[3]}-{c[4]}-s{c[5]}-ldx{c[6]}"


def _input(dev, seed, N, H, W, cin, ldx):
    buf = _rand(dev, seed, N, H, W, ldx)
    return buf[..., (ldx - cin):] if ldx > cin else buf


def _problem(ops, dev, case, epi):
    N, H, W, cin, cout, stride, ldx = case
    x = _input(dev, 3 + cin + W, N, H, W, cin, ldx)
    w = _rand(dev, 4 + cin + cout, cout, cin, 1, 1) / cin ** 0.5
    affine, relu, per_img = "affine" in epi, "relu" in epi, "per-image" in epi
    prm = _params(ops, w, stride, 0, 1, _rand(dev, 5, cout) if affine or per_img else None, _rand(dev, 6, cout) if affine else None, relu)
    kw = dict(shift_override=_rand(dev, 7, N, cout), per_image_shift=True) if per_img else {}
    return x, prm, kw, relu


@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_fp32_output_equals_id_43(hip_lib, dev, case, epi):
    from pemp_amd import ops
    x, prm, kw, relu = _problem(ops, dev, case, epi)
    want = ops.conv2d(x, prm, tile=43, **kw)
    assert bool(want.abs().sum() > 0) and bool((want < 0).any()) != relu
    for again in range(2):
        got = torch.full_like(want, float("nan"))
        ops.conv2d(x, prm, tile=RING, out=got, **kw)
        bad = got != want
        assert torch.equal(got, want), (again, int(bad.sum()), bad.nonzero()[:4].tolist())


@pytest.mark.parametrize("epi", ["plain", "affine-relu", "per-image"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_pre_split_output_equals_the_producer_of_id_49(hip_lib, dev, case, epi):
    from pemp_amd import ops
    x, prm, kw, _ = _problem(ops, dev, case, epi)
    N, _, _, _, cout, _, _ = case
    want = ops.conv2d(x, prm, tile=49, out_split3=True, **kw)
    assert bool((_bits(want) != 0).any())
    M = want.shape[0] * want.shape[1] * want.shape[2]
    for again in range(2):
        buf = torch.full((M * cout * 3 + 4096,), SENTINEL, dtype=torch.bfloat16, device=dev)
        out = buf[:M * cout * 3].view(want.shape)
        ops.conv2d(x, prm, tile=RING, out=out, out_split3=True, **kw)
        assert torch.equal(_bits(out), _bits(want)), again
        assert bool((buf[M * cout * 3:] == SENTINEL).all()), again                 # nothing behind row M - 1


@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[4], CASES[6]], ids=_ids)
def test_channel_window_of_a_wider_buffer(hip_lib, dev, case):
    from pemp_amd import ops
    x, prm, kw, _ = _problem(ops, dev, case, "affine-relu")
    want = ops.conv2d(x, prm, tile=43)
    N, Ho, Wo, cout = want.shape
    M, ld, c0 = N * Ho * Wo, cout + 96, 32
    for again in range(2):
        buf = torch.full((M * ld + 4096,), SENTINEL, device=dev)
        wide = buf[:M * ld].view(N, Ho, Wo, ld)
        ops.conv2d(x, prm, tile=RING, out=wide[..., c0:c0 + cout])
        assert torch.equal(wide[..., c0:c0 + cout], want), again
        assert bool((wide[..., :c0] == SENTINEL).all()) and bool((wide[..., c0 + cout:] == SENTINEL).all()) and bool((buf[M * ld:] == SENTINEL).all())


@pytest.mark.parametrize("cin", [128, 160])
def test_blocks_walk_several_tiles(hip_lib, dev, cin):
    """tests/test_conv_split3_persist_gpu.py's LARGE row count: several times more tiles than resident blocks (one 144 KiB block per CU),
    so that every block exchanges its offsets and runs the tile-to-tile hand-over three times or more; M is no multiple of 256."""
    from pemp_amd import ops
    N, H, W, cout = 50, 51, 51, 256
    assert -(-N * H * W // 256) * (cout // 128) >= 3 * torch.cuda.get_device_properties(dev).multi_processor_count
    x = _rand(dev, 9 + cin, N, H, W, cin)
    prm = _params(ops, _rand(dev, 10, cout, cin, 1, 1) / cin ** 0.5, 1, 0, 1, _rand(dev, 11, cout), _rand(dev, 12, cout), True)
    want = ops.conv2d(x, prm, tile=43)
    want3 = _bits(ops.conv2d(x, prm, tile=49, out_split3=True))
    assert bool(want.abs().sum() > 0)
    M = N * H * W
    for again in range(2):
        got = torch.full_like(want, float("nan"))
        ops.conv2d(x, prm, tile=RING, out=got)
        bad = got != want
        assert torch.equal(got, want), (again, int(bad.sum()), bad.nonzero()[:4].tolist())
        buf = torch.full((M * cout * 3 + 4096,), SENTINEL, dtype=torch.bfloat16, device=dev)
        out = buf[:M * cout * 3].view(ops.split3_shape(N, H, W, cout))
        ops.conv2d(x, prm, tile=RING, out=out, out_split3=True)
        assert torch.equal(_bits(out), want3) and bool((buf[M * cout * 3:] == SENTINEL).all()), again


def test_refusals_on_the_device_and_the_pick(hip_lib, dev, monkeypatch):
    from pemp_amd import ops
    monkeypatch.setattr(ops, "SPLIT3_RING", True)
    monkeypatch.setattr(ops, "PICK_HOOK", None)
    for what, rc, msg in library_refusals(hip_lib):
        assert rc == -1 and msg, (what, rc, msg)
    # three K steps: the id is an error, a call that names no id runs another one under a key without the suffix
    few = _params(ops, _rand(dev, 22, 128, 96, 1, 1) / 96 ** 0.5, 1, 0, 1)
    x96 = _rand(dev, 21, 2, 20, 13, 96)
    with pytest.raises(Exception, match="unsupported"):
        ops.conv2d(x96, few, tile=RING)
    with pytest.raises(Exception, match="unsupported"):
        ops.conv2d(x96, _params(ops, _rand(dev, 23, 128, 96, 3, 3) / 30, 1, 1, 1), tile=RING)
    x, prm, _, _ = _problem(ops, dev, CASES[3], "affine-relu")
    with pytest.raises(Exception, match="unsupported"):
        ops.conv2d(x, prm, tile=RING, residual=ops.conv2d(x, prm, tile=43))
    saved = dict(ops._TILE_CACHE)
    try:
        monkeypatch.setattr(ops, "_tunes", lambda rows, least=0: True)
        ops._TILE_CACHE.clear()
        assert torch.equal(ops.conv2d(x96, few), ops.conv2d(x96, few, tile=43))
        assert all(RING not in k and t != RING for k, t in ops._TILE_CACHE.items())
        # ... and where the id applies, a timing-based pick is made among candidates that include it, under a key of its own
        ops._TILE_CACHE.clear()
        assert torch.equal(ops.conv2d(x, prm), ops.conv2d(x, prm, tile=43))
        (key, tile), = ops._TILE_CACHE.items()
        assert RING in key and tile in ops.SPLIT3_TILES + ops.SPLIT3_RING_TILES + ops.SPLIT3_PANEL_TILES
        # the same call with a residual: a key of its own, never the id
        ops._TILE_CACHE.clear()
        res = _rand(dev, 24, *ops.conv2d(x, prm, tile=43).shape)
        assert torch.equal(ops.conv2d(x, prm, residual=res), ops.conv2d(x, prm, residual=res, tile=43))
        (key, tile), = ops._TILE_CACHE.items()
        assert RING not in key and tile != RING
    finally:
        ops._TILE_CACHE.clear()
        ops._TILE_CACHE.update(saved)
