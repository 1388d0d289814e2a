"""Persistent split3 forms (conv_dma2.hip: ids 47 and 49, the shapes of 43 and 46 on a resident grid that walks the tiles) against
id 43, bit for bit: with and without a residual, ReLU, a per-image shift, a padding value, 1x1 and dilated 3x3 convs, row counts
that are not a multiple of the tile, and launches whose tile count is below the resident grid (one tile per block) and several
times above it for BOTH ids (every block walks several tiles: the next tile's offsets and step-0 DMA, the counted wait past the
stores, the buffer parity after 1, 2 and an odd number of K steps, tap masks and padding values of the next tile).  Which block
computes a tile, and when, must not change a single bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

PERSISTENT = (47, 49)


def _params(ops, w, shift, pad, dil, relu):
    packed, kpad = ops.pack_conv_weight(w)
    co, ci, kh, kw = w.shape
    packed = packed.contiguous()
    return ops.ConvParams(packed, None, shift, ci, co, kh, kw, 1, pad, dil, kpad, False, relu, ops.pack_split3(packed))


def _problem(dev, seed, N, H, W, cin, cout, k):
    g = torch.Generator(device=dev).manual_seed(seed)
    M = N * H * W
    buf = torch.empty(M + 4, cin, device=dev)              # the padding vector sits right behind the activations
    buf[:M] = torch.randn(M, cin, generator=g, device=dev)
    buf[M:] = torch.randn(cin, generator=g, device=dev)
    w = torch.randn(cout, cin, k, k, generator=g, device=dev) / (cin * k * k) ** 0.5
    res = torch.randn(N, H, W, cout, generator=g, device=dev)
    per_img = torch.randn(N, cout, generator=g, device=dev)
    return buf[:M].view(N, H, W, cin), buf[M], w, torch.randn(cout, generator=g, device=dev), res, per_img


# block shape of each persistent id
SHAPE = {47: (64, 64), 49: (256, 128)}


def _tiles(tile, M, cout):
    bm, bn = SHAPE[tile]
    return -(-M // bm) * (cout // bn)


def _grid_bound(dev, tile):
    """An upper bound of the launch's resident grid: CUs x the blocks whose LDS fits in one CU (160 KiB on gfx950); registers
    can only lower it."""
    bm, bn = SHAPE[tile]
    lds = 2 * (8 * bm + 12 * bn) * 16
    return torch.cuda.get_device_properties(dev).multi_processor_count * (160 * 1024 // lds)


# (N, H, W, cin, cout, k, dil): a few tiles, below the resident grid of both ids (one tile per block at most)
SMALL = [
    (1, 5, 7, 64, 128, 1, 1),          # M = 35: one partial row tile
    (2, 13, 11, 32, 256, 1, 1),        # one K step (Cin = 32)
    (2, 33, 29, 128, 256, 3, 2),       # dilated 3x3, zero padding / padding value
    (3, 51, 51, 64, 256, 1, 1),        # two K steps, M tail (7803 rows): 488 tiles of 47, 62 of 49
]
# several times the resident grid of BOTH ids (asserted below); M is never a multiple of 64 or 256 (tails)
LARGE = [
    (50, 51, 51, 32, 1024, 1, 1),      # one K step per tile: the next tile's step 0 goes out after the epilogue
    (50, 51, 51, 64, 1024, 1, 1),      # two K steps: step 0 of the next tile at the barrier of step 0
    (50, 51, 51, 96, 1024, 1, 1),      # three K steps: the stage buffer of step 0 flips from tile to tile
    (20, 51, 51, 32, 1024, 3, 2),      # dilated 3x3, nine K steps (odd), zero padding / padding value, M tail
    (20, 51, 51, 64, 1024, 3, 2),      # dilated 3x3, 18 K steps
]
GEOMS = SMALL + LARGE


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
def test_persistent_forms_match_id_43_bit_for_bit(hip_lib, dev, geom, residual):
    from pemp_amd import ops
    N, H, W, cin, cout, k, dil = geom
    if geom in LARGE:
        for tile in PERSISTENT:                 # every block of either id walks several tiles
            assert _tiles(tile, N * H * W, cout) >= 3 * _grid_bound(dev, tile), (tile, geom)
    x, pv, w, shift, res, per_img = _problem(dev, 41 + cin + cout + k, N, H, W, cin, cout, k)
    pad = dil if k == 3 else 0
    for relu in (False, True):
        p = _params(ops, w, shift, pad, dil, relu)
        cases = [dict(), dict(shift_override=per_img, per_image_shift=True)]
        if k == 3:
            cases.append(dict(pad_value=pv))
        for kw in cases:
            r = res if residual else None
            want = ops.conv2d(x, p, residual=r, tile=43, **kw)
            assert bool(want.abs().sum() > 0)
            for tile in PERSISTENT:
                if cout % ops._tile_bn(tile):
                    continue
                got = torch.full_like(want, float("nan"))
                ops.conv2d(x, p, residual=r, out=got, tile=tile, **kw)
                bad = got != want
                assert not bool(bad.any()), (tile, relu, sorted(kw), int(bad.sum()))


def test_persistent_forms_leave_the_rest_of_a_strided_output_alone(hip_lib, dev):
    """The output is a channel window of a wider buffer (ldy > Cout): the persistent walk writes that window and nothing else
    (every block walks several tiles)."""
    from pemp_amd import ops
    x, _, w, shift, res, _ = _problem(dev, 7, 50, 51, 51, 64, 256, 1)
    p = _params(ops, w, shift, 0, 1, True)
    want = ops.conv2d(x, p, residual=res, tile=43)
    for tile in PERSISTENT:
        assert _tiles(tile, 50 * 51 * 51, 256) >= 3 * _grid_bound(dev, tile), tile
        big = torch.full((50, 51, 51, 384), 7.0, device=dev)
        ops.conv2d(x, p, residual=res, out=big[..., 64:320], tile=tile)
        assert torch.equal(big[..., 64:320], want), tile
        assert bool((big[..., :64] == 7.0).all()) and bool((big[..., 320:] == 7.0).all()), tile
