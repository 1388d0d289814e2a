"""The statistics epilogue on the split3 family (pemp_split3_conv2d_stats_nhwc_f32 through ops.conv2d_stats with ConvParams.w3):
z is the plain split3 conv of the same id bit for bit, the partial rows are the per-row-tile sums of z and z^2 in a fixed order,
and a BatchNorm finished from them is the BatchNorm of z.

Geometries: the smallest that reach every row-tile case of BM = 64, 128, 256 -- a partial last tile for each, one tile shorter
than every BM, a strided + dilated conv, and a conv whose every tap is partly out of the image with one K step per tap."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GEOMS = [  # N, H, W, Cin, Cout, k, stride, pad, dil
    (2, 13, 13, 64, 256, 3, 1, 1, 1),       # M = 338: the last tile is partial for BM 64, 128 and 256
    (1, 7, 9, 64, 128, 1, 1, 0, 1),         # M = 63: one tile, shorter than every BM
    (2, 21, 21, 128, 64, 3, 2, 2, 2),       # M = 242: strided and dilated; the 64-wide ids only
    (3, 9, 9, 32, 128, 3, 1, 6, 6),         # M = 243: every tap partly out of the image; one K step per tap
]
_CACHE = {}


def _ids(ops, cout):
    ids = ops.split3_stats_tiles(cout)
    assert ids and set(ids) <= {41, 42, 43, 44, 46}
    return ids


def _case(dev, geom, ints):
    """(x NHWC on the device, ConvParams with w3, float64 conv [M, Cout] on the CPU) -- computed once per case and left unchanged."""
    key = (geom, ints)
    if key not in _CACHE:
        from pemp_amd import ops
        N, H, W, Cin, Cout, k, s, p, d = geom
        g = torch.Generator().manual_seed(11)
        if ints:
            x = torch.randint(-2, 3, (N, Cin, H, W), generator=g).float()
            w = torch.randint(-1, 2, (Cout, Cin, k, k), generator=g).float()
        else:
            x = torch.randn(N, Cin, H, W, generator=g)
            w = torch.randn(Cout, Cin, k, k, generator=g) * (Cin * k * k) ** -0.5
        z64 = F.conv2d(x.double(), w.double(), None, s, p, d).permute(0, 2, 3, 1).reshape(-1, Cout)
        packed, kpad = ops.pack_conv_weight(w.to(dev))
        prm = ops.ConvParams(packed.contiguous(), None, None, Cin, Cout, k, k, s, p, d, kpad, False, False)
        prm.w3 = ops.pack_split3(prm.w)
        _CACHE[key] = (x.permute(0, 2, 3, 1).contiguous().to(dev), prm, z64)
    return _CACHE[key]


def _tile_sums(t, bm):
    """[M, C] float64 -> [row tiles of bm rows, C] column sums; rows beyond M contribute nothing."""
    M, C = t.shape
    return torch.cat([t, torch.zeros((-M) % bm, C, dtype=torch.float64)]).view(-1, bm, C).sum(1)


@pytest.mark.parametrize("geom", GEOMS)
def test_integer_probes_are_exact(hip_lib, dev, geom):
    """Small integers: every product, every K sum and every row-tile sum is exact in fp32 whatever the order, so z and both
    partial planes must EQUAL float64."""
    from pemp_amd import ops
    x, prm, z64 = _case(dev, geom, True)
    M, Cout = z64.shape
    for bm in (64, 128, 256):       # the premise: every row tile's sums stay below 2^24
        assert float(_tile_sums(z64.abs(), bm).max()) < 2 ** 24 and float(_tile_sums(z64 * z64, bm).max()) < 2 ** 24
    assert ops.stats_supported(x, prm)
    for tile in _ids(ops, Cout):
        bm = ops.tile_shape(tile)[0]
        z, part = ops.conv2d_stats(x, prm, tile=tile)
        assert part.shape == ((M + bm - 1) // bm, 2, Cout) and part.is_contiguous(), tile
        assert torch.equal(z.reshape(M, Cout).double().cpu(), z64), tile
        assert torch.equal(part[:, 0].double().cpu(), _tile_sums(z64, bm)), tile
        assert torch.equal(part[:, 1].double().cpu(), _tile_sums(z64 * z64, bm)), tile


@pytest.mark.parametrize("geom", GEOMS)
def test_random_data_z_is_the_plain_split3_conv_and_the_partials_are_its_sums(hip_lib, dev, geom):
    """z bit-identical to ops.conv2d of the same id; against float64 sums of that z per row tile, the forward bounds of a
    length-BM fp32 sum (BM * 2^-24 * sum |z|) and of one more rounding per square ((BM + 1) * 2^-24 * sum z^2)."""
    from pemp_amd import ops
    x, prm, z64 = _case(dev, geom, False)
    M, Cout = z64.shape
    u = 2.0 ** -24
    for tile in _ids(ops, Cout):
        bm = ops.tile_shape(tile)[0]
        z, part = ops.conv2d_stats(x, prm, tile=tile)
        z_plain = ops.conv2d(x, prm, tile=tile)
        assert torch.equal(z, z_plain), tile
        assert (z.reshape(M, Cout).double().cpu() - z64).abs().max() <= 1e-5 * z64.abs().max(), tile      # (and it is the conv)
        zd = z.reshape(M, Cout).double().cpu()
        pc = part.double().cpu()
        assert pc.shape == ((M + bm - 1) // bm, 2, Cout), tile
        e1, b1 = (pc[:, 0] - _tile_sums(zd, bm)).abs(), bm * u * _tile_sums(zd.abs(), bm)
        e2, b2 = (pc[:, 1] - _tile_sums(zd * zd, bm)).abs(), (bm + 1) * u * _tile_sums(zd * zd, bm)
        print(f"  {geom} tile {tile}: sum z {float((e1 / b1.clamp_min(1e-300)).max()):.3f} of its bound, "
              f"sum z^2 {float((e2 / b2.clamp_min(1e-300)).max()):.3f}")
        assert (e1 <= b1).all() and (e2 <= b2).all(), tile


@pytest.mark.parametrize("geom", GEOMS)
def test_batchnorm_from_the_partials_and_determinism(hip_lib, dev, geom):
    """T.bn_fwd_partials on the new partials against T.bn_stats + T.bn_apply on z: mean / invstd / running statistics at the
    tolerances tests/test_train_ops_gpu.py::test_conv_with_batch_statistics_in_the_epilogue applies to the fp32 form of this
    comparison (rtol 1e-5; atol 1e-7 where the value may be near zero), the output at that file's bound for a BatchNorm output
    (rtol 1e-5, atol 2e-5) -- the file keeps them as literals, restated here.  Two calls are bit-identical."""
    from pemp_amd import ops, train_ops as T
    x, prm, z64 = _case(dev, geom, False)
    M, Cout = z64.shape
    g = torch.Generator().manual_seed(5)
    rm, rv = torch.rand(Cout, generator=g) * 2 - 1, torch.rand(Cout, generator=g) + 0.5
    gamma, beta = (torch.rand(Cout, generator=g) + 0.5).to(dev), (torch.rand(Cout, generator=g) * 2 - 1).to(dev)
    for tile in _ids(ops, Cout):
        z, part = ops.conv2d_stats(x, prm, tile=tile)
        z2, part2 = ops.conv2d_stats(x, prm, tile=tile)
        assert torch.equal(z, z2) and torch.equal(part, part2), tile
        rm1, rv1, rm2, rv2 = rm.to(dev), rv.to(dev), rm.to(dev), rv.to(dev)
        y1, mean1, invstd1 = T.bn_fwd_partials(z, part, gamma, beta, torch.empty_like(z), 1e-5, 0.1, rm1, rv1, relu=True)
        mean0, invstd0 = T.bn_stats(z.reshape(M, Cout), 1e-5, 0.1, rm2, rv2)
        y0 = T.bn_apply(z, mean0, invstd0, gamma, beta, torch.empty_like(z), relu=True)
        assert torch.allclose(mean1, mean0, rtol=1e-5, atol=1e-7) and torch.allclose(invstd1, invstd0, rtol=1e-5), tile
        assert torch.allclose(rm1, rm2, rtol=1e-5, atol=1e-7) and torch.allclose(rv1, rv2, rtol=1e-5, atol=1e-7), tile
        assert torch.allclose(y1, y0, rtol=1e-5, atol=2e-5), tile


def test_tile_zero_picks_among_the_offered_ids_under_a_key_of_its_own(hip_lib, dev, monkeypatch):
    """tile=0: the pick hook sees the offered ids that fit Cout, the pick is remembered under a key that neither the fp32
    statistics pick nor the plain split3 pick of the same layer uses, and the partials are sliced to the picked id's row tiles."""
    from pemp_amd import ops
    x, prm, z64 = _case(dev, GEOMS[0], False)
    M, Cout = z64.shape
    saved = dict(ops._TILE_CACHE)
    seen = []

    def hook(kind, cands, key):
        seen.append((kind, tuple(cands), key))
        return 46 if 46 in cands else cands[0]

    monkeypatch.setattr(ops, "PICK_HOOK", hook)
    try:
        ops._TILE_CACHE.clear()
        z, part = ops.conv2d_stats(x, prm)
        assert seen[-1][0] == "conv" and sorted(seen[-1][1]) == sorted(ops.split3_stats_tiles(Cout))
        assert part.shape[0] == (M + 255) // 256 and torch.equal(z, ops.conv2d(x, prm, tile=46))
        k_stats3 = seen[-1][2]
        ops.conv2d(x, prm)
        fp32 = ops.ConvParams(prm.w, None, None, prm.cin, prm.cout, prm.kh, prm.kw, prm.stride, prm.pad, prm.dil, prm.kpad, False, False)
        ops.conv2d_stats(x, fp32)
        keys = [s[2] for s in seen]
        assert len(keys) == 3 and len(set(keys)) == 3 and ops._TILE_CACHE[k_stats3] == 46
        assert set(seen[2][1]) <= set(range(21, 38))                    # the fp32 statistics pick is what it was
        n = len(seen)
        ops.conv2d_stats(x, prm)                                        # remembered: no second pick
        assert len(seen) == n
    finally:
        ops._TILE_CACHE.clear()
        ops._TILE_CACHE.update(saved)
