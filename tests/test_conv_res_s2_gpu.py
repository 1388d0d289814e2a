"""The strided residual of the split3 convs (PEMP_CONV_RES_S2, ops.conv2d residual_stride=2; conv_panel_rs2_kernel on ids 71 / 72,
conv_dma2_rs2_kernel on id 43): output row (n, ho, wo) adds pixel (n, 2 ho, 2 wo) of a residual on a grid twice as fine.

 * every id that takes the flag against the SAME id on the gathered dense residual, bit for bit: residual grids 13 x 13 -> 7 x 7
   (odd / odd; 147 rows: two panel blocks, the second partial; three row tiles of id 43), 12 x 14 -> 6 x 7 (even / even) and
   5 x 6 -> 3 x 3; Cin 64 and 128, Cout 256, ReLU on; the residual as a channel window of a wider buffer (ldr > Cout);
 * one case against float64 on the CPU (torch.nn.functional.conv2d + the gathered residual) at the family's bound
   (tests/test_conv_split3_fuzz_cpu.py: ratio_bound), so that two wrong paths cannot agree;
 * the refusals: the persistent ids, the other split3 ids, the fp32 chain, split-K, a pre-split output, mismatched sizes."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests.test_conv_split3_fuzz_cpu import errors, ratio_bound

pytestmark = pytest.mark.gpu

# (N, Hr, Wr) of the residual's grid -> the output's (Ho, Wo)
GRIDS = {(3, 13, 13): (7, 7), (2, 12, 14): (6, 7), (1, 5, 6): (3, 3)}
CINS = (64, 128)
COUT = 256


def _params(ops, w, shift, relu=True):
    packed, kpad = ops.pack_conv_weight(w)
    packed = packed.contiguous()
    co, ci, kh, kw = w.shape
    return ops.ConvParams(packed, None, shift, ci, co, kh, kw, 1, 0, 1, kpad, False, relu, ops.pack_split3(packed))


@pytest.fixture(scope="module")
def data(dev):
    """One pool of random numbers every case slices: the compact activations, weights, shift and the full-grid residual."""
    g = torch.Generator(device=dev).manual_seed(128)
    return dict(x=torch.randn(147, 128, generator=g, device=dev), w=torch.randn(COUT, 128, generator=g, device=dev) / 8.0,
                shift=torch.randn(COUT, generator=g, device=dev), res=torch.randn(3 * 13 * 13, COUT, generator=g, device=dev))


def _problem(data, grid, cin):
    n, hr, wr = grid
    ho, wo = GRIDS[grid]
    x = data["x"][:n * ho * wo, :cin].contiguous().view(n, ho, wo, cin)
    w = data["w"][:, :cin].contiguous().view(COUT, cin, 1, 1)
    res = data["res"][:n * hr * wr].contiguous().view(n, hr, wr, COUT)
    return x, w, data["shift"], res


def test_the_ids_that_take_the_flag(hip_lib):
    from pemp_amd import ops
    p64 = ops.ConvParams(None, None, None, 64, 256, 1, 1, 1, 0, 1, 64, False, True, w3=object())
    p128 = ops.ConvParams(None, None, None, 128, 256, 1, 1, 1, 0, 1, 128, False, True, w3=object())
    p3x3 = ops.ConvParams(None, None, None, 64, 256, 3, 3, 1, 1, 1, 576, False, True, w3=object())
    assert set(ops.res_s2_tiles(p64)) == {43, 71, 72} and set(ops.res_s2_tiles(p128)) == {43, 72} and ops.res_s2_tiles(p3x3) == (43,)
    assert not set(ops.SPLIT3_RES_S2_TILES) & set(ops.SPLIT3_PERSISTENT)


@pytest.mark.parametrize("cin", CINS)
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_strided_residual_equals_the_gathered_one_bit_for_bit(hip_lib, dev, data, grid, cin):
    from pemp_amd import ops
    x, w, shift, res = _problem(data, grid, cin)
    p = _params(ops, w, shift)
    dense = res[:, ::2, ::2, :].contiguous()
    assert tuple(dense.shape[1:3]) == GRIDS[grid]
    tiles = ops.res_s2_tiles(p)
    assert set(tiles) == ({43, 71, 72} if cin == 64 else {43, 72})
    ref43 = ops.conv2d(x, p, residual=dense, tile=43)
    for tile in tiles:
        want = ops.conv2d(x, p, residual=dense, tile=tile)
        assert bool(want.abs().sum() > 0) and torch.equal(want, ref43)
        got = torch.full_like(want, float("nan"))
        ops.conv2d(x, p, residual=res, residual_stride=2, out=got, tile=tile)
        bad = got != want
        assert not bool(bad.any()), (tile, int(bad.sum()), bad.nonzero()[:4].tolist())


@pytest.mark.parametrize("cin", CINS)
def test_the_residual_as_a_channel_window_of_a_wider_buffer(hip_lib, dev, data, cin):
    from pemp_amd import ops
    grid = (3, 13, 13)
    x, w, shift, res = _problem(data, grid, cin)
    p = _params(ops, w, shift)
    want = ops.conv2d(x, p, residual=res[:, ::2, ::2, :].contiguous(), tile=43)
    rb = torch.full((3, 13, 13, COUT + 96), -2.0, device=dev)
    rb[..., 64:64 + COUT] = res
    for tile in ops.res_s2_tiles(p):
        got = torch.full_like(want, float("nan"))
        ops.conv2d(x, p, residual=rb[..., 64:64 + COUT], residual_stride=2, out=got, tile=tile)
        assert torch.equal(got, want), tile


def test_the_untuned_call_and_the_pick_key(hip_lib, dev, data, monkeypatch):
    """A call that names no id runs one that takes the flag, and a pick made on the dense residual is never replayed on the strided
    one, nor the reverse: the two calls remember their picks under different keys, and only the ids of res_s2_tiles are offered."""
    from pemp_amd import ops
    x, w, shift, res = _problem(data, (3, 13, 13), 64)
    p = _params(ops, w, shift)
    dense = res[:, ::2, ::2, :].contiguous()
    want = ops.conv2d(x, p, residual=dense, tile=43)
    saved = dict(ops._TILE_CACHE)
    offered = []

    def last_candidate(launch, key, cands):
        offered.append((key, list(cands)))
        ops._TILE_CACHE[key] = cands[-1]
        return cands[-1]

    monkeypatch.setattr(ops, "_pick_tile", last_candidate)
    monkeypatch.setattr(ops, "_tunes", lambda rows, least=1024: True)
    monkeypatch.setattr(ops, "SPLIT3_PANEL", True)
    monkeypatch.setattr(ops, "EVAL_SPLITK", False)
    try:
        ops._TILE_CACHE.clear()
        assert torch.equal(ops.conv2d(x, p, residual=dense), want)
        monkeypatch.setattr(ops, "EVAL_SPLITK", True)        # split-K is never offered to the strided call
        assert torch.equal(ops.conv2d(x, p, residual=res, residual_stride=2), want)
        assert torch.equal(ops.conv2d(x, p, residual=res, residual_stride=2), want)
        assert len(offered) == 2 and offered[0][0] != offered[1][0]
        assert 47 in offered[0][1] and set(offered[1][1]) == set(ops.res_s2_tiles(p))
    finally:
        ops._TILE_CACHE.clear()
        ops._TILE_CACHE.update(saved)


def test_one_case_against_float64_on_the_cpu(hip_lib, dev, data):
    """Every id's error against the float64 conv + shift + gathered residual + ReLU, as a multiple of the error of torch's CPU fp32
    conv2d with the same epilogue: at most the family's bound for this K."""
    from pemp_amd import ops
    cin = 128
    x, w, shift, res = (t.cpu() for t in _problem(data, (3, 13, 13), cin))
    gathered = res[:, ::2, ::2, :]
    nchw = lambda t: t.permute(0, 3, 1, 2)
    ref = torch.relu(F.conv2d(nchw(x).double(), w.double()).permute(0, 2, 3, 1) + shift.double() + gathered.double())
    yard = torch.relu(F.conv2d(nchw(x), w).permute(0, 2, 3, 1) + shift + gathered)
    mag = F.conv2d(nchw(x).abs().double(), w.abs().double()).permute(0, 2, 3, 1) + shift.abs().double() + gathered.abs().double()
    ymax, yrms = errors(yard, ref, mag)
    bound = ratio_bound(cin)
    p = _params(ops, w.to(dev), shift.to(dev))
    for tile in ops.res_s2_tiles(p):
        y = torch.full(tuple(ref.shape), float("nan"), device=dev)
        ops.conv2d(x.to(dev), p, residual=res.to(dev), residual_stride=2, out=y, tile=tile)
        emax, erms = errors(y.cpu(), ref, mag)
        print(f"strided residual vs float64 | id {tile} | max x{emax / ymax:.2f} | rms x{erms / yrms:.2f} | bound {bound}")
        assert emax <= bound * ymax and erms <= bound * yrms, (tile, emax / ymax, erms / yrms, bound)


def test_ops_refuses_what_does_not_take_the_flag(hip_lib, dev, data):
    from pemp_amd import ops
    x, w, shift, res = _problem(data, (3, 13, 13), 64)
    p = _params(ops, w, shift)
    p128 = _params(ops, _problem(data, (3, 13, 13), 128)[1], shift)
    x128 = _problem(data, (3, 13, 13), 128)[0]
    plain = ops.ConvParams(p.w, None, shift, 64, COUT, 1, 1, 1, 0, 1, 64, False, True)           # no split weights: the fp32 chain
    bad = [
        dict(tile=47), dict(tile=49), dict(tile=41), dict(tile=42), dict(tile=44), dict(tile=46), dict(tile=23), dict(tile=51),
        dict(splitk=True), dict(out_split3=True), dict(residual=None), dict(residual_stride=3),
        dict(pad_value=torch.zeros(64, device=dev)),
        dict(residual=res[:, :12].contiguous()),             # 12 rows -> 6, the output has 7
        dict(residual=res[:, :, :11].contiguous()),
        dict(residual=res[:2]),
        dict(residual=res[..., :128]),
        dict(p=plain),
        dict(p=p128, x=x128, tile=71),                       # 71 at K = 128: not instantiated (it would spill)
    ]
    for kw in bad:
        kw = dict(dict(x=x, p=p, residual=res, residual_stride=2), **kw)
        with pytest.raises(ValueError):
            ops.conv2d(kw.pop("x"), kw.pop("p"), **kw)
    with pytest.raises(ValueError):
        ops.conv2d(x, p, residual=res[:, ::2, ::2, :].contiguous(), residual_stride=2)     # a dense residual under the flag: 7 -> 4


def test_the_library_refuses_what_does_not_take_the_flag(hip_lib, dev, data):
    """The entry itself, below ops: nothing is launched, pemp_last_error names the flag."""
    from pemp_amd import _lib, ops
    x, w, shift, res = _problem(data, (3, 13, 13), 64)
    p = _params(ops, w, shift)
    y = torch.empty(3, 7, 7, COUT, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    S2 = _lib.CONV_RES_S2

    def call(tile, flags, kpad=64, residual=res, weights=None, fn="pemp_conv2d_nhwc_f32", extra=()):
        d = _lib.ConvDesc(3, 7, 7, kpad, kpad, 7, 7, COUT, COUT, 1, 1, 1, 0, 1, COUT, kpad, flags, tile)
        wp = ptr(p.w3 if weights is None else weights)
        return getattr(hip_lib, fn)(C.byref(d), ptr(x), wp, ptr(y), None, ptr(shift), None if residual is None else ptr(residual),
                                    *extra, ops._stream())

    ws = torch.empty(1 << 20, device=dev)
    cases = [("47", call(47, S2)), ("49", call(49, S2)), ("41", call(41, S2)), ("46", call(46, S2)), ("fp32 chain", call(23, S2, weights=p.w)),
             ("tile 0", call(0, S2, weights=p.w)), ("71 at K = 128", call(71, S2, kpad=128)), ("no residual", call(43, S2, residual=None)),
             ("out_split3", call(43, S2 | _lib.CONV_OUT_SPLIT3)), ("parity bit alone", call(43, _lib.CONV_RES_HEVEN)),
             ("split-K", call(51, S2, fn="pemp_conv2d_splitk_nhwc_f32", extra=(ptr(ws), C.c_size_t(ws.numel() * 4)))),
             ("workspace", call(43, S2, fn="pemp_conv2d_splitk_nhwc_f32", extra=(ptr(ws), C.c_size_t(ws.numel() * 4))))]
    for what, rc in cases:
        assert rc != 0, what
    assert b"RES_S2" in hip_lib.pemp_last_error()
    assert call(43, S2 | _lib.CONV_RELU) == 0, hip_lib.pemp_last_error()
    torch.cuda.synchronize()
    assert torch.equal(y, ops.conv2d(x, p, residual=res[:, ::2, ::2, :].contiguous(), tile=43))
