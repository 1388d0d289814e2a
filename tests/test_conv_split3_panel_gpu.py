"""The activation-stationary split3 kernels (conv_panel.hip, tile ids 71 / 72: a block keeps 128 rows x K of split activations in
registers and walks all of Cout) against id 43, bit for bit, and against float64.

 * K = 32, 96, 256 (1, 3, 8 K steps: every form of the counted wait); M = 63, 338 and 384 (a tail inside a wave's 32 rows, inside a
   block's 128, none); Cout = 64, 128, 1024 (one, two and many N tiles); residual / ReLU on and off, no scale; stride 2 (a row
   gather); input and output as channel windows of wider buffers; a launch replayed from a captured graph, twice.
 * the six piece probes of tests/test_conv_split3_fuzz_cpu.py in their 1x1 geometry are exact; one fuzz case is held to float64
   with that file's bound for K <= 576."""
import itertools

import pytest
import torch

from tests import test_conv_split3_fuzz_cpu as A

pytestmark = pytest.mark.gpu

PANEL = (71, 72)
# (N, H, W): M = 63, 338, 384
MAPS = ((1, 7, 9), (2, 13, 13), (2, 12, 16))
KS = (32, 96, 256)
COUTS = (64, 128, 1024)


def _params(ops, w, shift, stride, relu):
    packed, kpad = ops.pack_conv_weight(w)
    packed = packed.contiguous()
    co, ci, kh, kw = w.shape
    return ops.ConvParams(packed, None, shift, ci, co, kh, kw, stride, 0, 1, kpad, False, relu, ops.pack_split3(packed))


@pytest.fixture(scope="module")
def data(dev):
    """One pool of random numbers every case slices: activations, weights, shift, residual."""
    g = torch.Generator(device=dev).manual_seed(71)
    return dict(x=torch.randn(384, 256, generator=g, device=dev), w=torch.randn(1024, 256, generator=g, device=dev) / 16.0,
                shift=torch.randn(1024, generator=g, device=dev), res=torch.randn(384, 1024, generator=g, device=dev))


def _problem(data, nhw, cin, cout, stride=1):
    N, H, W = nhw
    M = N * H * W
    x = data["x"][:M, :cin].contiguous().view(N, H, W, cin)
    w = data["w"][:cout, :cin].contiguous().view(cout, cin, 1, 1)
    ho, wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    res = data["res"][:N * ho * wo, :cout].contiguous().view(N, ho, wo, cout)
    return x, w, data["shift"][:cout].contiguous(), res


def _check(ops, x, p, res, want=None):
    want = ops.conv2d(x, p, residual=res, tile=43) if want is None else want
    assert bool(want.abs().sum() > 0)
    for tile in PANEL:
        if p.cout % ops._tile_bn(tile):
            continue
        got = torch.full_like(want, float("nan"))
        ops.conv2d(x, p, residual=res, out=got, tile=tile)
        bad = got != want
        assert not bool(bad.any()), (tile, int(bad.sum()), bad.nonzero()[:4].tolist())
    return want


@pytest.mark.parametrize("cout", COUTS)
@pytest.mark.parametrize("cin", KS)
@pytest.mark.parametrize("nhw", MAPS, ids=lambda m: "x".join(map(str, m)))
def test_panel_ids_match_id_43_bit_for_bit(hip_lib, dev, data, nhw, cin, cout):
    from pemp_amd import ops
    x, w, shift, res = _problem(data, nhw, cin, cout)
    for residual, relu in itertools.product((False, True), repeat=2):
        _check(ops, x, _params(ops, w, shift, 1, relu), res if residual else None)


@pytest.mark.parametrize("cin,cout", [(32, 64), (256, 1024)])
def test_stride_2_is_a_row_gather(hip_lib, dev, data, cin, cout):
    from pemp_amd import ops
    x, w, shift, res = _problem(data, (2, 13, 13), cin, cout, stride=2)
    p = _params(ops, w, shift, 2, True)
    assert tuple(res.shape[1:3]) == (7, 7)
    _check(ops, x, p, res)
    _check(ops, x, p, None)


def test_channel_windows_of_wider_buffers(hip_lib, dev, data):
    """x, the residual and the output are channel slices (per-pixel strides above their channel counts); nothing but the output
    window is written."""
    from pemp_amd import ops
    x, w, shift, res = _problem(data, (2, 13, 13), 96, 128)
    p = _params(ops, w, shift, 1, True)
    want = ops.conv2d(x, p, residual=res, tile=43)
    xb = torch.full((2, 13, 13, 160), 3.0, device=dev)
    xb[..., 32:128] = x
    rb = torch.full((2, 13, 13, 192), -2.0, device=dev)
    rb[..., 64:] = res
    for tile in PANEL:
        big = torch.full((2, 13, 13, 320), 7.0, device=dev)
        ops.conv2d(xb[..., 32:128], p, residual=rb[..., 64:], out=big[..., 64:192], tile=tile)
        assert torch.equal(big[..., 64:192], want), tile
        assert bool((big[..., :64] == 7.0).all()) and bool((big[..., 192:] == 7.0).all()), tile


def test_graph_replay_and_run_to_run_identity(hip_lib, dev, data):
    from pemp_amd import ops
    x, w, shift, res = _problem(data, (2, 13, 13), 256, 1024)
    p = _params(ops, w, shift, 1, True)
    want = ops.conv2d(x, p, residual=res, tile=43)
    for tile in PANEL:
        out = torch.empty_like(want)
        ops.conv2d(x, p, residual=res, out=out, tile=tile)           # warm: the launch's one-time attribute call is not captured
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                ops.conv2d(x, p, residual=res, out=out, tile=tile)
        torch.cuda.current_stream().wait_stream(s)
        for _ in range(2):
            out.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want), tile
        a = ops.conv2d(x, p, residual=res, tile=tile)
        b = ops.conv2d(x, p, residual=res, tile=tile)
        assert torch.equal(a, b) and torch.equal(a, want), tile


def test_a_remembered_panel_pick_is_not_replayed_by_a_call_the_ids_do_not_take(hip_lib, dev, data, monkeypatch):
    """The same layer and input shape with and without a per-image shift (a bottleneck's conv1 in the stage-2 engine): the pick
    made where 71 / 72 are candidates is remembered apart from the pick of the call they do not take."""
    from pemp_amd import ops
    x, w, shift, _ = _problem(data, (2, 13, 13), 256, 64)
    p = _params(ops, w, shift, 1, True)
    per_img = data["res"][:2, :64].contiguous()
    saved = dict(ops._TILE_CACHE)
    offered = []

    def last_candidate(launch, key, cands):
        offered.append(list(cands))
        ops._TILE_CACHE[key] = cands[-1]
        return cands[-1]

    monkeypatch.setattr(ops, "_pick_tile", last_candidate)
    monkeypatch.setattr(ops, "_tunes", lambda rows, least=1024: True)
    monkeypatch.setattr(ops, "AUTOTUNE", True)
    monkeypatch.setattr(ops, "SPLIT3_PANEL", True)
    try:
        ops._TILE_CACHE.clear()
        plain = ops.conv2d(x, p)
        assert offered[-1][-1] == 72 and 72 in ops._TILE_CACHE.values()
        assert torch.equal(plain, ops.conv2d(x, p, tile=43))
        for _ in range(2):                                   # picks, then replays its own pick
            got = ops.conv2d(x, p, shift_override=per_img, per_image_shift=True)
            assert torch.equal(got, ops.conv2d(x, p, shift_override=per_img, per_image_shift=True, tile=43))
        assert len(offered) == 2 and not set(offered[-1]) & set(PANEL)
        assert torch.equal(ops.conv2d(x, p), plain) and len(offered) == 2
    finally:
        ops._TILE_CACHE.clear()
        ops._TILE_CACHE.update(saved)


# ---- float64 --------------------------------------------------------------------------------------------------------------------
PROBES_1X1 = [pr for pr in A.PROBES if pr[1][4] == 1 and pr[1][6] == 0]
FUZZ_CASE = next(c for c in A.fuzz_cases() if c[5] == 1 and c[7] == 0 and c[9] == "affine" and c[3] <= 256)


def test_the_probe_and_fuzz_selection_is_what_it_should_be():
    assert len(PROBES_1X1) == 6 and {pr[0] for pr in PROBES_1X1} == set(A.PRODUCTS)
    assert FUZZ_CASE[3] * FUZZ_CASE[5] ** 2 <= A.SMALL_K


def _dev_params(ops, dev, w, stride, dil, scale=None, shift=None, relu=False):
    packed, kpad = ops.pack_conv_weight(w.to(dev))
    packed = packed.contiguous()
    co, ci, kh, kw = w.shape
    dv = lambda t: None if t is None else t.to(dev)
    return ops.ConvParams(packed, dv(scale), dv(shift), ci, co, kh, kw, stride, 0, dil, kpad, False, relu, ops.pack_split3(packed))


@pytest.mark.parametrize("probe", PROBES_1X1, ids=A.probe_id)
def test_panel_ids_are_exact_on_the_piece_probes(hip_lib, dev, probe):
    from pemp_amd import ops
    q = A.probe_problem(probe)
    ref = A.conv_f64(q["x"], q["w"], q["stride"], q["pad"], q["dil"], q["pv"])
    want = ref.float().to(dev)
    assert torch.equal(want.double().cpu(), ref)
    x = q["x"].to(dev)
    prm = _dev_params(ops, dev, q["w"], q["stride"], q["dil"])
    for tile in PANEL:
        for _ in range(2):
            y = torch.full_like(want, float("nan"))
            ops.conv2d(x, prm, out=y, tile=tile)
            bad = y != want
            assert not bool(bad.any()), (A.probe_id(probe), tile, int(bad.sum()), bad.nonzero()[:4].tolist())


def test_a_fuzz_case_against_float64(hip_lib, dev):
    """The error of each id against the float64 convolution with the epilogue, as a multiple of the yardstick's (torch's CPU fp32
    conv2d): at most tests/test_conv_split3_fuzz_cpu.py's bound for K <= 576."""
    from pemp_amd import ops
    case = FUZZ_CASE
    N, H, W, cin, cout, k, s, p, d, epi = case
    ref, mag, (ymax, yrms) = A.fuzz_reference(case)
    o = A.fuzz_operands(case)
    prm = _dev_params(ops, dev, o["w"], s, d, o["scale"], o["shift"], relu=True)
    x, res = o["x"].to(dev), o["res"].to(dev)
    bound = A.ratio_bound(cin * k * k)
    for tile in PANEL:
        if cout % ops._tile_bn(tile):
            continue
        y = torch.full(tuple(ref.shape), float("nan"), device=dev)
        ops.conv2d(x, prm, residual=res, out=y, tile=tile)
        emax, erms = A.errors(y.cpu(), ref, mag)
        print(f"split3 panel fuzz {A.case_id(case)} | id {tile} | max x{emax / ymax:.2f} | rms x{erms / yrms:.2f} | bound {bound}")
        assert emax <= bound * ymax and erms <= bound * yrms, (tile, emax / ymax, erms / yrms, bound)
