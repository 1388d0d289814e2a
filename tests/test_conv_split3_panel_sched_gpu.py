"""The long-K schedule of the activation-stationary split3 kernels (conv_panel.hip, ids 71 / 72 at K >= 128: a tile's residual quads
requested in its first K step, a weight ring of 5 to 8 stages, every counted wait derived from the issue order) against id 43, bit
for bit.  Shapes sit where that bookkeeping can go wrong:

 * K = 128, 160, 256 (4, 5, 8 K steps: the two-blocks-per-CU form, an odd step count, the register-tight form);
 * Cout = 64, 128, 256, 1024: BN, 2 BN and 1024 of either id (one tile: no previous tile's stores behind any wait; two: a single
   hand-over; 8 / 16 tiles: the ring wraps several times and ends in the phantom stages past the last real one);
 * M = 63 (one partial block: rows >= M go behind the descriptor's range) and 3 x 13 x 11 = 429 (four blocks, a tail in the last);
 * residual and ReLU on and off; scale and shift both, shift alone, neither;
 * the residual and the output as channel windows of wider buffers, a sentinel around the output window;
 * a launch replayed twice from a captured graph."""
import itertools

import pytest
import torch

from tests import test_conv_split3_panel_gpu as P

pytestmark = pytest.mark.gpu

SCHED = (71, 72)                         # every id that carries the schedule
MAPS = ((1, 7, 9), (3, 13, 11))          # (N, H, W): M = 63, 429
KS = (128, 160, 256)
COUTS = (64, 128, 256, 1024)             # id 72 (BN = 64): 1, 2, 4, 16 tiles; id 71 (BN = 128): none, 1, 2, 8


@pytest.fixture(scope="module")
def pool(dev):
    """One pool of random numbers every case slices: activations, weights, scale, shift, residual."""
    g = torch.Generator(device=dev).manual_seed(7172)
    return dict(x=torch.randn(429, 256, generator=g, device=dev), w=torch.randn(1024, 256, generator=g, device=dev) / 16.0,
                scale=torch.rand(1024, generator=g, device=dev) + 0.5, shift=torch.randn(1024, generator=g, device=dev),
                res=torch.randn(429, 1024, generator=g, device=dev))


def _problem(pool, nhw, cin, cout):
    N, H, W = nhw
    M = N * H * W
    x = pool["x"][:M, :cin].contiguous().view(N, H, W, cin)
    w = pool["w"][:cout, :cin].contiguous().view(cout, cin, 1, 1)
    res = pool["res"][:M, :cout].contiguous().view(N, H, W, cout)
    return x, w, res


def _params(ops, pool, w, affine, relu):
    """affine: "both" = scale and shift, "shift", "none"."""
    co, ci = w.shape[:2]
    packed, kpad = ops.pack_conv_weight(w)
    packed = packed.contiguous()
    scale = pool["scale"][:co].contiguous() if affine == "both" else None
    shift = pool["shift"][:co].contiguous() if affine != "none" else None
    return ops.ConvParams(packed, scale, shift, ci, co, 1, 1, 1, 0, 1, kpad, False, relu, ops.pack_split3(packed))


def test_the_existing_helper_checks_the_ids_of_the_schedule():
    assert tuple(P.PANEL) == SCHED


@pytest.mark.parametrize("cout", COUTS)
@pytest.mark.parametrize("cin", KS)
@pytest.mark.parametrize("nhw", MAPS, ids=lambda m: "x".join(map(str, m)))
def test_long_k_schedule_matches_id_43_bit_for_bit(hip_lib, dev, pool, nhw, cin, cout):
    from pemp_amd import ops
    x, w, res = _problem(pool, nhw, cin, cout)
    for residual, relu in itertools.product((False, True), repeat=2):
        P._check(ops, x, _params(ops, pool, w, "shift", relu), res if residual else None)


@pytest.mark.parametrize("affine", ("both", "none"))
@pytest.mark.parametrize("cin", KS)
def test_scale_and_shift_present_and_absent(hip_lib, dev, pool, cin, affine):
    from pemp_amd import ops
    for cout in (128, 256):
        x, w, res = _problem(pool, MAPS[1], cin, cout)
        for residual in (False, True):
            P._check(ops, x, _params(ops, pool, w, affine, True), res if residual else None)


@pytest.mark.parametrize("cin", KS)
def test_residual_and_output_as_channel_windows(hip_lib, dev, pool, cin):
    """ldr, ldy > Cout: the residual and the output are channel slices of wider buffers; nothing but the output window is written."""
    from pemp_amd import ops
    N, H, W = MAPS[1]
    for tile in SCHED:
        cout = 2 * ops._tile_bn(tile)
        x, w, res = _problem(pool, MAPS[1], cin, cout)
        p = _params(ops, pool, w, "shift", True)
        want = ops.conv2d(x, p, residual=res, tile=43)
        rb = torch.full((N, H, W, cout + 96), -2.0, device=dev)
        rb[..., 64:64 + cout] = res
        big = torch.full((N, H, W, cout + 160), 7.0, device=dev)
        ops.conv2d(x, p, residual=rb[..., 64:64 + cout], out=big[..., 32:32 + cout], tile=tile)
        assert torch.equal(big[..., 32:32 + cout], want), tile
        assert bool((big[..., :32] == 7.0).all()) and bool((big[..., 32 + cout:] == 7.0).all()), tile


def test_graph_replays_equal_each_other_and_the_eager_result(hip_lib, dev, pool):
    from pemp_amd import ops
    x, w, res = _problem(pool, MAPS[1], 256, 1024)
    p = _params(ops, pool, w, "shift", True)
    want = ops.conv2d(x, p, residual=res, tile=43)
    for tile in SCHED:
        out = torch.empty_like(want)
        ops.conv2d(x, p, residual=res, out=out, tile=tile)           # warm: the launch's one-time attribute call is not captured
        torch.cuda.synchronize()
        eager = out.clone()
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                ops.conv2d(x, p, residual=res, out=out, tile=tile)
        torch.cuda.current_stream().wait_stream(s)
        replays = []
        for _ in range(2):
            out.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            replays.append(out.clone())
        assert torch.equal(replays[0], replays[1]), tile
        assert torch.equal(replays[0], eager) and torch.equal(eager, want), tile
