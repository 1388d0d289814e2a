"""The split3 conv family (tile ids 41..44, 46 and the split-K forms 51, 52, 54, 56; include/pemp_hip.h): fp32 operands as three bf16
pieces on v_mfma_f32_32x32x16_bf16.  Held here: the weight pack is exact and laid out as stated; every variant is exact on integer
probes (zero padding, padding values, whole and split tiles); on random data its error against float64 stays within 1.5 x the
fp32-chain kernel's; the unsplit variants and the grouped launch are bit-identical among themselves; the stage-1 model on the
family (the default) moves its logits by no more than the end-to-end tolerance against the fp32 chain.

What the integer probes here do not reach: their weights are 1..3 and their activations integers below 1021, so the weight planes m
and l and the activation plane l are all zero, and of the six kept products (lh, hl, mm, mh, hm, hh; activation piece first) only
hh and mh are ever non-zero.  A kernel that read a wrong weight plane or lost one of hl, lh, hm, mm would pass them.  The probes of
tests/test_conv_split3_fuzz_gpu.py exercise each product on its own, and that file measures the random-data error against float64
with torch's CPU fp32 conv2d as the yardstick, at strides, kernel sizes and paddings this file does not use."""
import pytest
import torch
import torch.nn.functional as F

from tests import util
from tests.test_conv_probe_gpu import GEOMS, _problem, _reference
from tests.test_conv_split3_cpu import _cases, split3_reference
from tests.test_conv_split3_fuzz_cpu import conv_f64, errors, ratio_bound

pytestmark = pytest.mark.gpu

S3_UNSPLIT = (41, 42, 43, 44, 46)
S3_ALL = S3_UNSPLIT + (51, 52, 54, 56)


def _params(ops, w_oihw, shift=None, relu=False, pad=1, dil=1):
    packed, kpad = ops.pack_conv_weight(w_oihw)
    co, ci, kh, kw = w_oihw.shape
    return ops.ConvParams(packed.contiguous(), None, shift, ci, co, kh, kw, 1, pad, dil, kpad, False, relu, ops.pack_split3(packed.contiguous()))


def test_pack_is_exact_and_matches_the_layout(hip_lib, dev):
    from pemp_amd import ops
    for w in _cases():
        got = ops.pack_split3(w.to(dev).contiguous()).cpu()
        assert torch.equal(got.view(torch.int16), split3_reference(w).view(torch.int16))
        assert torch.equal(got.double().sum(dim=2).reshape(w.shape), w.double())


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(str(v) for v in g))
@pytest.mark.parametrize("padv", [False, True], ids=["zero-padding", "padding-value"])
def test_every_split3_variant_is_exact_on_integer_probes(hip_lib, dev, geom, padv):
    from pemp_amd import ops
    N, H, W, Cin, d = geom
    x, w, pv = _problem(N, H, W, Cin, d)
    ref = _reference(x, w, pv if padv else None, d)
    M = N * H * W
    buf = torch.empty(M + 4, Cin, device=dev)
    buf[:M] = x.view(M, Cin).float().to(dev)
    buf[M:] = pv.float().to(dev)
    xd, pvd = buf[:M].view(N, H, W, Cin), buf[M]
    prm = _params(ops, w.float().to(dev), pad=d, dil=d)
    want = ref.float().to(dev)
    for tile in S3_ALL:
        y = ops.conv2d(xd, prm, pad_value=pvd if padv else None, tile=tile)
        bad = y != want
        assert not bool(bad.any()), (geom, padv, tile, int(bad.sum()), (y - want)[bad][:4].tolist())


@pytest.mark.parametrize("N,HW,Cin,Cout,k,dil", [(2, 21, 64, 64, 1, 1), (2, 33, 128, 256, 3, 2), (3, 29, 256, 128, 1, 1),
                                                 (2, 51, 256, 256, 3, 1), (1, 40, 512, 256, 3, 6)])
def test_split3_error_is_within_the_fp32_chain_error(hip_lib, dev, N, HW, Cin, Cout, k, dil):
    from pemp_amd import ops
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, HW, HW, Cin, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) * (1.0 / (Cin * k * k) ** 0.5)
    pad = dil if k == 3 else 0
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), None, 1, pad, dil).permute(0, 2, 3, 1)
    prm = _params(ops, w.to(dev), pad=pad, dil=dil)
    xd = x.to(dev)
    e_chain = (ops.conv2d(xd, prm, tile=23).double().cpu() - ref).abs()
    y3 = ops.conv2d(xd, prm, tile=43).double().cpu()
    e3 = (y3 - ref).abs()
    assert e3.max().item() <= 1.5 * e_chain.max().item(), (e3.max().item(), e_chain.max().item())
    rms = lambda e: e.pow(2).mean().sqrt().item()
    assert rms(e3) <= 1.5 * rms(e_chain), (rms(e3), rms(e_chain))
    # and against a yardstick that is no kernel of this library: torch's CPU fp32 conv2d, errors relative to conv(|x|, |w|)
    mag = conv_f64(x.abs(), w.abs(), 1, pad, dil)
    y_cpu = F.conv2d(x.permute(0, 3, 1, 2), w, None, 1, pad, dil).permute(0, 2, 3, 1)
    (m3, r3), (mc, rc) = errors(y3, ref, mag), errors(y_cpu, ref, mag)
    print(f"split3 id 43 vs CPU fp32 {N}x{HW}x{HW}x{Cin}x{Cout}x{k}x{dil} | K {Cin * k * k} | max {m3:.2e} = x{m3 / mc:.2f} | "
          f"rms {r3:.2e} = x{r3 / rc:.2f} | yardstick max {mc:.2e} rms {rc:.2e}")
    bound = ratio_bound(Cin * k * k)
    assert m3 <= bound * mc and r3 <= bound * rc, (bound, m3, mc, r3, rc)


def test_split3_variants_and_the_grouped_launch_are_bit_identical(hip_lib, dev):
    from pemp_amd import ops
    g = torch.Generator().manual_seed(5)
    N, HW, Cin, Cout = 2, 51, 256, 256
    M = N * HW * HW
    buf = torch.empty(M + 4, Cin, device=dev)
    buf[:M] = torch.randn(M, Cin, generator=g).to(dev)
    buf[M:] = torch.randn(Cin, generator=g).to(dev)
    x, pv = buf[:M].view(N, HW, HW, Cin), buf[M]
    ps = [_params(ops, (torch.randn(Cout, Cin, 3, 3, generator=g) / 48).to(dev), shift=torch.randn(Cout, generator=g).to(dev),
                  relu=True, pad=dd, dil=dd) for dd in (1, 2, 6)]
    res = torch.randn(N, HW, HW, Cout, generator=g).to(dev)
    for pad_value in (None, pv):
        first = [ops.conv2d(x, p, pad_value=pad_value, residual=res, tile=43) for p in ps]
        for tile in S3_UNSPLIT:
            for p, f in zip(ps, first):
                assert torch.equal(ops.conv2d(x, p, pad_value=pad_value, residual=res, tile=tile), f), (tile, pad_value is None)
            outs = [torch.empty_like(f) for f in first]
            ops.conv2d_group([x] * 3, ps, outs, pad_values=None if pad_value is None else [pad_value] * 3, residuals=[res] * 3,
                             tile=tile)
            for o, f in zip(outs, first):
                assert torch.equal(o, f), ("group", tile, pad_value is None)
        # a batch of one image equals its slice of the batch of two
        one = ops.conv2d(x[1:].contiguous(), ps[1], residual=res[1:].contiguous(), tile=43)
        if pad_value is None:
            assert torch.equal(one, first[1][1:])


def test_default_engine_runs_split3_within_the_end_to_end_tolerance(hip_lib, dev):
    from pemp_amd import synth
    from pemp_amd.networks import pemp_stage1 as m
    net = m.ModelClass(None)
    net.load_state_dict(util.wgen_state_dict("stage1_rn50"))
    net = net.to(dev).eval()
    b = synth.make_batch([5678, 5679, 5680], shot=1, out_hw=(366, 500))
    t = lambda k_: torch.from_numpy(b[k_]).to(dev)
    sup, msk, qry = t("sup_img"), t("sup_mask"), t("qry_img")
    with torch.no_grad():
        p3 = net.lowres(sup, msk, qry)[0].clone()
        with net.precision("f32_chain"):
            pc = net.lowres(sup, msk, qry)[0].clone()
        eng = net.__dict__["_engines"]
        assert eng[0]["trunk"].stem.w3 is None                             # the NHWC4 stem stays on the fp32 chain
        assert all(v["trunk"].stem.w3 is None for v in eng.values())
    d = (p3 - pc).abs().max().item()
    print(f"split3 vs fp32 chain: max |d logit| {d:.2e}")
    assert 0 < d <= util.LOGIT_TOL
    util.assert_argmax_exact(p3, pc.argmax(1).cpu(), what="split3 vs fp32 chain")
