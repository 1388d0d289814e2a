"""The split3 conv family (conv_dma2.hip; tile ids 41, 42, 43, 44, 46, persistent 47, 49, split-K 51, 52, 54, 56) held to float64
and to a yardstick that is not a kernel of this library, at the geometries the engines use and at awkward ones: stride 2, 5x5,
padding that is not the dilation's, ragged and tiny M, Cin 96 / 160, Cout 64 / 320, every epilogue.

 * piece probes: six exact problems, one per kept bf16 product (lh, hl, mm, mh, hm, hh); every id gives the float64 result bit for
   bit, twice.  A kernel that reads a wrong weight plane, mis-indexes the 192-byte weight row or loses a product fails here.
 * fuzz accuracy: every id against the float64 convolution; its error may be ratio_bound(K) x that of torch's CPU fp32 conv2d.
 * every unsplit id, 47 and 49 included, and the grouped launch equal id 43 bit for bit; channel windows of wider buffers.
 * power-of-two scaling of either operand scales the result and changes no bit.
 * the in-register activation split loses nothing on the hard values of the weight split's tests.

tests/test_conv_split3_fuzz_cpu.py proves on the CPU that the probes are exact and that the bound sees a dropped product."""
import pytest
import torch

from tests import test_conv_split3_fuzz_cpu as A
from tests.test_conv_split3_cpu import _cases as _split_cases

pytestmark = pytest.mark.gpu

CASES = A.fuzz_cases()
GROUPABLE = (41, 42, 43, 44, 46)            # the grouped launch has no persistent form


def _ids(ops, cout):
    return [t for t in A.S3_IDS if cout % ops._tile_bn(t) == 0]


def _layout(dev, x, pv):
    """The activations on the device with the padding vector directly behind them (PurifierEngine's layout)."""
    buf, _, _ = A.cpu_layout(x, pv)
    buf = buf.to(dev)
    N, H, W, C = x.shape
    M = N * H * W
    return buf[:M].view(N, H, W, C), (None if pv is None else buf[M])


def _params(ops, dev, w, stride, pad, dil, scale=None, shift=None, relu=False):
    packed, kpad = ops.pack_conv_weight(w.to(dev))
    packed = packed.contiguous()
    co, ci, kh, kw = w.shape
    dv = lambda t: None if t is None else t.to(dev)
    return ops.ConvParams(packed, dv(scale), dv(shift), ci, co, kh, kw, stride, pad, dil, kpad, False, relu, ops.pack_split3(packed))


def _case_on_device(ops, dev, case, epilogue=True):
    """-> (x view, padding vector or None, ConvParams, conv2d keywords of the case's epilogue)."""
    N, H, W, cin, cout, k, s, p, d, epi = case
    o = A.fuzz_operands(case)
    x, pv = _layout(dev, o["x"], o["pv"])
    kw = {}
    if epilogue and epi == "affine":
        prm = _params(ops, dev, o["w"], s, p, d, o["scale"], o["shift"], relu=True)
        kw["residual"] = o["res"].to(dev)
    else:
        prm = _params(ops, dev, o["w"], s, p, d)
        if epilogue and epi == "per-image":
            kw.update(shift_override=o["per_img"].to(dev), per_image_shift=True)
    return x, pv, prm, kw


def _conv(ops, x, prm, pv, tile, **kw):
    ho, wo = ops.conv_out_size(x.shape[1], prm.kh, prm.stride, prm.pad, prm.dil), ops.conv_out_size(x.shape[2], prm.kw, prm.stride, prm.pad, prm.dil)
    out = torch.full((x.shape[0], ho, wo, prm.cout), float("nan"), device=x.device)
    ops.conv2d(x, prm, out=out, pad_value=pv, tile=tile, **kw)
    return out


# ---- piece probes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("probe", A.PROBES, ids=A.probe_id)
def test_every_id_is_exact_on_the_piece_probes(hip_lib, dev, probe):
    from pemp_amd import ops
    q = A.probe_problem(probe)
    ref = A.conv_f64(q["x"], q["w"], q["stride"], q["pad"], q["dil"], q["pv"])
    want = ref.float().to(dev)
    assert torch.equal(want.double().cpu(), ref)
    x, pv = _layout(dev, q["x"], q["pv"])
    prm = _params(ops, dev, q["w"], q["stride"], q["pad"], q["dil"])
    assert A.family_takes(ops, x, prm, pv)
    for tile in A.S3_IDS:
        y = _conv(ops, x, prm, pv, tile)
        bad = y != want
        assert not bool(bad.any()), (A.probe_id(probe), tile, int(bad.sum()), bad.nonzero()[:4].tolist(), (y - want)[bad][:4].tolist())
        assert torch.equal(_conv(ops, x, prm, pv, tile), want), (A.probe_id(probe), tile, "second launch")


# ---- fuzz: accuracy against float64, bit identity among the unsplit ids -----------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=A.case_id)
def test_fuzz_accuracy_and_bit_identity(hip_lib, dev, case):
    """Every id against the float64 convolution with the epilogue.  Printed per id: the error (maximum and rms, relative to
    conv(|x|, |w|) through the epilogue's magnitudes) as a multiple of the yardstick's, torch's CPU fp32 conv2d."""
    from pemp_amd import ops
    ref, mag, (ymax, yrms) = A.fuzz_reference(case)
    x, pv, prm, kw = _case_on_device(ops, dev, case)
    if not A.family_takes(ops, x, prm, pv):
        print(f"split3 fuzz {A.case_id(case)}: outside the family (counted by test_the_skipped_share_is_small)")
        return
    first = _conv(ops, x, prm, pv, 43, **kw)
    over, bound = [], A.ratio_bound(case[3] * case[5] ** 2)
    for tile in _ids(ops, case[4]):
        y = first if tile == 43 else _conv(ops, x, prm, pv, tile, **kw)
        if tile in A.S3_UNSPLIT:
            bad = y != first
            assert not bool(bad.any()), (case, tile, "differs from id 43", int(bad.sum()), bad.nonzero()[:4].tolist())
            if tile != 43:
                continue
        emax, erms = A.errors(y.cpu(), ref, mag)
        what = "unsplit ids" if tile == 43 else f"id {tile}"
        print(f"split3 fuzz {A.case_id(case)} | K {case[3] * case[5] ** 2} | {what} | max {emax:.2e} = x{emax / ymax:.2f} | "
              f"rms {erms:.2e} = x{erms / yrms:.2f} | yardstick max {ymax:.2e} rms {yrms:.2e}")
        if emax > bound * ymax or erms > bound * yrms:
            over.append((tile, emax / ymax, erms / yrms))
    assert not over, (case, bound, over)


def test_the_skipped_share_is_small(hip_lib, dev):
    """With the buffers as the tests above build them: at most 10 % of the (case, id) pairs lie outside the family, and every id
    runs on at least 10 cases."""
    from pemp_amd import ops
    pairs = skipped = 0
    runs = {t: 0 for t in A.S3_IDS}
    for case in CASES:
        x, pv, prm, _ = _case_on_device(ops, dev, case)
        ok = A.family_takes(ops, x, prm, pv)
        for t in _ids(ops, case[4]):
            pairs += 1
            skipped += int(not ok)
            runs[t] += int(ok)
    print(f"split3 fuzz: skipped {skipped} of {pairs} (case, id) pairs = {100.0 * skipped / pairs:.1f} %; cases per id {runs}")
    assert skipped <= 0.10 * pairs, (skipped, pairs)
    assert min(runs.values()) >= 10, runs


def _groups():
    """Cases a grouped launch can take together (no per-image shift; padding values for all members or for none), in twos and
    threes."""
    out = []
    for padv in (False, True):
        rows = [c for c in CASES if c[9] != "per-image" and (c[5] > 1) == padv]
        while rows:
            n = 3 if len(rows) != 4 and len(rows) != 2 else 2
            out.append(tuple(rows[:n]))
            rows = rows[n:]
    return [g for g in out if len(g) > 1]


@pytest.mark.parametrize("group", _groups(), ids=lambda g: "+".join(A.case_id(c) for c in g))
def test_grouped_launch_equals_the_single_launches(hip_lib, dev, group):
    from pemp_amd import ops
    members = [_case_on_device(ops, dev, c) for c in group]
    if not all(A.family_takes(ops, x, prm, pv) for x, pv, prm, _ in members):
        print("split3 fuzz group: a member lies outside the family")
        return
    singles = [_conv(ops, x, prm, pv, 43, **kw) for x, pv, prm, kw in members]
    ran = 0
    for tile in GROUPABLE:
        if any(c[4] % ops._tile_bn(tile) for c in group):
            continue
        outs = [torch.full_like(s, float("nan")) for s in singles]
        pvs = [m[1] for m in members]
        ops.conv2d_group([m[0] for m in members], [m[2] for m in members], outs, pad_values=None if pvs[0] is None else pvs,
                         residuals=[m[3].get("residual") for m in members], tile=tile)
        for c, o, s in zip(group, outs, singles):
            bad = o != s
            assert not bool(bad.any()), (tile, c, int(bad.sum()), bad.nonzero()[:4].tolist())
        ran += 1
    assert ran >= 2            # 42 and 43 take every Cout


def test_groups_cover_twos_and_threes():
    sizes = {len(g) for g in _groups()}
    assert sizes == {2, 3}, sizes
    assert any(c[5] > 1 for g in _groups() for c in g) and any(c[5] == 1 for g in _groups() for c in g)


# ---- output windows ---------------------------------------------------------------------------------------------------------------
WINDOW_CASES = [next(c for c in CASES if c[9] == epi) for epi in A.EPILOGUES]


@pytest.mark.parametrize("case", WINDOW_CASES, ids=A.case_id)
def test_a_channel_window_is_written_and_nothing_else(hip_lib, dev, case):
    from pemp_amd import ops
    x, pv, prm, kw = _case_on_device(ops, dev, case)
    assert A.family_takes(ops, x, prm, pv)
    want = _conv(ops, x, prm, pv, 43, **kw)
    cout = case[4]
    for tile in _ids(ops, cout):
        if tile in A.S3_SPLITK:
            want_t = _conv(ops, x, prm, pv, tile, **kw)
        else:
            want_t = want
        big = torch.full(tuple(want.shape[:3]) + (cout + 128,), -7.5, device=dev)
        ops.conv2d(x, prm, out=big[..., 64:64 + cout], pad_value=pv, tile=tile, **kw)
        assert torch.equal(big[..., 64:64 + cout], want_t), (case, tile)
        assert bool((big[..., :64] == -7.5).all()) and bool((big[..., 64 + cout:] == -7.5).all()), (case, tile)


# ---- power-of-two scaling -----------------------------------------------------------------------------------------------------------
SCALING_CASES = [c for c in CASES if c[4] % 128 == 0][:4]
SCALING_IDS = (43, 46, 49)
SCALING_EXPONENTS = ((40, -40), (-40, 40), (30, 30), (-30, -30))


@pytest.mark.parametrize("case", SCALING_CASES, ids=A.case_id)
def test_power_of_two_scaling_changes_no_bit(hip_lib, dev, case):
    """conv(2^a x, 2^b w) == 2^(a + b) conv(x, w), bit for bit: the splits and the fp32 products of bf16 pieces commute with a
    power of two while nothing leaves the normal range (all four exponent pairs stay inside it).  No epilogue; the padding value
    is scaled with the activations."""
    from pemp_amd import ops
    N, H, W, cin, cout, k, s, p, d, epi = case
    o = A.fuzz_operands(case)
    x, pv = _layout(dev, o["x"], o["pv"])
    prm = _params(ops, dev, o["w"], s, p, d)
    assert A.family_takes(ops, x, prm, pv)
    for tile in SCALING_IDS:
        base = _conv(ops, x, prm, pv, tile)
        assert bool(base.abs().sum() > 0)
        for a, b in SCALING_EXPONENTS:
            xs, pvs = _layout(dev, o["x"] * 2.0 ** a, None if o["pv"] is None else o["pv"] * 2.0 ** a)
            got = _conv(ops, xs, _params(ops, dev, o["w"] * 2.0 ** b, s, p, d), pvs, tile)
            want = base * 2.0 ** (a + b)
            assert bool(want.isfinite().all())
            bad = got != want
            assert not bool(bad.any()), (case, tile, a, b, int(bad.sum()), bad.nonzero()[:4].tolist())


# ---- the in-register activation split -----------------------------------------------------------------------------------------------
def test_the_activation_split_loses_nothing_on_the_hard_values(hip_lib, dev):
    """Activations from the hard values of the weight split's tests (1 + 2^-23, -(1 + 2^-9 + 2^-17), negatives, 1e-20 and 1e30
    scales, 2^-126) through a 1x1 conv whose weights are one power of two per output channel: the output is that input channel,
    scaled, exactly -- on every id.  The kernels add l w, m w, h w in that order, and l + m and l + m + h are fp32 values; a split
    that does not satisfy h + m + l == x shows here."""
    from pemp_amd import ops
    cin, cout = 96, 256
    rows = [w if w.shape[1] == cin else w.repeat(1, cin // w.shape[1]) for w in _split_cases()]
    N, H, W = 1, 19, 20                                           # 380 of the 384 rows: M is no multiple of a block's rows
    x = torch.cat(rows)[:N * H * W].view(N, H, W, cin).contiguous()
    assert bool((x == 1.0 + 2.0 ** -23).any()) and bool((x == 2.0 ** -126).any()) and bool((x.abs() > 1e29).any())
    n = torch.arange(cout)
    ch = (n * 7 + 3) % cin
    # channels 3 mod 4 carry 2^-126 in the last block of rows: no negative exponent there, the product must stay a normal number
    ex = torch.where(ch % 4 == 3, n % 3, n % 6 - 2)
    w = torch.zeros(cout, cin, 1, 1)
    w[n, ch, 0, 0] = 2.0 ** ex.float()
    want = x.double()[..., ch] * 2.0 ** ex.double()
    assert torch.equal(want.float().double(), want) and bool(((want == 0) | (want.abs() >= 2.0 ** -126)).all())
    want = want.float().to(dev)
    xd, _ = _layout(dev, x, None)
    prm = _params(ops, dev, w, 1, 0, 1)
    for tile in A.S3_IDS:
        y = _conv(ops, xd, prm, None, tile)
        bad = y != want
        assert not bool(bad.any()), (tile, int(bad.sum()), bad.nonzero()[:4].tolist(), y[bad][:4].tolist(), want[bad][:4].tolist())
