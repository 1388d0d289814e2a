"""The arbiter of the split3 conv family's fuzz tests (tests/test_conv_split3_fuzz_gpu.py), on the CPU: an emulator of the family's
arithmetic as DESIGN.md (Split3) states it, six exact piece probes -- one per kept bf16 product -- a seeded generator of awkward
conv geometries, and the proof that the random-data bound of the GPU file would see a dropped product.

Names: a product is written (activation piece)(weight piece), as in DESIGN.md: lh = x.l * w.h.  The kernels keep lh, hl, mm, mh,
hm, hh and drop ml, lm, ll.  Nothing here is kernel code; it restates the design so that the kernels can be held to it."""
import functools
import random

import pytest
import torch
import torch.nn.functional as F

from tests.test_conv_split3_cpu import _cases as _split_cases, split3_reference

PRODUCTS = ("lh", "hl", "mm", "mh", "hm", "hh")          # the kept ones, in the kernels' order (smallest first)
DROPPED = ("ml", "lm", "ll")
S3_UNSPLIT = (41, 42, 43, 44, 46, 47, 49)                # bit-identical among themselves (47, 49: persistent forms of 43, 46)
S3_SPLITK = (51, 52, 54, 56)
S3_IDS = S3_UNSPLIT + S3_SPLITK

#: What the GPU file allows for (split3 error) / (error of torch's CPU fp32 conv2d), both against float64 and relative to
#: conv(|x|, |w|), in maximum and in rms: 1.5 x the largest ratio measured on one MI355X over every fuzz case and id, and over the
#: shapes of test_conv_split3_gpu.py's random-data test (Split3, carries the table: 7.89 at K = 6400, in the maximum).
#: The kernels add their products to one fp32 accumulator in K order, so their relative error does not fall with K; the
#: yardstick's blocked sums do (3e-8 at K = 6400 against 2e-7 at K = 64), and the ratio grows with K.
RATIO_BOUND = 11.8
#: The cases of K <= SMALL_K are held to their own largest measured ratio (2.75) x 1.5 as well.  At RATIO_BOUND alone a dropped
#: 2^-17-level product (5 to 30 x the yardstick's error there) would pass; at this bound it fails in every such case, which
#: test_the_random_data_bound_sees_a_dropped_product asserts.
RATIO_BOUND_SMALL_K, SMALL_K = 4.1, 576


def ratio_bound(K):
    """The allowed (split3 error) / (yardstick error) of a conv with K = Cin * taps."""
    return RATIO_BOUND_SMALL_K if K <= SMALL_K else RATIO_BOUND


# ---- the emulator -------------------------------------------------------------------------------------------------------------
def split3(t):
    """fp32 tensor -> its pieces {"h", "m", "l"} as float64 tensors: split3_reference's arithmetic (round to nearest even to bf16
    at each stage, differences in fp32), element by element."""
    assert t.dtype == torch.float32
    h = t.to(torch.bfloat16)
    r = t - h.float()
    m = r.to(torch.bfloat16)
    l = (r - m.float()).to(torch.bfloat16)
    return {"h": h.double(), "m": m.double(), "l": l.double()}


def padded_nchw(x, pad, pad_value=None):
    """NHWC [N, H, W, C] -> NCHW with `pad` pixels of `pad_value` ([C], or zero) around the image; same dtype."""
    N, H, W, C = x.shape
    xp = torch.zeros(N, C, H + 2 * pad, W + 2 * pad, dtype=x.dtype)
    if pad_value is not None:
        xp[:] = pad_value.to(x.dtype).view(1, C, 1, 1)
    xp[:, :, pad:pad + H, pad:pad + W] = x.permute(0, 3, 1, 2)
    return xp


def _conv_nhwc(xp, w, stride, dil):
    return F.conv2d(xp, w, None, stride, 0, dil).permute(0, 2, 3, 1).contiguous()


def conv_f64(x, w, stride=1, pad=0, dil=1, pad_value=None):
    """float64 convolution of the fp32 operands: x NHWC, w OIHW -> NHWC."""
    return _conv_nhwc(padded_nchw(x, pad, pad_value).double(), w.double(), stride, dil)


def split3_products(x, w, stride=1, pad=0, dil=1, pad_value=None, which=PRODUCTS):
    """{product: float64 NHWC convolution of that pair of pieces}.  The padding is applied in fp32 before the split, as in the
    kernels (padding values reach LDS as fp32 and are split in registers like any activation)."""
    xs, ws = split3(padded_nchw(x, pad, pad_value)), split3(w)
    return {pq: _conv_nhwc(xs[pq[0]], ws[pq[1]], stride, dil) for pq in which}


def split3_conv_emulated(x, w, stride=1, pad=0, dil=1, pad_value=None, drop=None):
    """The split3 family's convolution with exact accumulation: both fp32 operands split as split3_reference does, the six kept
    products formed and summed in float64.  `drop` names one kept product to leave out (what a kernel that lost it would give)."""
    assert drop is None or drop in PRODUCTS
    prods = split3_products(x, w, stride, pad, dil, pad_value, which=[pq for pq in PRODUCTS if pq != drop])
    return sum(prods.values())


# ---- piece probes -------------------------------------------------------------------------------------------------------------
# Tables of fp32 values whose pieces are known integers times a power of two.  Values with one piece (h only):
_SMALL = [1.0, -2.0, 3.0, -1.0, 2.0, -3.0]
_BYTE = [129.0, -255.0, 171.0, -201.0, 147.0, -233.0, 219.0, -135.0, 253.0, -187.0]
# two pieces: h in {128, 192} (bf16 spacing 1 there), |m| < 1/2 a multiple of 2^-3 -- never 128 - m (a tie at the binade's edge)
_TWO = [s * (h + m) for s in (1.0, -1.0) for h, m in ((128.0, 0.25), (128.0, 0.375), (192.0, 0.25), (192.0, -0.375), (192.0, 0.375),
                                                        (192.0, -0.25))]
# three pieces: h a multiple of 16 in [128, 256), m a multiple of 2^-4 in (1/4, 1/2) (bf16 spacing 2^-9), |l| <= 2^-11 a multiple
# of 2^-12: 20 significant bits, so that a few products with a one-piece partner stay below 2^24 units
_THREE = [s * (h + m + l) for s in (1.0, -1.0) for h in (144.0, 160.0, 192.0, 208.0) for m in (0.3125, -0.375, 0.4375, -0.3125)
          for l in (2.0 ** -11, -3 * 2.0 ** -12, 3 * 2.0 ** -12, -2.0 ** -11)]
# kind -> (table, unit every piece of every entry is a multiple of, number of non-zero pieces)
_KINDS = {"small": (_SMALL, 1.0, 1), "byte": (_BYTE, 1.0, 1), "two": (_TWO, 2.0 ** -3, 2), "three": (_THREE, 2.0 ** -12, 3)}
# product -> (kind of the activations, kind of the weights): each operand carries its pieces down to the named one and no further,
# so the dropped products (ml, lm, ll) cannot occur and the named product is the smallest one present
PROBE_KINDS = {"hh": ("byte", "byte"), "mh": ("two", "byte"), "hm": ("byte", "two"), "mm": ("two", "two"),
               "lh": ("three", "small"), "hl": ("small", "three")}
X_SCALE, W_SCALE = 2.0 ** -7, 2.0 ** -9
PROBE_COUT, PROBE_TERMS = 256, 4
# (N, H, W, Cin, k, stride, pad, dil, padding value): none a multiple of a block shape.  A 1x1 over three K steps (M = 231); a
# dilated 3x3 whose padding (3) is not its dilation (2), with a padding value (M = 330); a strided 3x3, zero padding (M = 60)
PROBE_GEOMS = [(3, 7, 11, 96, 1, 1, 0, 1, False), (2, 9, 13, 32, 3, 1, 3, 2, True), (2, 11, 9, 96, 3, 2, 1, 1, False)]
PROBES = [(pq, g) for pq in PRODUCTS for g in PROBE_GEOMS]


def probe_id(probe):
    return probe[0] + "-" + "x".join(str(int(v)) for v in probe[1])


def probe_problem(probe):
    """-> dict(x NHWC fp32, w OIHW fp32, pv [Cin] fp32 or None, stride, pad, dil, ux, uw).  Activations are dense, weights have
    PROBE_TERMS entries per output channel at (tap, channel) positions that move with the channel, so an output has at most
    PROBE_TERMS terms per product."""
    pq, (N, H, W, Cin, k, s, p, d, padv) = probe
    (xt, ux, _), (wt, uw, _) = _KINDS[PROBE_KINDS[pq][0]], _KINDS[PROBE_KINDS[pq][1]]
    xt, wt = torch.tensor(xt, dtype=torch.float64), torch.tensor(wt, dtype=torch.float64)
    m = torch.arange(N * H * W)
    c = torch.arange(Cin)
    x = xt[(m[:, None] * 7 + c[None, :] * 13 + 3) % len(xt)].view(N, H, W, Cin) * X_SCALE
    pv = xt[(c * 5 + 1) % len(xt)] * X_SCALE if padv else None
    w = torch.zeros(PROBE_COUT, Cin, k, k, dtype=torch.float64)
    n = torch.arange(PROBE_COUT)
    for i in range(PROBE_TERMS):
        tap = (n + 2 * i) % (k * k)
        w[n, (5 * n + 7 * i + 1) % Cin, tap // k, tap % k] = wt[(n + 3 * i) % len(wt)] * W_SCALE
    assert int((w != 0).sum()) == PROBE_COUT * PROBE_TERMS
    for t in (x, w) + ((pv,) if padv else ()):
        assert torch.equal(t.float().double(), t)                 # the operands are fp32 values
    return dict(x=x.float(), w=w.float(), pv=None if pv is None else pv.float(), stride=s, pad=p, dil=d, ux=ux * X_SCALE, uw=uw * W_SCALE)


@pytest.mark.parametrize("probe", PROBES, ids=probe_id)
def test_piece_probe_is_exact_and_sees_its_product(probe):
    pq = probe[0]
    q = probe_problem(probe)
    geo = dict(stride=q["stride"], pad=q["pad"], dil=q["dil"], pad_value=q["pv"])
    ref = conv_f64(q["x"], q["w"], **geo)
    M = ref.numel() // PROBE_COUT
    assert M % 64 != 0
    # the operands carry exactly the pieces their kind promises, each a multiple of the operand's unit
    xs, ws = split3(padded_nchw(q["x"], q["pad"], q["pv"])), split3(q["w"])
    for pieces, unit, kind in ((xs, q["ux"], PROBE_KINDS[pq][0]), (ws, q["uw"], PROBE_KINDS[pq][1])):
        for i, name in enumerate("hml"):
            assert torch.equal((pieces[name] / unit).round() * unit, pieces[name]), (name, kind)
            assert bool((pieces[name] != 0).any()) == (i < _KINDS[kind][2]), (name, kind)
    assert bool((xs[pq[0]] != 0).any()) and bool((ws[pq[1]] != 0).any())
    # (a) the float64 convolution is an fp32 value
    assert torch.equal(ref.float().double(), ref)
    # (b) every term of every kept product is a multiple of ux * uw, and the magnitudes of all terms of one output sum to less
    # than 2^24 units: every partial sum of every subset is an integer below 2^24 units, exact in fp32 in any order
    unit = q["ux"] * q["uw"]
    mags = sum(_conv_nhwc(xs[a].abs(), ws[b].abs(), q["stride"], q["dil"]) for a, b in PRODUCTS)
    assert mags.max().item() < 2 ** 24 * unit, (mags.max().item() / unit, 2 ** 24)
    assert bool((ref != 0).float().mean() > 0.5)
    # (c) the dropped products do not occur
    for a, b in DROPPED:
        assert _conv_nhwc(xs[a].abs(), ws[b].abs(), q["stride"], q["dil"]).max().item() == 0.0, a + b
    # the emulator agrees with float64 where nothing is dropped, and (d) loses the named product in a quarter of the outputs
    assert torch.equal(split3_conv_emulated(q["x"], q["w"], **geo), ref)
    off = split3_conv_emulated(q["x"], q["w"], drop=pq, **geo) != ref
    assert off.float().mean().item() >= 0.25, off.float().mean().item()


def test_the_emulators_split_is_the_reference_split():
    for w in _split_cases():
        s, mine = split3_reference(w), split3(w)
        for i, name in enumerate("hml"):
            assert torch.equal(s[:, :, i].reshape(w.shape).double(), mine[name]), name


def test_a_wrong_weight_plane_or_a_lost_activation_piece_changes_a_probe():
    """The two mutations the probes are meant for, played on the emulator: weights whose l plane repeats the m plane, and
    activations without their l piece.  Each changes at least one probe."""
    hit_w = hit_x = 0
    for probe in PROBES:
        q = probe_problem(probe)
        xs, ws = split3(padded_nchw(q["x"], q["pad"], q["pv"])), split3(q["w"])
        ref = conv_f64(q["x"], q["w"], q["stride"], q["pad"], q["dil"], q["pv"])
        conv = lambda a, b: _conv_nhwc(a, b, q["stride"], q["dil"])
        wrong_w = sum(conv(xs[a], ws["m" if b == "l" else b]) for a, b in PRODUCTS)
        wrong_x = sum(conv(xs[a], ws[b]) for a, b in PRODUCTS if a != "l")
        hit_w += int(not torch.equal(wrong_w, ref))
        hit_x += int(not torch.equal(wrong_x, ref))
    assert hit_w >= len(PROBE_GEOMS) and hit_x >= len(PROBE_GEOMS), (hit_w, hit_x)


# ---- fuzz cases, shared with the GPU file ----------------------------------------------------------------------------------------
EPILOGUES = ("none", "affine", "per-image")     # none; scale + shift + residual + ReLU; a per-image shift
N_CASES, SEED = 24, 2033


def fuzz_cases(n=N_CASES, seed=SEED):
    """n cases (N, H, W, Cin, Cout, k, stride, pad, dil, epilogue), every one a geometry engine.with_split3 attaches split weights
    to (no stem, <= 32 taps, Cin % 32 == 0, Cout % 64 == 0)."""
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        k = rng.choice((1, 1, 3, 3, 5))
        s = rng.choice((1, 1, 2))
        d = rng.choice((1, 1, 2, 3, 6))
        p = rng.choice((0, d * (k // 2), d * (k // 2) + 1, 1))
        H, W, N = rng.randint(3, 37), rng.randint(3, 37), rng.randint(1, 5)
        cin, cout = rng.choice((32, 64, 96, 160, 256)), rng.choice((64, 128, 192, 256, 320, 512))
        epi = rng.choice(EPILOGUES)
        if H + 2 * p < d * (k - 1) + 1 or W + 2 * p < d * (k - 1) + 1:
            continue
        assert k * k <= 32 and cin % 32 == 0 and cout % 64 == 0
        out.append((N, H, W, cin, cout, k, s, p, d, epi))
    return out


def case_id(case):
    return "x".join(str(v) for v in case)


def out_hw(case):
    N, H, W, cin, cout, k, s, p, d, epi = case
    return (H + 2 * p - d * (k - 1) - 1) // s + 1, (W + 2 * p - d * (k - 1) - 1) // s + 1


def fuzz_operands(case):
    """The case's CPU operands: x NHWC, w OIHW (unit-variance outputs), pv [Cin] where k > 1 (else None), and the epilogue's
    tensors: scale, shift [Cout], res [N, Ho, Wo, Cout] for "affine", per_img [N, Cout] for "per-image"."""
    N, H, W, cin, cout, k, s, p, d, epi = case
    seed = 0
    for v in case[:9]:
        seed = (seed * 131 + v) % (2 ** 31 - 1)
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=g)
    ho, wo = out_hw(case)
    o = dict(x=r(N, H, W, cin), w=r(cout, cin, k, k) / (cin * k * k) ** 0.5, pv=r(cin) if k > 1 else None)
    if epi == "affine":
        o.update(scale=torch.rand(cout, generator=g) + 0.5, shift=r(cout), res=r(N, ho, wo, cout))
    elif epi == "per-image":
        o.update(per_img=r(N, cout))
    return o


def epilogue(y, o, case):
    """The case's epilogue on an NHWC convolution result, in y's precision."""
    epi = case[9]
    if epi == "affine":
        return F.relu(y * o["scale"].to(y.dtype) + o["shift"].to(y.dtype) + o["res"].to(y.dtype))
    if epi == "per-image":
        return y + o["per_img"].to(y.dtype)[:, None, None, :]
    return y


def magnitude(o, case):
    """What an error of the case's output is measured against: conv(|x|, |w|) through the epilogue's magnitudes, float64."""
    N, H, W, cin, cout, k, s, p, d, epi = case
    mag = conv_f64(o["x"].abs(), o["w"].abs(), s, p, d, None if o["pv"] is None else o["pv"].abs())
    if epi == "affine":
        return mag * o["scale"].double().abs() + o["shift"].double().abs() + o["res"].double().abs()
    if epi == "per-image":
        return mag + o["per_img"].double().abs()[:, None, None, :]
    return mag


def errors(y, ref, mag):
    """(maximum, rms) of |y - ref| / mag.  Where mag is zero (every tap of a 1x1 conv's padded border reads zero) any result
    but the exact one counts as an infinite error."""
    e = (y.double() - ref).abs()
    e = torch.where(mag > 0, e / mag.clamp_min(1e-300), torch.where(e > 0, float("inf"), 0.0).to(e.dtype))
    return e.max().item(), e.pow(2).mean().sqrt().item()


@functools.lru_cache(maxsize=None)
def fuzz_reference(case):
    """-> (float64 result with the epilogue, magnitude, (max, rms) error of the yardstick).  The yardstick is torch's CPU fp32
    conv2d of the same operands with the epilogue in fp32."""
    N, H, W, cin, cout, k, s, p, d, epi = case
    o = fuzz_operands(case)
    ref = epilogue(conv_f64(o["x"], o["w"], s, p, d, o["pv"]), o, case)
    mag = magnitude(o, case)
    yard = epilogue(_conv_nhwc(padded_nchw(o["x"], p, o["pv"]), o["w"], s, d), o, case)
    assert yard.dtype == torch.float32
    return ref, mag, errors(yard, ref, mag)


def cpu_layout(x, pv):
    """Activations with the padding vector directly behind them in one buffer, as the engines and the GPU tests lay them out."""
    N, H, W, C = x.shape
    M = N * H * W
    buf = torch.empty(M + 4, C, dtype=torch.float32)
    buf[:M] = x.reshape(M, C)
    buf[M:] = 0.0 if pv is None else pv
    return buf, buf[:M].view(N, H, W, C), (None if pv is None else buf[M])


def family_takes(ops, x, prm, pv):
    """Whether the split3 family takes this call (otherwise conv2d leaves the layer to the fp32 chain)."""
    return bool(ops.dma2_supported(x, prm) and ops._group_member_ok(x, prm, pv))


def test_the_case_set_covers_the_awkward_kinds():
    cases = fuzz_cases()
    assert len(set(c[:9] for c in cases)) == N_CASES
    kinds = {
        "stride 2, k = 1": lambda c: c[6] == 2 and c[5] == 1, "stride 2, k = 3": lambda c: c[6] == 2 and c[5] == 3,
        "k = 5": lambda c: c[5] == 5, "pad != d (k // 2)": lambda c: c[7] != c[8] * (c[5] // 2),
        "Cin = 96": lambda c: c[3] == 96, "Cin = 160": lambda c: c[3] == 160, "Cout = 64": lambda c: c[4] == 64,
        "Cout = 320": lambda c: c[4] == 320, "M < 64": lambda c: c[0] * out_hw(c)[0] * out_hw(c)[1] < 64,
        "scale + shift + residual + ReLU": lambda c: c[9] == "affine", "per-image shift": lambda c: c[9] == "per-image", "no epilogue": lambda c: c[9] == "none",
        "a padding value": lambda c: c[5] > 1, "K <= 576": lambda c: c[3] * c[5] ** 2 <= 576, "K >= 2304": lambda c: c[3] * c[5] ** 2 >= 2304,
    }
    for name, f in kinds.items():
        assert any(f(c) for c in cases), name


def test_the_family_takes_nearly_every_case_on_every_id():
    """Geometry alone: with the padding vector directly behind the activations, at most 10 % of the (case, id) pairs whose Cout the
    id's block divides lie outside the family, and every id runs on at least 10 cases."""
    from pemp_amd import ops
    pairs = skipped = 0
    runs = {t: 0 for t in S3_IDS}
    for case in fuzz_cases():
        N, H, W, cin, cout, k, s, p, d, epi = case
        _, x, pv = cpu_layout(torch.zeros(N, H, W, cin), torch.zeros(cin) if k > 1 else None)
        prm = ops.ConvParams(torch.zeros(cout, k * k * cin), None, None, cin, cout, k, k, s, p, d, k * k * cin, False, False)
        ok = family_takes(ops, x, prm, pv)
        for t in S3_IDS:
            if cout % ops._tile_bn(t) == 0:
                pairs += 1
                skipped += int(not ok)
                runs[t] += int(ok)
    print(f"split3 fuzz geometry: {skipped} of {pairs} (case, id) pairs outside the family; cases per id {runs}")
    assert skipped <= 0.10 * pairs, (skipped, pairs)
    assert min(runs.values()) >= 10, runs


@pytest.mark.parametrize("case", fuzz_cases(), ids=case_id)
def test_the_random_data_bound_sees_a_dropped_product(case):
    """At ratio_bound(K) x the yardstick's error, the emulator without one of hl, lh, hm, mm fails the GPU file's accuracy check in
    every case of K <= 576.  At larger K the bound has to leave room for the kernels' sequential fp32 sum against the yardstick's
    blocked one, and a dropped product (5 to 11 x the yardstick's error there) may hide in it: printed, not asserted.  The piece
    probes are exact at any K."""
    N, H, W, cin, cout, k, s, p, d, epi = case
    o = fuzz_operands(case)
    ref, mag, (ymax, yrms) = fuzz_reference(case)
    prods = split3_products(o["x"], o["w"], s, p, d, o["pv"])
    full = sum(prods.values())
    emax, erms = errors(epilogue(full, o, case), ref, mag)
    assert emax <= ymax and erms <= yrms, "the emulator with all six products is at least as exact as fp32"
    caught, K = {}, cin * k * k
    for pq in ("hl", "lh", "hm", "mm"):
        dmax, drms = errors(epilogue(full - prods[pq], o, case), ref, mag)
        caught[pq] = dmax > ratio_bound(K) * ymax or drms > ratio_bound(K) * yrms
        caught[pq] = (caught[pq], round(dmax / ymax, 1), round(drms / yrms, 1))
    print(f"split3 fuzz sensitivity {case_id(case)}: K {K}, bound x{ratio_bound(K)}, yardstick max {ymax:.2e} rms {yrms:.2e}, "
          + ", ".join(f"-{pq} {'caught' if c else 'MISSED'} (max x{a}, rms x{b})" for pq, (c, a, b) in caught.items()))
    if K <= SMALL_K:
        assert all(c for c, _, _ in caught.values()), caught
