"""PFENet support banks at kernel level (csrc/pfenet.hip: prior_bank_pack_kernel, prior_bank_kernel): the packed support operand
against a torch gather, and the bank prior against ``ops.prior_mask`` on the supports the bank was packed from -- bit for bit, for
every (query, class) pair, with and without an index.

Every case has K = 3 classes: class 0 with a full mask (fractional values, no zero row: count == HW), class 1 with an empty mask
(count == 1, the prior is exactly 0) and class 2 with exactly 64 non-zero pixels per shot (count == 65: the zero row alone opens a
second support tile).  A 7 x 7 map has 49 pixels, so there class 2 has 48 non-zero pixels (count == 49 == HW, the zero row is the
map's last row of the only tile).  The store is one tile larger than any count needs and everything beyond ``count`` is set to NaN
after packing: a kernel that read it could not give finite, equal results."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

K, N, INDEX = 3, 4, [2, 0, 2, 1]          # a repeated and a permuted class
CASES = [(1, 9, 11, 64, False),           # tails in both tile directions
         (1, 9, 11, 64, True),            # signed features: a masked pixel's products are -0 as well as +0
         (2, 13, 13, 2048, False),        # the long K loop
         (5, 7, 7, 96, False),
         (1, 51, 51, 512, False)]         # 41 support tiles for the full mask


@functools.lru_cache(maxsize=None)
def _case(S, h, w, C, signed):
    """-> (qry [N,h,w,C], sup [K*S,h,w,C], mask [K*S,h,w]) on the CPU, made like tests/test_pfenet_gpu.py's _feats / _mask."""
    gen = torch.Generator().manual_seed(1000 * S + 10 * h + C + int(signed))
    if signed:
        feats = lambda shape: torch.randn(shape, generator=gen)
    else:
        feats = lambda shape: (torch.rand(shape, generator=gen) - 0.3).clamp_min(0.0)      # post-ReLU-like
    q, s = feats((N, h, w, C)), feats((K * S, h, w, C))
    frac = torch.rand((K * S, h * w), generator=gen).clamp_min(0.5)                        # fractional mask values, never 0
    m = torch.zeros((K, S, h * w))
    m[0] = frac.view(K, S, -1)[0]
    some = min(64, h * w - 1)
    for si in range(S):
        keep = torch.randperm(h * w, generator=gen)[:some]
        m[2, si, keep] = frac.view(K, S, -1)[2, si, keep]
    return q, s, m.view(K * S, h, w).contiguous()


def _packed(ops, dev, S, h, w, C, signed, poison=True):
    q, s, m = _case(S, h, w, C, signed)
    cap = ops._round64(h * w) + 64
    rows, norms, count = ops.prior_bank_pack(s.to(dev), m.to(dev), K, S, cap=cap)
    if poison:
        beyond = torch.arange(cap, device=dev)[None, None, :] >= count[:, :, None]
        rows[beyond] = float("nan")
        norms[beyond] = float("nan")
    return q.to(dev), s.to(dev), m.to(dev), rows, norms, count


@pytest.mark.parametrize("S,h,w,C,signed", CASES)
def test_bank_prior_equals_prior_mask_bit_for_bit(hip_lib, dev, S, h, w, C, signed):
    from pemp_amd import ops
    q, s, m, rows, norms, count = _packed(ops, dev, S, h, w, C, signed)
    some = min(64, h * w - 1)
    assert count.cpu().tolist() == [[h * w] * S, [1] * S, [some + 1] * S]
    ref = torch.stack([torch.stack([ops.prior_mask(q[n:n + 1], s[k * S:(k + 1) * S], m[k * S:(k + 1) * S], S)[0] for k in range(K)])
                       for n in range(N)])                                                  # [N,K,h,w]
    every = ops.prior_bank(q, rows, norms, count)
    assert every.shape == (N, K, h, w) and torch.isfinite(every).all()
    for n in range(N):
        for k in range(K):
            assert torch.equal(every[n, k], ref[n, k]), (n, k, (every[n, k] - ref[n, k]).abs().max().item())
    assert (every[:, 1] == 0).all()                      # the empty mask: one zero row, exactly 0
    assert ref[:, 0].max() > 0.5 and ref[:, 2].max() > 0.5 and not torch.equal(ref[:, 0], ref[:, 2])
    picked = ops.prior_bank(q, rows, norms, count, index=INDEX)
    assert picked.shape == (N, h, w)
    for n, k in enumerate(INDEX):
        assert torch.equal(picked[n], ref[n, k]), (n, k)
    # a device index through the launch wrapper (what a captured graph replays), into a given buffer
    out = torch.full((N, h, w), 7.0, device=dev)
    idx = torch.tensor(INDEX[::-1], dtype=torch.int32, device=dev)
    assert ops._prior_bank(q, rows, norms, count, idx, out=out) is out
    for n, k in enumerate(INDEX[::-1]):
        assert torch.equal(out[n], ref[n, k]), (n, k)
    assert torch.equal(ops.prior_bank(q, rows, norms, count), every)                      # bit-stable


@pytest.mark.parametrize("S,h,w,C,signed", [c for c in CASES if c[1] != 51])
def test_pack_stores_the_foreground_rows_in_pixel_order(hip_lib, dev, S, h, w, C, signed):
    from pemp_amd import ops
    q, s, m, rows, norms, count = _packed(ops, dev, S, h, w, C, signed, poison=False)
    again = _packed(ops, dev, S, h, w, C, signed, poison=False)
    assert all(torch.equal(a, b) for a, b in zip((rows, norms, count), again[3:]))          # pack twice: identical
    rows, norms, count = rows.cpu(), norms.cpu(), count.cpu()
    _, sc, mc = _case(S, h, w, C, signed)
    sc, mc = sc.view(K, S, h * w, C), mc.view(K, S, h * w)
    for k in range(K):
        for si in range(S):
            fg = (mc[k, si] != 0).nonzero()[:, 0]                                           # ascending: pixel order
            nnz = fg.numel()
            assert int(count[k, si]) == nnz + (1 if nnz < h * w else 0)
            want = sc[k, si, fg] * mc[k, si, fg, None]                                      # fl(m * s): one fp32 product each
            assert torch.equal(rows[k, si, :nnz], want), (k, si)
            if nnz:
                # an fp32 sum of positive terms: a lane's chain is C / 8 fmas long, then 3 butterfly adds and the square root, each
                # within 2^-24 relative -- (C / 8 + 8) 2^-24 bounds the norm's relative error with room; its exact value is pinned by
                # the bit-equality test above
                wn = want.double().norm(dim=1)
                assert ((norms[k, si, :nnz].double() - wn).abs() <= (C / 8 + 8) * 2.0 ** -24 * wn).all(), (k, si)
            if nnz < h * w:
                assert (rows[k, si, nnz] == 0).all() and norms[k, si, nnz] == 0               # the one zero row
            n_stored = int(count[k, si])
            assert (rows[k, si, n_stored:] == 0).all() and (norms[k, si, n_stored:] == 0).all()   # never written (a new store is zeroed)
    # the count-only form agrees
    assert torch.equal(ops.prior_bank_count(m, K, S).cpu(), count)


def test_pack_into_a_store_that_is_too_small_reports_the_need_and_stays_inside(hip_lib, dev):
    """Class 0 needs HW = 99 rows; with cap = 64 its slot keeps the first 64 and ``count`` still says 99 (the caller compares it
    with cap); the neighbouring slots hold what they hold in a store that is large enough."""
    from pemp_amd import ops
    S, h, w, C = 1, 9, 11, 64
    _, s, m = _case(S, h, w, C, False)
    big = ops.prior_bank_pack(s.to(dev), m.to(dev), K, S, cap=128)
    rows, norms, count = ops.prior_bank_pack(s.to(dev), m.to(dev), K, S, cap=64)
    assert count.cpu().tolist() == [[99], [1], [65]]
    assert torch.equal(rows[0, :, :64], big[0][0, :, :64]) and torch.equal(norms[0, :, :64], big[1][0, :, :64])
    assert torch.equal(rows[1], big[0][1, :, :64]) and torch.equal(rows[2], big[0][2, :, :64])     # class 2's zero row (row 64) is dropped
    assert torch.equal(norms[1:], big[1][1:, :, :64])


def test_host_checks_refuse_bad_arguments(hip_lib, dev):
    from pemp_amd import ops
    S, h, w, C = 1, 9, 11, 64
    q, s, m, rows, norms, count = _packed(ops, dev, S, h, w, C, False)
    for bad in ([0, 3, 0, 0], [0, -1, 0, 0], [0, 1, 2], torch.tensor([0, 1, 2, 3])):
        with pytest.raises(ValueError, match="index"):
            ops.prior_bank(q, rows, norms, count, index=bad)
    with pytest.raises(ValueError, match="CPU tensor"):                  # the checked entry wants the index where it can read it
        ops.prior_bank(q, rows, norms, count, index=torch.tensor(INDEX, device=dev))
    with pytest.raises(ValueError, match="device index"):                # the launch wrapper wants it on the device
        ops._prior_bank(q, rows, norms, count, torch.tensor(INDEX, dtype=torch.int32))
    with pytest.raises(ValueError, match="device index"):
        ops._prior_bank(q, rows, norms, count, torch.tensor(INDEX, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.prior_bank(q, rows[:, :, :100].contiguous(), norms[:, :, :100].contiguous(), count)
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.prior_bank_pack(s, m, K, S, cap=100)
    with pytest.raises(ValueError, match="C = 64"):
        ops.prior_bank(torch.zeros((N, h, w, 96), device=dev), rows, norms, count)
    with pytest.raises(ValueError, match="C=64"):
        ops.prior_bank_pack(torch.zeros((K * S, h, w, 96), device=dev), m, K, S, rows=rows, norms=norms, count=count)
    with pytest.raises(ValueError, match="norms"):
        ops.prior_bank(q, rows, norms[:, :, :64].contiguous(), count)
    with pytest.raises(ValueError, match="count"):
        ops.prior_bank(q, rows, norms, count.long())
