"""The RPMMs bank kernel (csrc/rpmms.hip: bank_l56_kernel) against the two episode kernels it fuses: ``ops.rpmms_bank_l56`` must
EQUAL ``ops.rpmms_proto_sum`` + ``ops.rpmms_prob_map`` on operands gathered with torch, for every (query, class) pair, all-classes
and indexed; ``ops.rpmms_proto_taps`` must equal the ``taps`` scratch ``rpmms_proto_sum`` leaves.  Every comparison is
``torch.equal``.  The shapes keep what the workload's own does not reach: 3 x 3 maps have no interior pixel at dilation 2, 9 x 11
is not square and ends in a ragged pixel chunk (99 = 6 * 16 + 3)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
C = 256
LD = 288
SENTINEL = 7.0
SHAPES = [(1, 1, 3, 3), (3, 2, 3, 3), (2, 3, 9, 11), (3, 4, 13, 13), (1, 2, 51, 51)]


def _operands(N, K, h, w, dev):
    """qry and base as channel slices of wider buffers (ld > C), mu with one dead prototype side, wz, bias."""
    gen = torch.Generator().manual_seed(1000 * N + 100 * K + 10 * h + w)
    wide_q = torch.randn(N, h, w, C + 64, generator=gen)
    wide_b = torch.randn(N, h, w, C + 32, generator=gen)
    mu = torch.randn(K, 2, 10, C, generator=gen)
    mu = mu / mu.norm(dim=3, keepdim=True)
    mu[:, 0, 5] = 0.0                                               # a component that attracted no pixel
    if K > 1:
        mu[1, 1] = 0.0                                              # a dead prototype side: an all-foreground support
    wz = torch.randn(9, C, C, generator=gen) * (1.0 / (C * 9) ** 0.5)
    bias = torch.randn(C, generator=gen) * 0.1
    qry = wide_q.to(dev)[..., 32:32 + C]
    base = wide_b.to(dev)[..., 16:16 + C]
    return qry, base, bias.to(dev), mu.contiguous().to(dev), wz.contiguous().to(dev)


def _episode(qry, base, bias, mu, wz, pairs):
    """The two episode kernels on the gathered operands of ``pairs`` [(n, k)] -> ([3,P,h,w,LD], taps [P,10,9,C])."""
    from pemp_amd import ops
    ns = torch.tensor([n for n, _ in pairs], device=qry.device)
    ks = torch.tensor([k for _, k in pairs], device=qry.device)
    q, b, m = qry[ns].contiguous(), base[ns].contiguous(), mu[ks].contiguous()
    P, h, w, _ = q.shape
    out = torch.full((3, P, h, w, LD), SENTINEL, device=qry.device)
    taps = torch.empty((P, 10, 9, C), device=qry.device)
    ops.rpmms_proto_sum(wz, m, b, bias, out[..., :C], dil=2, taps=taps)
    ops.rpmms_prob_map(q, m, out)
    return out, taps


@pytest.fixture(scope="module")
def cases(hip_lib, dev):
    """Per shape the operands and the episode-path reference of every (n, k) pair, computed once."""
    made = {}
    for N, K, h, w in SHAPES:
        ops_ = _operands(N, K, h, w, dev)
        pairs = [(n, k) for n in range(N) for k in range(K)]
        ref, taps = _episode(*ops_, pairs)
        made[(N, K, h, w)] = (ops_, ref, taps)
    return made


@pytest.mark.parametrize("N,K,h,w", SHAPES)
def test_proto_taps_equals_the_scratch_of_proto_sum(cases, dev, N, K, h, w):
    from pemp_amd import ops
    (qry, base, bias, mu, wz), ref, ref_taps = cases[(N, K, h, w)]
    taps = ops.rpmms_proto_taps(wz, mu)
    assert taps.shape == (K, 10, 9, C)
    for k in range(K):
        assert torch.equal(taps[k], ref_taps[k]), k               # pair (0, k) is row k of the all-pairs reference
    into = torch.empty_like(taps)
    assert ops.rpmms_proto_taps(wz, mu, out=into) is into and torch.equal(into, taps)
    assert (taps[:, 5] == 0).all() and taps.abs().max().item() > 0  # the dead component's taps are zero, the others are not


@pytest.mark.parametrize("N,K,h,w", SHAPES)
def test_all_classes_equals_every_pair_computed_alone(cases, dev, N, K, h, w):
    from pemp_amd import ops
    (qry, base, bias, mu, wz), ref, _ = cases[(N, K, h, w)]
    taps = ops.rpmms_proto_taps(wz, mu)
    out = torch.full((3, N * K, h, w, LD), SENTINEL, device=dev)
    assert ops.rpmms_bank_l56(qry, base, bias, mu, taps, out) is out
    assert (out[..., C + 2:] == SENTINEL).all()                     # channels 258.. are not written
    assert torch.equal(out[..., :C + 2], ref[..., :C + 2])
    got = out.view(3, N, K, h, w, LD)
    for n in range(N):
        for k in range(K):
            alone, _ = _episode(qry, base, bias, mu, wz, [(n, k)])                 # the pair as a one-image episode
            assert torch.equal(got[:, n, k, :, :, :C + 2], alone[:, 0, :, :, :C + 2]), (n, k)
    assert torch.isfinite(out).all()
    if K > 1:
        assert not torch.equal(got[:, 0, 0], got[:, 0, 1])


@pytest.mark.parametrize("N,K,h,w", SHAPES)
def test_indexed_equals_the_gathered_pairs(cases, dev, N, K, h, w):
    from pemp_amd import ops
    (qry, base, bias, mu, wz), ref, _ = cases[(N, K, h, w)]
    taps = ops.rpmms_proto_taps(wz, mu)
    full = ref.view(3, N, K, h, w, LD)
    repeated = [K - 1] * N                                          # every query names one class: the others are named by nobody
    permuted = [(n + 1) % K for n in range(N)]
    for index in (repeated, permuted, torch.tensor([0] * N, dtype=torch.int64)):
        out = torch.full((3, N, h, w, LD), SENTINEL, device=dev)
        ops.rpmms_bank_l56(qry, base, bias, mu, taps, out, index=index)
        assert (out[..., C + 2:] == SENTINEL).all()
        for n, k in enumerate(int(v) for v in index):
            assert torch.equal(out[:, n, :, :, :C + 2], full[:, n, k, :, :, :C + 2]), (list(index), n)
    # the launch wrapper of captured graphs takes the same index from the device
    idx_dev = torch.tensor(permuted, dtype=torch.int32, device=dev)
    a = torch.full((3, N, h, w, LD), SENTINEL, device=dev)
    ops._rpmms_bank_l56(qry, base, bias, mu, taps, a, idx_dev)
    b = torch.full((3, N, h, w, LD), SENTINEL, device=dev)
    ops.rpmms_bank_l56(qry, base, bias, mu, taps, b, index=permuted)
    assert torch.equal(a, b)


def test_a_pair_does_not_depend_on_n_k_or_its_position(cases, dev):
    """Query 1 against class 2 of the 9 x 11 case: alone in a bank of one, and inside the full call."""
    from pemp_amd import ops
    N, K, h, w = 2, 3, 9, 11
    (qry, base, bias, mu, wz), ref, _ = cases[(N, K, h, w)]
    taps = ops.rpmms_proto_taps(wz, mu)
    out = torch.full((3, 1, h, w, LD), SENTINEL, device=dev)
    ops.rpmms_bank_l56(qry[1:2], base[1:2], bias, mu[2:3].contiguous(), taps[2:3].contiguous(), out)
    assert torch.equal(out[:, 0, :, :, :C + 2], ref.view(3, N, K, h, w, LD)[:, 1, 2, :, :, :C + 2])


def test_wrapper_refusals(hip_lib, dev):
    from pemp_amd import ops
    qry, base, bias, mu, wz = _operands(2, 3, 3, 3, dev)
    taps = ops.rpmms_proto_taps(wz, mu)
    out = torch.zeros((3, 2, 3, 3, LD), device=dev)
    with pytest.raises(ValueError, match="index values"):
        ops.rpmms_bank_l56(qry, base, bias, mu, taps, out, index=[0, 3])
    with pytest.raises(ValueError, match="index has 1 entries"):
        ops.rpmms_bank_l56(qry, base, bias, mu, taps, out, index=[0])
    with pytest.raises(ValueError, match="CPU tensor"):
        ops.rpmms_bank_l56(qry, base, bias, mu, taps, out, index=torch.zeros(2, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="device index"):
        ops._rpmms_bank_l56(qry, base, bias, mu, taps, out, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="out must be fp32"):
        ops.rpmms_bank_l56(qry, base, bias, mu, taps, out)                         # all-classes needs N * K = 6 images
    with pytest.raises(ValueError, match="out must be fp32"):
        ops.rpmms_bank_l56(qry, base, bias, mu, taps, torch.zeros((3, 2, 3, 3, C), device=dev), index=[0, 1])
    with pytest.raises(ValueError, match="taps"):
        ops.rpmms_bank_l56(qry, base, bias, mu, taps[:2], out, index=[0, 1])
    with pytest.raises(ValueError, match="mu"):
        ops.rpmms_bank_l56(qry, base, bias, mu[:, :1], taps, out, index=[0, 1])
    with pytest.raises(ValueError, match="base"):
        ops.rpmms_bank_l56(qry, base[:1], bias, mu, taps, out, index=[0, 1])
    with pytest.raises(ValueError, match="wz"):
        ops.rpmms_proto_taps(wz[:8], mu)
