"""pemp_cosine_bank_max_f32 against pemp_cosine_proto_max_f32, HIP against HIP, bit for bit: for every query b and class k
the bank launch must write what the episode kernel writes for query b with protos = bank[k] -- prediction and response index.

Shapes: n = 169 (13 x 13: no multiple of 16 or 64, three blocks of 64 pixels), 16 and 1; c = 512 / 128 / 64 (the MFMA row
stream with 8 / 2 / 1 passes) and 12 (wave per pixel); p = 1, 3, 4 (two classes fill a 16-column tile exactly) and 5 (2p > 8:
wave per pixel at every c); K = 1, 2, 3, 5 (odd: a half-used tile; 5: three tiles) and 9 (more classes than one block keeps:
a second class group on grid.z); N = 1, 3.

The PEMP_HEAD_VALU leg is not here: both entries read that switch once per process, so it cannot be set per call."""
import pytest
import torch

from pemp_amd import ops

pytestmark = pytest.mark.gpu


def _rand(shape, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g).to(dev)


def _reference(q, bank, want_resp=True):
    """[N,K,2,h,w] / [N,K,h,w] from N * K launches of the episode kernel."""
    N, K = q.shape[0], bank.shape[0]
    pred = torch.empty((N, K, 2) + tuple(q.shape[1:3]), dtype=torch.float32, device=q.device)
    resp = torch.empty((N, K) + tuple(q.shape[1:3]), dtype=torch.uint8, device=q.device)
    for b in range(N):
        for k in range(K):
            pr, rs = ops.cosine_proto_max(q[b:b + 1], bank[k:k + 1].contiguous(), 20.0, want_resp=True)
            pred[b, k], resp[b, k] = pr[0], rs[0]
    return pred, resp


def _check(q, bank, what):
    ref_p, ref_r = _reference(q, bank)
    pred, resp = ops.cosine_bank_max(q, bank, 20.0, want_resp=True)
    assert pred.shape == ref_p.shape and resp.shape == ref_r.shape and resp.dtype == torch.uint8
    assert torch.equal(pred, ref_p), f"{what}: pred differs, max |d| {(pred - ref_p).abs().max().item():.3e}"
    assert torch.equal(resp, ref_r), f"{what}: resp differs at {(resp != ref_r).sum().item()} pixels"
    assert torch.equal(ops.cosine_bank_max(q, bank, 20.0), ref_p), f"{what}: pred without resp"
    return ref_p, ref_r


@pytest.mark.parametrize("c", [512, 128, 64, 12])
def test_every_query_against_every_class(hip_lib, dev, c):
    cases = [(13, p, K, N) for p in (1, 3, 4, 5) for K in (1, 2, 3, 5) for N in (1, 3)]
    cases += [(hw, p, 3, 3) for hw in (4, 1) for p in (1, 3, 4, 5)] + [(13, 3, 9, 2), (13, 4, 9, 1), (4, 5, 9, 1)]
    for s, (hw, p, K, N) in enumerate(cases):
        q = _rand((N, hw, hw, c), dev, 100 + s)
        bank = _rand((K, 2 * p, c), dev, 500 + s)
        _check(q, bank, f"c={c} n={hw * hw} p={p} K={K} N={N}")


@pytest.mark.parametrize("c,p", [(512, 3), (64, 4), (12, 3), (128, 5)])
def test_indexed_form_equals_slices_of_the_all_classes_form(hip_lib, dev, c, p):
    K, N = 5, 4
    q = _rand((N, 13, 13, c), dev, 7)
    bank = _rand((K, 2 * p, c), dev, 8)
    ref_p, ref_r = _check(q, bank, "all classes")
    index = [4, 0, 4, 2]                                     # repeated, out of order
    for idx in (index, torch.tensor(index), torch.tensor(index, dtype=torch.int32)):
        pred, resp = ops.cosine_bank_max(q, bank, 20.0, index=idx, want_resp=True)
        assert pred.shape == (N, 2, 13, 13) and resp.shape == (N, 13, 13)
        for b, k in enumerate(index):
            assert torch.equal(pred[b], ref_p[b, k]) and torch.equal(resp[b], ref_r[b, k]), (b, k)
    assert torch.equal(ops.cosine_bank_max(q, bank, 20.0, index=index), pred)
    # caller's buffers
    pb, rb = torch.full_like(pred, -1.0), torch.full_like(resp, 255)
    out = ops.cosine_bank_max(q, bank, 20.0, index=index, want_resp=True, pred=pb, resp=rb)
    assert out[0] is pb and out[1] is rb and torch.equal(pb, pred) and torch.equal(rb, resp)
    with pytest.raises(ValueError, match="index values"):
        ops.cosine_bank_max(q, bank, 20.0, index=[0, 1, 2, 5])
    with pytest.raises(ValueError, match="CPU tensor"):
        ops.cosine_bank_max(q, bank, 20.0, index=torch.tensor(index, device=dev))


@pytest.mark.parametrize("c", [512, 12])
def test_strided_feature_view(hip_lib, dev, c):
    """ldf > c: the features are the leading channels of a wider NHWC tensor."""
    big = _rand((3, 13, 13, c + 16), dev, 21)
    q = big[..., :c]
    assert not q.is_contiguous()
    bank = _rand((3, 6, c), dev, 22)
    ref_p, ref_r = _check(q, bank, f"ldf = {c + 16}")
    dense_p, dense_r = ops.cosine_bank_max(q.contiguous(), bank, 20.0, want_resp=True)
    assert torch.equal(dense_p, ref_p) and torch.equal(dense_r, ref_r)


@pytest.mark.parametrize("c,p", [(512, 3), (128, 4), (12, 3), (64, 5)])
def test_degenerate_bank_rows(hip_lib, dev, c, p):
    """An all-zero row (the prototype of an empty mask: the 1e-8 norm clamp) beside ordinary ones, a whole class of zeros,
    and two identical prototypes inside one class (the response tie: the first maximum wins)."""
    q = _rand((2, 13, 13, c), dev, 31)
    bank = _rand((4, 2 * p, c), dev, 32)
    bank[0, 0] = 0.0                                  # fg row 0 of class 0
    bank[1, 2 * p - 1] = 0.0                          # last bg row of class 1
    bank[2] = 0.0                                     # class 2: nothing but zeros
    if p > 1:
        bank[3, 1] = bank[3, 0]                       # fg tie
        bank[3, p + 1] = bank[3, p]                   # bg tie
    q[1, 0, 0] = 0.0                                  # and a zero query pixel (the query-norm clamp)
    ref_p, ref_r = _check(q, bank, "degenerate rows")
    assert torch.isfinite(ref_p).all()
    assert (ref_p[:, 2] == 0).all() and (ref_r[:, 2] == 0).all()          # zeros against anything: cosine 0, bg row 0 answers
    if p > 1:           # never the second of two equal prototypes: bg index 1 answers as 1, fg index 1 as 1 + 3 (bg indices stop at 3 for p <= 4)
        assert not (ref_r[:, 3] == 1).any() and (p > 4 or not (ref_r[:, 3] == 4).any())
