"""Layout of the split3 weight pack (pemp_pack_split3_bf16, include/pemp_hip.h), restated on the CPU: [Cout][Kpad] fp32 ->
[Cout][Kpad / 32][3][32] bf16, per row and 32-channel K step the planes h, m, l of x = h + m + l (round to nearest even at each
stage).  tests/test_conv_split3_gpu.py holds the device pack to this function bit for bit."""
import torch


def split3_reference(w):
    """CPU split of a [Cout, Kpad] fp32 weight into the pack's [Cout, Kpad / 32, 3, 32] bf16 layout."""
    co, kpad = w.shape
    h = w.to(torch.bfloat16)
    r = w - h.float()                       # exact in fp32
    m = r.to(torch.bfloat16)
    l = (r - m.float()).to(torch.bfloat16)
    return torch.stack([p.view(co, kpad // 32, 32) for p in (h, m, l)], dim=2).contiguous()


def _cases():
    g = torch.Generator().manual_seed(3)
    yield torch.randn(64, 96, generator=g)
    yield torch.randn(64, 96, generator=g) * 1e-20               # tiny (the split is exact while l stays an fp32 normal: |x| >= ~2^-110)
    yield torch.randn(64, 96, generator=g) * 1e30                # large
    yield -torch.rand(64, 96, generator=g) - 1.0                 # negative
    yield torch.zeros(64, 96)
    yield torch.tensor([[1.0 + 2.0 ** -23, -(1.0 + 2.0 ** -9 + 2.0 ** -17), 3.0, 2.0 ** -126] * 8] * 64)


def test_split3_pieces_add_up_exactly_and_shrink():
    for w in _cases():
        s = split3_reference(w)
        h, m, l = (s[:, :, i].reshape(w.shape).double() for i in range(3))
        assert torch.equal(h + m + l, w.double())
        assert bool((m.abs() <= w.double().abs() * 2.0 ** -8).all())
        assert bool((l.abs() <= w.double().abs() * 2.0 ** -16).all())


def test_split3_layout_keeps_the_channel_order_per_k_step():
    co, kpad = 4, 64
    w = torch.arange(co * kpad, dtype=torch.float32).view(co, kpad)     # small integers: h carries them, m = l = 0 where exact
    s = split3_reference(w)
    assert s.shape == (co, kpad // 32, 3, 32) and s.dtype == torch.bfloat16
    for n in range(co):
        for k in range(kpad):
            pieces = s[n, k // 32, :, k % 32].double()
            assert pieces.sum().item() == w[n, k].item()
            assert pieces[0].item() == float(torch.tensor(w[n, k].item()).to(torch.bfloat16))
    # byte offsets the kernel uses: row n, K step j, plane p, channel c -> ((n * Kpad / 32 + j) * 3 + p) * 32 + c elements
    flat = s.view(-1)
    n, j, p, c = 3, 1, 0, 17
    assert flat[((n * (kpad // 32) + j) * 3 + p) * 32 + c].item() == s[n, j, p, c].item()
