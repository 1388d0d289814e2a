"""Pre-split activations (PEMP_CONV_OUT_SPLIT3 / PEMP_CONV_IN_SPLIT3, tile ids 146 / 149; include/pemp_hip.h), on the CPU:

 * a model of the layout -- fp32 [N, H, W, C] <-> bf16 [N, H, W, C / 32, 3, 32], per pixel and 32-channel group the planes h, m, l of
   the reference split the weight pack's tests use (tests/test_conv_split3_cpu.py) -- whose pieces add up to the value bit for bit;
   tests/test_conv_split3_presplit_gpu.py holds the kernels to it;
 * the code object: the two instantiations exist, use no scratch and keep two waves per SIMD (registers and LDS);
 * what ops.conv2d and the library refuse."""
import ctypes as C
import os

import pytest
import torch

from tests.test_conv_split3_cpu import _cases as _split_cases, split3_reference
from tests.test_conv_split3_persist_cpu import LLVM, _kernels


def presplit(x):
    """fp32 [N, H, W, C] (C % 32 == 0) -> its pre-split form, bf16 [N, H, W, C / 32, 3, 32]: split3_reference's arithmetic (round to
    nearest even at each stage, the differences in fp32).  Works on any device."""
    n, h, w, c = x.shape
    hi = x.to(torch.bfloat16)
    r = x - hi.float()
    mid = r.to(torch.bfloat16)
    lo = (r - mid.float()).to(torch.bfloat16)
    return torch.stack([p.reshape(n, h, w, c // 32, 32) for p in (hi, mid, lo)], dim=4).contiguous()


def unsplit(s):
    """The fp32 tensor [N, H, W, C] whose pre-split form is ``s`` (h + m + l is an fp32 value: the float64 sum is exact)."""
    n, h, w, g = s.shape[:4]
    return s.double().sum(dim=4).float().reshape(n, h, w, g * 32)


def _hard_rows():
    """[rows, 96] fp32: the hard values of the weight split's tests (1 + 2^-23, -(1 + 2^-9 + 2^-17), 2^-126, negatives, 1e-20 and
    1e30 scales, zeros) plus values next to the denormal range."""
    rows = [w if w.shape[1] == 96 else w.repeat(1, 96 // w.shape[1]) for w in _split_cases()]
    g = torch.Generator().manual_seed(11)
    # |x| in [2^-101, 2^-99): l lands next to the fp32 denormals and is still exact (the split is, down to |x| ~ 2^-110)
    rows.append((torch.rand(64, 96, generator=g) + 0.5) * (1 - 2 * torch.randint(0, 2, (64, 96), generator=g)) * 2.0 ** -100)
    rows.append(torch.tensor([[2.0 ** -126, -2.0 ** -126, 2.0 ** -125 + 2.0 ** -126, -(2.0 ** -120)] * 24] * 8))
    return torch.cat(rows)


def test_layout_model_packs_and_unpacks_bit_for_bit():
    x = _hard_rows()
    m = x.shape[0] // 4 * 4
    x = x[:m].reshape(1, 4, m // 4, 96).contiguous()
    s = presplit(x)
    assert s.shape == (1, 4, m // 4, 3, 3, 32) and s.dtype == torch.bfloat16 and s.is_contiguous()
    assert torch.equal(unsplit(s).view(torch.int32), x.view(torch.int32))             # bit for bit (signs of zero included)
    # in the kernels' order of addition, in fp32: (l + m) + h
    p = s.float()
    assert torch.equal(((p[..., 2, :] + p[..., 1, :]) + p[..., 0, :]).reshape(x.shape), x)
    # the same pieces as the weight pack's reference, pixel rows in place of weight rows
    want = split3_reference(x.reshape(m, 96))
    assert torch.equal(s.reshape(m, 3, 3, 32).view(torch.int16), want.view(torch.int16))
    # element (pixel, channel c, plane p) sits at ((pixel * C / 32 + c / 32) * 3 + p) * 32 + c % 32
    flat, pix, c, pl = s.reshape(-1), 7, 70, 1
    assert flat[((pix * 3 + c // 32) * 3 + pl) * 32 + c % 32].item() == s.reshape(m, 3, 3, 32)[pix, c // 32, pl, c % 32].item()


BM, BN, WGM, NW = 256, 128, 4, 8          # 4 x 2 waves of 64 x 64
KERNELS = {146: "_ZN4pemp19conv_dma2_a3_kernelILi{bm}ELi{bn}ELi{wgm}ELi{nw}ELb{padv}EEEvNS_8ConvArgsE",
           149: "_ZN4pemp20conv_dma2_a3p_kernelILi{bm}ELi{bn}ELi{wgm}ELi{nw}ELb{padv}EEEvNS_8ConvArgsE"}


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/clang-offload-bundler"), reason="needs the ROCm LLVM tools")
@pytest.mark.parametrize("tile", sorted(KERNELS))
def test_presplit_kernels_use_no_scratch_and_keep_two_waves_per_simd(tile):
    ks = _kernels()
    for padv in (0, 1):
        meta = ks[KERNELS[tile].format(bm=BM, bn=BN, wgm=WGM, nw=NW, padv=padv)]
        assert int(meta["private_segment_fixed_size"]) == 0 and int(meta["vgpr_spill_count"]) == 0, (tile, padv, meta)
        regs = (int(meta["vgpr_count"]) + 3) // 4 * 4 + int(meta["agpr_count"])
        assert 512 // regs >= 2, (tile, padv, meta)                              # two waves per SIMD by registers
        lds = 2 * 12 * (BM + BN) * 16                                              # A and B rows of 12 quads, two stages
        assert lds == 144 * 1024 and (160 * 1024 // lds) * NW // 4 >= 2           # ... and by LDS: one 8-wave block per CU
    # the 128 x 128 shape would drop from two blocks per CU to one: no id
    assert 160 * 1024 // (2 * (8 * 128 + 12 * 128) * 16) == 2 and 160 * 1024 // (2 * 12 * (128 + 128) * 16) == 1


def test_registry_names_the_new_ids(hip_lib):
    from pemp_amd import ops
    assert ops.SPLIT3_PRESPLIT_TILES == (146, 149)
    bm, bn = C.c_int(-1), C.c_int(-1)
    for t in ops.SPLIT3_PRESPLIT_TILES:
        assert ops.tile_shape(t) == (256, 128) == ops.tile_shape(46)
        assert hip_lib.pemp_conv2d_tile_shape(t, C.byref(bm), C.byref(bn)) == 1 and (bm.value, bn.value) == (256, 128)
        assert t not in ops.SPLIT3_TILES and t not in ops.SPLIT3_PANEL_TILES and t not in ops.TILE_VARIANTS
    for t in list(range(100, 146)) + [147, 148] + list(range(150, 200)):
        assert ops.tile_shape(t) is None and hip_lib.pemp_conv2d_tile_shape(t, None, None) == 0, t


def _layer(ops, cin, cout, k, split=True, stem=False):
    w = torch.zeros(cout, k * k * cin)
    w3 = torch.zeros(cout, k * k * cin // 32, 3, 32, dtype=torch.bfloat16) if split else None
    return ops.ConvParams(w, None, None, cin, cout, k, k, 1, k // 2, 1, k * k * cin, stem, False, w3)


def test_ops_refuses_what_the_forms_do_not_take():
    """Every refusal is raised before a device is touched: the tensors here live on the CPU."""
    from pemp_amd import ops
    x = torch.zeros(1, 5, 5, 64)
    xs = presplit(x)
    out_s = torch.zeros(ops.split3_shape(1, 5, 5, 128), dtype=torch.bfloat16)
    p1, p3 = _layer(ops, 64, 128, 1), _layer(ops, 64, 128, 3)
    bad_out = [
        dict(p=_layer(ops, 64, 128, 1, split=False)),                    # an fp32-chain layer
        dict(residual=torch.zeros(1, 5, 5, 128)),
        dict(splitk=True),
        dict(dropblock=(torch.zeros(1, 5, 5), torch.zeros(1, dtype=torch.int32))),
        dict(tile=51), dict(tile=71), dict(tile=23),                     # split-K, panel and fp32-chain ids
        dict(out=torch.zeros(1, 5, 5, 128)),                             # not the pre-split shape / dtype
        dict(out=torch.zeros(ops.split3_shape(1, 5, 5, 256), dtype=torch.bfloat16)[..., :4, :, :]),      # a channel window
    ]
    for kw in bad_out:
        kw = dict(dict(p=p1, out=out_s), **kw)
        with pytest.raises(ValueError):
            ops.conv2d(x, kw.pop("p"), out_split3=True, **kw)
    bad_in = [
        dict(p=p1),                                                      # a 1x1 conv
        dict(p=_layer(ops, 64, 128, 3, split=False)),
        dict(p=_layer(ops, 64, 64, 3)),                                  # Cout % 128
        dict(splitk=True),
        dict(per_image_shift=True, shift_override=torch.zeros(1, 128)),
        dict(dropblock=(torch.zeros(1, 5, 5), torch.zeros(1, dtype=torch.int32))),
        dict(tile=46), dict(tile=49), dict(tile=56),                     # ids of the fp32-input forms
        dict(x=x),                                                       # an fp32 tensor
        dict(x=presplit(torch.zeros(1, 5, 5, 96))),                      # another channel count
    ]
    for kw in bad_in:
        kw = dict(dict(p=p3, x=xs), **kw)
        with pytest.raises(ValueError):
            ops.conv2d(kw.pop("x"), kw.pop("p"), x_split3=True, **kw)
    for tile in ops.SPLIT3_PRESPLIT_TILES:                               # the new ids without a pre-split input
        with pytest.raises(ValueError):
            ops.conv2d(x, p3, tile=tile)


def _desc(ConvDesc, cin, cout, k, flags, tile, ldy=None, ldx=None, n=1, h=5, w=5):
    return ConvDesc(n, h, w, cin, ldx or cin, h, w, cout, ldy or cout, k, k, 1, k // 2, 1, cout, k * k * cin, flags, tile)


def test_library_refuses_what_the_forms_do_not_take(hip_lib):
    """The entry points return -1 before anything is launched (the pointers are never dereferenced)."""
    from pemp_amd._lib import ConvDesc, CONV_OUT_SPLIT3 as OUT, CONV_IN_SPLIT3 as IN, CONV_SHIFT_PER_IMAGE as PER_IMG
    p = C.c_void_p(0x10000)

    def conv(d, residual=None):
        return hip_lib.pemp_conv2d_nhwc_f32(C.byref(d), p, p, p, None, None, residual, None)

    # producer: fp32-chain ids, split-K ids, the panel ids, a residual, a channel window
    for tile in (0, 3, 13, 23, 29, 33, 51, 56, 71, 72):
        assert conv(_desc(ConvDesc, 64, 128, 1, OUT, tile)) == -1, tile
    assert conv(_desc(ConvDesc, 64, 128, 1, OUT, 43), residual=p) == -1
    assert conv(_desc(ConvDesc, 64, 128, 1, OUT, 43, ldy=256)) == -1
    assert b"SPLIT3" in hip_lib.pemp_last_error()
    # ... with a workspace (the split-K entry), grouped, DropBlock, statistics
    d = _desc(ConvDesc, 64, 128, 1, OUT, 43)
    assert hip_lib.pemp_conv2d_splitk_nhwc_f32(C.byref(d), p, p, p, None, None, None, p, 1 << 20, None) == -1
    arr = (C.c_void_p * 1)(p)
    assert hip_lib.pemp_conv2d_group_nhwc_f32(1, C.byref(d), arr, arr, arr, None, None, None, None, None) == -1
    d23 = _desc(ConvDesc, 64, 128, 1, OUT, 23)
    assert hip_lib.pemp_conv2d_dropblock_nhwc_f32(C.byref(d23), p, p, p, None, None, None, p, p, None, 0, None) == -1
    assert hip_lib.pemp_conv2d_stats_nhwc_f32(C.byref(d23), p, p, p, p, None, 0, None) == -1
    # consumer: the flag and the ids come together; 1x1, per-image shift, a workspace, a channel window, Cout % 128, grouped
    for tile in (0, 43, 46, 49, 56, 23):
        assert conv(_desc(ConvDesc, 64, 128, 3, IN, tile)) == -1, tile
    for tile in (146, 149):
        assert conv(_desc(ConvDesc, 64, 128, 3, 0, tile)) == -1, tile
        assert conv(_desc(ConvDesc, 64, 128, 1, IN, tile)) == -1, tile
        assert conv(_desc(ConvDesc, 64, 128, 3, IN | PER_IMG, tile)) == -1, tile
        assert conv(_desc(ConvDesc, 64, 128, 3, IN, tile, ldx=128)) == -1, tile
        assert conv(_desc(ConvDesc, 48, 128, 3, IN, tile)) == -1, tile
        assert conv(_desc(ConvDesc, 64, 64, 3, IN, tile)) == -1, tile
        assert conv(_desc(ConvDesc, 64, 128, 5, IN, tile)) == -1, tile              # 25 taps: the tap masks hold 16
        d = _desc(ConvDesc, 64, 128, 3, IN, tile)
        assert hip_lib.pemp_conv2d_splitk_nhwc_f32(C.byref(d), p, p, p, None, None, None, p, 1 << 20, None) == -1, tile
        assert hip_lib.pemp_conv2d_group_nhwc_f32(1, C.byref(d), arr, arr, arr, None, None, None, None, None) == -1, tile
