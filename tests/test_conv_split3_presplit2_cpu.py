"""The kernels that STORE pre-split from a persistent tile loop, and the second, pre-split output (PEMP_CONV_OUT_SPLIT3 on ids 47 / 49 /
149; PEMP_CONV_OUT_SPLIT3_ALSO on ids 146 / 149; include/pemp_hip.h), on the CPU:

 * the code object: every instantiation the header names exists for both padding forms, uses no scratch, spills no vector register
   and stays within 256 registers (two waves per SIMD; the 64 x 64 shape within 128: its four);
 * what ops.conv2d and the library refuse for the second output."""
import ctypes as C
import os
import re

import pytest
import torch

from tests.test_conv_split3_persist_cpu import LLVM, _kernels
from tests.test_conv_split3_presplit_cpu import _desc, _layer, presplit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#: kernel template -> (mangled name, its instantiations as (BM, BN, WGM, NW, OUT or None), registers per wave it may use)
NEW = {
    "conv_dma2_s3po_kernel": ("_ZN4pemp21conv_dma2_s3po_kernelILi{bm}ELi{bn}ELi{wgm}ELi{nw}ELb{padv}ELi{out}EEEvNS_8ConvArgsE",
                              [(256, 128, 8, 8, 1), (64, 64, 2, 4, 1)]),
    "conv_dma2_a3po_kernel": ("_ZN4pemp21conv_dma2_a3po_kernelILi{bm}ELi{bn}ELi{wgm}ELi{nw}ELb{padv}ELi{out}EEEvNS_8ConvArgsE",
                              [(256, 128, 4, 8, 1), (256, 128, 4, 8, 2)]),
    "conv_dma2_a3o_kernel": ("_ZN4pemp20conv_dma2_a3o_kernelILi{bm}ELi{bn}ELi{wgm}ELi{nw}ELb{padv}EEEvNS_8ConvArgsE",
                             [(256, 128, 4, 8, None)]),
}
CASES = [(k, inst) for k, (_, insts) in sorted(NEW.items()) for inst in insts]


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/clang-offload-bundler"), reason="needs the ROCm LLVM tools")
@pytest.mark.parametrize("kernel,inst", CASES, ids=[f"{k}-{'x'.join(map(str, i))}" for k, i in CASES])
def test_new_instantiations_use_no_scratch_and_keep_their_waves(kernel, inst):
    ks = _kernels()
    bm, bn, wgm, nw, out = inst
    for padv in (0, 1):
        meta = ks[NEW[kernel][0].format(bm=bm, bn=bn, wgm=wgm, nw=nw, padv=padv, out=out)]
        assert int(meta["private_segment_fixed_size"]) == 0 and int(meta["vgpr_spill_count"]) == 0, (kernel, inst, padv, meta)
        regs = (int(meta["vgpr_count"]) + 3) // 4 * 4 + int(meta["agpr_count"])
        assert regs <= 256, (kernel, inst, padv, meta)                      # two waves per SIMD
        if bm == 64:
            assert regs <= 128, (kernel, inst, padv, meta)                  # ... four for the 64 x 64 shape, as its LDS allows


def test_header_names_the_instantiations():
    with open(os.path.join(ROOT, "include", "pemp_hip.h")) as f:
        text = f.read()
    named = set(re.findall(r"conv_dma2_\w*o_kernel", text))
    assert named == set(NEW), named
    assert "PEMP_CONV_OUT_SPLIT3_ALSO 64u" in text
    ks = _kernels() if os.path.exists(f"{LLVM}/clang-offload-bundler") else None
    if ks is not None:
        built = {re.match(r"_ZN4pemp\d+(conv_dma2_\w*o_kernel)I", k).group(1) for k in ks if re.match(r"_ZN4pemp\d+conv_dma2_\w*o_kernelI", k)}
        assert built == set(NEW), built
        # ... and nothing beside the instantiations listed above
        want = {NEW[k][0].format(bm=i[0], bn=i[1], wgm=i[2], nw=i[3], padv=p, out=i[4]) for k, i in CASES for p in (0, 1)}
        assert {k for k in ks if re.match(r"_ZN4pemp\d+conv_dma2_\w*o_kernelI", k)} == want


def test_ops_refuses_what_the_second_output_does_not_take():
    """Every refusal is raised before a device is touched: the tensors here live on the CPU."""
    from pemp_amd import ops
    x = torch.zeros(1, 5, 5, 64)
    xs = presplit(x)
    p3 = _layer(ops, 64, 128, 3)
    also = torch.zeros(ops.split3_shape(1, 5, 5, 128), dtype=torch.bfloat16)
    bad = [
        dict(x=x, x_split3=False),                                       # an fp32 input: not the ids 146 / 149
        dict(residual=torch.zeros(1, 5, 5, 128)),
        dict(out_split3=True),
        dict(splitk=True),
        dict(dropblock=(torch.zeros(1, 5, 5), torch.zeros(1, dtype=torch.int32))),
        dict(tile=46), dict(tile=49), dict(tile=71),
        dict(also_split3=torch.zeros(1, 5, 5, 128)),                     # not the pre-split shape / dtype
        dict(also_split3=torch.zeros(ops.split3_shape(1, 5, 5, 256), dtype=torch.bfloat16)),
        dict(also_split3=torch.zeros(ops.split3_shape(1, 5, 5, 256), dtype=torch.bfloat16)[..., :4, :, :]),      # a channel window
    ]
    for kw in bad:
        kw = dict(dict(x=xs, x_split3=True, also_split3=also), **kw)
        with pytest.raises(ValueError):
            ops.conv2d(kw.pop("x"), p3, **kw)


def library_refusals(hip_lib):
    """[(what, return code)] of the calls with PEMP_CONV_OUT_SPLIT3_ALSO that the entries must refuse (nothing is launched and no
    pointer dereferenced), preceded by nothing that succeeds; shared with the GPU test."""
    from pemp_amd._lib import ConvDesc, CONV_OUT_SPLIT3 as OUT, CONV_IN_SPLIT3 as IN, CONV_STEM4 as STEM, CONV_OUT_SPLIT3_ALSO as ALSO
    y, s = C.c_void_p(0x10000), C.c_void_p(0x4000000)                  # 64 MiB apart: the two outputs of these shapes do not overlap
    p = C.c_void_p(0x8000000)

    def conv(d, second=s, out=y):
        return hip_lib.pemp_conv2d_nhwc_f32(C.byref(d), p, p, out, None, None, second, None)

    got = []
    for tile in (0, 3, 23, 43, 46, 47, 49, 51, 56, 71, 72):              # every id but 146 / 149 (with or without a pre-split input)
        got.append((f"tile {tile}", conv(_desc(ConvDesc, 64, 128, 3, ALSO, tile))))
        got.append((f"tile {tile} + IN", conv(_desc(ConvDesc, 64, 128, 3, ALSO | IN, tile))))
    got.append(("1x1 on a panel id", conv(_desc(ConvDesc, 64, 128, 1, ALSO, 71))))
    arr = (C.c_void_p * 1)(p)
    for tile in (146, 149):
        d = _desc(ConvDesc, 64, 128, 3, ALSO | IN, tile)
        got.append((f"{tile}: no second tensor", conv(d, second=None)))
        got.append((f"{tile}: with OUT_SPLIT3", conv(_desc(ConvDesc, 64, 128, 3, ALSO | IN | OUT, tile))))
        got.append((f"{tile}: stem", conv(_desc(ConvDesc, 64, 128, 3, ALSO | IN | STEM, tile))))
        got.append((f"{tile}: without IN_SPLIT3", conv(_desc(ConvDesc, 64, 128, 3, ALSO, tile))))
        got.append((f"{tile}: misaligned", conv(d, second=C.c_void_p(0x4000008))))
        got.append((f"{tile}: second == y", conv(d, second=y)))
        got.append((f"{tile}: second inside y", conv(d, second=C.c_void_p(0x10000 + 1024))))
        got.append((f"{tile}: y inside second", conv(d, second=C.c_void_p(0x10000 - 1024))))
        got.append((f"{tile}: split-K / workspace", hip_lib.pemp_conv2d_splitk_nhwc_f32(C.byref(d), p, p, y, None, None, s, p, 1 << 20, None)))
        got.append((f"{tile}: grouped", hip_lib.pemp_conv2d_group_nhwc_f32(1, C.byref(d), arr, arr, arr, None, None, arr, None, None)))
    d23 = _desc(ConvDesc, 64, 128, 1, ALSO, 23)
    got.append(("dropblock", hip_lib.pemp_conv2d_dropblock_nhwc_f32(C.byref(d23), p, p, y, None, None, s, p, p, None, 0, None)))
    got.append(("statistics", hip_lib.pemp_conv2d_stats_nhwc_f32(C.byref(d23), p, p, y, p, None, 0, None)))
    return got


def test_library_refuses_what_the_second_output_does_not_take(hip_lib):
    for what, rc in library_refusals(hip_lib):
        assert rc == -1, what
