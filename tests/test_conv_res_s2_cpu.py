"""The strided-residual variants (PEMP_CONV_RES_S2: conv_panel_rs2_kernel, conv_dma2_rs2_kernel) without a GPU, from the metadata of
the built gfx950 code objects -- no disassembly is read:

 * the register rule: a new instantiation has no scratch and no spilled VGPR, and its waves per SIMD are no lower than those of the
   dense-residual instantiation it derives from;
 * the instantiations are the intended ones and no other (71 at K = 128 is NOT one: like its dense form it would count 16 spilled
   VGPRs, so the id refuses the flag there);
 * every kernel conv_panel.hip and conv_dma2.hip had before keeps its VGPR / AGPR / scratch / static-LDS figures
   (tests/golden/conv_res_s2_kernel_figures.json, recorded before the variants were added);
 * the header, the Python constants and the entry's refusals that need no device."""
import ctypes as C
import json
import os

import pytest

from tests import test_conv_split3_panel_cpu as P
from tests import test_conv_split3_persist_cpu as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_res_s2_kernel_figures.json")
needs_llvm = pytest.mark.skipif(not os.path.exists(f"{P.LLVM}/clang-offload-bundler"), reason="needs the ROCm LLVM tools")

PANEL_RS2 = "_ZN4pemp21conv_panel_rs2_kernelILi{nk}ELi{bn}ELi4EEEvNS_8ConvArgsE"
PANEL_DENSE = "_ZN4pemp17conv_panel_kernelILi{nk}ELi{bn}ELi4EEEvNS_8ConvArgsE"
PANEL_INSTS = ((2, 64), (4, 64), (2, 128))               # (K steps, BN): K = 64 and 128 on id 72, K = 64 on id 71
DMA2_RS2 = "_ZN4pemp20conv_dma2_rs2_kernelILi64ELi64ELi2ELi4EEEvNS_8ConvArgsE"
DMA2_DENSE = "_ZN4pemp16conv_dma2_kernelILi64ELi64ELi2ELi4ELb0ELi0ELb0ELb0ELb0ELb0ELb1EEEvNS_8ConvArgsE"


def _clean(meta):
    assert int(meta["private_segment_fixed_size"]) == 0 and int(meta["vgpr_spill_count"]) == 0, meta
    assert int(meta.get("sgpr_spill_count", 0)) == 0, meta


def _waves_by_registers(meta):
    regs = (int(meta["vgpr_count"]) + 7) // 8 * 8         # the unified file's total (the AGPRs are part of it), granule 8
    assert int(meta["agpr_count"]) <= regs <= 512
    return min(8, 512 // regs)


@needs_llvm
def test_the_panel_variants_hold_the_register_rule():
    ks = P._kernels()
    built = sorted(k for k in ks if "conv_panel_rs2_kernel" in k)
    assert built == sorted(PANEL_RS2.format(nk=nk, bn=bn) for nk, bn in PANEL_INSTS), built
    for nk, bn in PANEL_INSTS:
        new, dense = ks[PANEL_RS2.format(nk=nk, bn=bn)], ks[PANEL_DENSE.format(nk=nk, bn=bn)]
        _clean(new)
        assert P._waves(new, bn) >= P._waves(dense, bn) == P.INTENDED[(nk, bn)], (nk, bn, new, dense)
        assert int(new["vgpr_count"]) <= int(dense["vgpr_count"]), (nk, bn, new, dense)


@needs_llvm
def test_the_64_x_64_variant_holds_the_register_rule():
    ks = S._kernels()
    assert [k for k in ks if "conv_dma2_rs2_kernel" in k] == [DMA2_RS2]
    new, dense = ks[DMA2_RS2], ks[DMA2_DENSE]
    _clean(new)
    assert _waves_by_registers(new) >= _waves_by_registers(dense) >= 4, (new, dense)      # its LDS holds the shape to 4


@needs_llvm
def test_the_kernels_from_before_keep_their_figures():
    with open(GOLDEN) as f:
        want = json.load(f)
    for unit, kernels in (("conv_panel", P._kernels()), ("conv_dma2", S._kernels())):
        assert len(want[unit]) > 0 and set(want[unit]) <= set(kernels), (unit, sorted(set(want[unit]) - set(kernels)))
        assert all("rs2" in k for k in set(kernels) - set(want[unit])), sorted(set(kernels) - set(want[unit]))
        for name, figures in want[unit].items():
            m = kernels[name]
            got = [int(m["vgpr_count"]), int(m["agpr_count"]), int(m["private_segment_fixed_size"]), int(m["group_segment_fixed_size"])]
            assert got == figures, (name, got, figures)
    assert want["conv_panel"][PANEL_DENSE.format(nk=8, bn=128)][0] == 506          # the one that sits at 506 of 512


def test_header_and_constants():
    from pemp_amd import _lib
    with open(os.path.join(ROOT, "include", "pemp_hip.h")) as f:
        text = f.read()
    assert "#define PEMP_ABI_VERSION 2 " in text
    for name, value in (("PEMP_CONV_RES_S2", 128), ("PEMP_CONV_RES_HEVEN", 512), ("PEMP_CONV_RES_WEVEN", 1024)):
        assert f"#define {name} {value}u" in text
        assert getattr(_lib, name[5:]) == value
    with open(os.path.join(ROOT, "pemp_amd", "csrc", "conv_common.h")) as f:
        assert "#define PEMP_CONV_BF16_IO 0x100u" in f.read()                      # the bit between them is the library's own
    assert C.sizeof(_lib.ConvDesc) == 18 * 4
    assert "conv_panel_rs2_kernel" in text and "conv_dma2_rs2_kernel" in text


def test_the_entries_refuse_the_flag_before_a_device_is_touched(hip_lib):
    """Refusals that are decided on the descriptor alone: the pointers are never read."""
    from pemp_amd import _lib
    x, w, y, r, ws = (C.c_void_p(v) for v in (0x10000, 0x4000000, 0x8000000, 0xC000000, 0x10000000))
    S2 = _lib.CONV_RES_S2

    def desc(tile, flags, kpad=64):
        return _lib.ConvDesc(3, 7, 7, kpad, kpad, 7, 7, 256, 256, 1, 1, 1, 0, 1, 256, kpad, flags, tile)

    def conv(tile, flags, kpad=64, residual=r):
        return hip_lib.pemp_conv2d_nhwc_f32(C.byref(desc(tile, flags, kpad)), x, w, y, None, None, residual, None)

    got = {"47": conv(47, S2), "49": conv(49, S2), "41": conv(41, S2), "42": conv(42, S2), "44": conv(44, S2), "46": conv(46, S2),
           "fp32 chain": conv(23, S2), "the entry's own choice": conv(0, S2), "71 at K = 128": conv(71, S2, 128),
           "72 at K = 96": conv(72, S2, 96), "no residual": conv(43, S2, residual=None),
           "a pre-split output": conv(43, S2 | _lib.CONV_OUT_SPLIT3), "a pre-split input": conv(146, S2 | _lib.CONV_IN_SPLIT3),
           "the second output": conv(146, S2 | _lib.CONV_IN_SPLIT3 | _lib.CONV_OUT_SPLIT3_ALSO),
           "a parity bit alone": conv(43, _lib.CONV_RES_WEVEN),
           "split-K": hip_lib.pemp_conv2d_splitk_nhwc_f32(C.byref(desc(51, S2)), x, w, y, None, None, r, ws, 1 << 24, None),
           "a workspace": hip_lib.pemp_conv2d_splitk_nhwc_f32(C.byref(desc(43, S2)), x, w, y, None, None, r, ws, 1 << 24, None),
           "DropBlock": hip_lib.pemp_conv2d_dropblock_nhwc_f32(C.byref(desc(23, S2)), x, w, y, None, None, r, ws, ws, None, 0, None)}
    d3 = _lib.ConvDesc(3, 7, 7, 64, 64, 7, 7, 256, 256, 3, 3, 1, 1, 1, 256, 576, S2, 43)        # 3x3: a padding value is admissible
    got["a padding value"] = hip_lib.pemp_conv2d_padv_nhwc_f32(C.byref(d3), x, w, y, None, None, r, ws, None)
    d1 = desc(43, S2)
    ptrs = lambda v: (C.c_void_p * 1)(v)
    got["grouped"] = hip_lib.pemp_conv2d_group_nhwc_f32(1, C.byref(d1), ptrs(x), ptrs(w), ptrs(y), None, None, ptrs(r), None, None)
    got["statistics"] = hip_lib.pemp_split3_conv2d_stats_nhwc_f32(C.byref(d1), x, w, y, ws, None)
    got["bf16"] = hip_lib.pemp_conv2d_bf16_nhwc(C.byref(d1), x, w, y, None, None, r, None, 0, None)
    assert all(rc != 0 for rc in got.values()), got
