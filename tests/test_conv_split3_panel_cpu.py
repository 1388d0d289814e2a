"""The activation-stationary split3 kernels (conv_panel.hip, tile ids 71 / 72) without a GPU: every instantiation's register
budget from the built gfx950 code object (no scratch; the intended waves per SIMD, counting registers and LDS), and the ids'
place in the registries: none of the four old ones, a registry of their own, and ids 0..64 answer every query as before."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

from tests import test_conv_tiles_cpu as T

LLVM = "/opt/rocm/llvm/bin"
NW = 4
# (K steps, BN) -> intended waves per SIMD: one block of four waves per CU, two where K <= 128 runs 64 columns at a time
INTENDED = {(nk, bn): (2 if bn == 64 and nk <= 4 else 1) for nk in range(1, 9) for bn in (64, 128)}


def _kernels():
    from pemp_amd import build
    build.build()
    obj = os.path.join(build.OBJ, "conv_panel.o")
    tmp = os.path.join(build.OBJ, "conv_panel.gfx950")
    fb, co = tmp + ".fatbin", tmp + ".elf"
    subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", obj, os.devnull], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fb}", f"--output={co}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], check=True)
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    out, cur = {}, {}
    for line in notes.splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s+(\S+)", line)
        if not m:
            continue
        key, val = m.groups()
        if key == "agpr_count" and line.lstrip().startswith("-"):
            cur = {}
        cur[key] = val
        if key == "name":
            out[val] = cur
    return out


def _waves(meta, bn):
    regs = (int(meta["vgpr_count"]) + 7) // 8 * 8      # the unified file's total: the AGPRs are part of it, granule 8
    assert int(meta["agpr_count"]) <= regs <= 512
    by_regs = min(8, 512 // regs)
    lds = (3 * bn * 12 + NW * 256) * 16            # three weight stages + one transpose patch per wave
    assert int(meta["group_segment_fixed_size"]) == 0          # all of it is dynamic: the launch passes `lds`
    return min(by_regs, (160 * 1024 // lds) * NW // 4)


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/clang-offload-bundler"), reason="needs the ROCm LLVM tools")
def test_every_instantiation_has_no_scratch_and_its_waves_per_simd():
    ks = _kernels()
    panel = {k: v for k, v in ks.items() if "conv_panel_kernel" in k}
    assert len(panel) == len(INTENDED), sorted(panel)
    for (nk, bn), want in INTENDED.items():
        meta = panel[f"_ZN4pemp17conv_panel_kernelILi{nk}ELi{bn}ELi{NW}EEEvNS_8ConvArgsE"]
        assert int(meta["private_segment_fixed_size"]) == 0, (nk, bn, meta)
        assert _waves(meta, bn) == want, (nk, bn, want, meta)


def test_the_new_ids_have_a_registry_of_their_own(hip_lib):
    from pemp_amd import ops
    new = set(ops.SPLIT3_PANEL_TILES)
    assert new == {71, 72} and min(new) > 64
    for reg in (ops.TILE_VARIANTS, ops.SPLITK_TILES, ops.SPLIT3_TILES, ops.SPLIT3_SPLITK_TILES):
        assert not new & set(reg)
    assert ops.tile_shape(71) == (128, 128) and ops.tile_shape(72) == (128, 64)
    for t in new:
        bm, bn = C.c_int(-1), C.c_int(-1)
        assert hip_lib.pemp_conv2d_tile_shape(t, C.byref(bm), C.byref(bn)) == 1 and (bm.value, bn.value) == ops.tile_shape(t)
    for t in list(range(57, 71)) + list(range(73, 100)):
        assert ops.tile_shape(t) is None and hip_lib.pemp_conv2d_tile_shape(t, None, None) == 0, t


def test_ids_up_to_64_answer_as_before(hip_lib):
    """The recorded answers of the three id-decoding queries (tests/golden/conv_tile_queries.json) for every id 0..64, and the new
    ids take no part in statistics, split-K or hybrid launches."""
    from pemp_amd._lib import ConvDesc
    with open(T.GOLDEN) as f:
        want = json.load(f)
    assert T._queries(hip_lib, ConvDesc) == want
    for spec in T.DESCS.values():
        for t in (71, 72):
            d = T._desc(ConvDesc, spec, t)
            assert hip_lib.pemp_conv2d_stats_rows(C.byref(d)) == 0 and hip_lib.pemp_conv2d_splitk_workspace_bytes(C.byref(d)) == 0
