"""Register budget of the persistent split3 kernels (conv_dma2.hip: conv_dma2_s3p_kernel, ids 47 / 49), read from the built
gfx950 code object: no scratch, and no fewer waves per SIMD than the one-tile-per-block kernel of the same shape (ids 43 / 46),
counting both registers and LDS.  The persistent loop keeps the next tile's offsets and the epilogue's batched loads in
registers; that must not cost a wave."""
import os
import re
import subprocess

import pytest

LLVM = "/opt/rocm/llvm/bin"
# id -> (BM, BN, WGM, NW) of the one-tile kernel and of its persistent form
SHAPES = {47: (64, 64, 2, 4), 49: (256, 128, 8, 8)}


def _kernels():
    from pemp_amd import build
    build.build()
    obj = os.path.join(build.OBJ, "conv_dma2.o")
    tmp = os.path.join(build.OBJ, "conv_dma2.gfx950")
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


def _waves(meta, bm, bn, nw):
    regs = (int(meta["vgpr_count"]) + 3) // 4 * 4 + int(meta["agpr_count"])
    by_regs = min(8, 512 // regs)
    lds = 2 * (8 * bm + 12 * bn) * 16
    by_lds = (160 * 1024 // lds) * nw // 4
    return min(by_regs, by_lds)


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/clang-offload-bundler"), reason="needs the ROCm LLVM tools")
@pytest.mark.parametrize("tile", sorted(SHAPES))
def test_persistent_kernels_keep_occupancy_and_use_no_scratch(tile):
    ks = _kernels()
    bm, bn, wgm, nw = SHAPES[tile]
    for padv in (0, 1):
        one = ks[f"_ZN4pemp16conv_dma2_kernelILi{bm}ELi{bn}ELi{wgm}ELi{nw}ELb{padv}ELi0ELb0ELb0ELb0ELb0ELb1EEEvNS_8ConvArgsE"]
        per = ks[f"_ZN4pemp20conv_dma2_s3p_kernelILi{bm}ELi{bn}ELi{wgm}ELi{nw}ELb{padv}EEEvNS_8ConvArgsE"]
        assert int(per["private_segment_fixed_size"]) == 0 and int(per["vgpr_spill_count"]) == 0, (tile, padv, per)
        assert _waves(per, bm, bn, nw) >= _waves(one, bm, bn, nw), (tile, padv, per, one)
