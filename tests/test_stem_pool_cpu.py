"""The fused stem (PEMP_CONV_POOL3S2: 7x7 / 2 / 3 split3 conv + 3 / 2 / 1 ceil-mode max-pool in one launch, csrc/conv_stem_pool.hip),
what can be held without a GPU: the entry point refuses the flag outside its one use before anything is launched, the pool-size
formula is ATen's, and the kernel's code object uses no scratch."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

LLVM = "/opt/rocm/llvm/bin"
FAKE = 1 << 20          # a 16-byte aligned address that is never dereferenced: every call below is refused by its arguments


def _lib():
    from pemp_amd import build, _lib
    build.build()
    return _lib


def _desc(L, flags, tile, cin=4, kpad=224, k=7, stride=2, pad=3, ldr=0):
    h = w = 23
    ho = (h + 2 * pad - k) // stride + 1
    return L.ConvDesc(1, h, w, cin, cin, ho, ho, 64, 64, k, k, stride, pad, 1, ldr, kpad, flags, tile)


def _refused(L, d, residual=None):
    lib = L.load()
    p = C.c_void_p(FAKE)
    rc = lib.pemp_conv2d_nhwc_f32(C.byref(d), p, p, p, None, None, C.c_void_p(residual) if residual else None, None)
    return rc != 0 and lib.pemp_last_error().decode()


def test_the_flag_is_refused_without_the_stem_or_split_weights():
    L = _lib()
    stem = L.CONV_STEM4 | L.CONV_POOL3S2
    # no STEM4: an ordinary 3x3 conv descriptor on a split3 id
    msg = _refused(L, _desc(L, L.CONV_POOL3S2, 43, cin=32, kpad=288, k=3, stride=1, pad=1))
    assert msg and "POOL3S2" in msg, msg
    # STEM4, but ids whose `w` is the plain fp32 pack (no split weights): auto, the fp32-chain families
    for tile in (0, 3, 13, 23, 29):
        msg = _refused(L, _desc(L, stem, tile))
        assert msg and "POOL3S2" in msg, (tile, msg)
    # a residual
    msg = _refused(L, _desc(L, stem, 43, ldr=64), residual=FAKE)
    assert msg and "POOL3S2" in msg, msg
    # a stem of another geometry (3x3 / 1 / 1, the VGG one) and a per-image shift
    msg = _refused(L, _desc(L, stem, 43, kpad=64, k=3, stride=1, pad=1))
    assert msg and "POOL3S2" in msg, msg
    msg = _refused(L, _desc(L, stem | L.CONV_SHIFT_PER_IMAGE, 43))
    assert msg and "POOL3S2" in msg, msg


def test_the_flag_is_refused_by_the_other_conv_entries():
    L = _lib()
    lib = L.load()
    d = _desc(L, L.CONV_STEM4 | L.CONV_POOL3S2, 43)
    p = C.c_void_p(FAKE)
    arr = (C.c_void_p * 1)(FAKE)
    assert lib.pemp_conv2d_group_nhwc_f32(1, C.byref(d), arr, arr, arr, None, None, None, None, None) != 0
    assert "POOL3S2" in lib.pemp_last_error().decode()
    assert lib.pemp_conv2d_bf16_nhwc(C.byref(d), p, p, p, None, None, None, None, 0, None) != 0


@pytest.mark.parametrize("i", range(1, 41))
def test_pool_size_formula_is_atens(i):
    from pemp_amd import ops
    want = F.max_pool2d(torch.zeros(1, 1, i, i), 3, 2, 1, ceil_mode=True).shape[-1]
    assert ops._pool_out(i, 3, 2, 1, True) == want
    assert i // 2 + 1 == want             # the closed form the header states for this window


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/clang-offload-bundler"), reason="needs the ROCm LLVM tools")
def test_the_kernel_uses_no_scratch_and_two_blocks_fit_a_cu():
    from pemp_amd import build
    build.build()
    obj = os.path.join(build.OBJ, "conv_stem_pool.o")
    tmp = os.path.join(build.OBJ, "conv_stem_pool.gfx950")
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
    (name, meta), = [(k, v) for k, v in out.items() if "conv_stem_pool_kernel" in k]
    assert int(meta["private_segment_fixed_size"]) == 0 and int(meta["vgpr_spill_count"]) == 0, meta
    # 10 waves per block, two blocks per CU (LDS: 2 x 73984 bytes <= 160 KiB): 5 waves per SIMD need <= 96 registers per lane
    regs = (int(meta["vgpr_count"]) + 7) // 8 * 8 + int(meta["agpr_count"])
    assert regs <= 96, meta
