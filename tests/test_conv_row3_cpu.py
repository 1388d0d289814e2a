"""The row-stage forms of the pre-split 3x3 convs (conv_row3.hip, tile ids 246 / 249; include/pemp_hip.h), on the CPU:

 * the code object: no scratch, no spilled register, two waves per SIMD, LDS within the CU's 160 KiB;
 * the registry: the id, its shape, the candidate set and the pick key it is offered under, the A/B switch;
 * the capacity rule, on both sides of the C ABI;
 * what the entry refuses (nothing is launched, no pointer dereferenced)."""
import ctypes as C
import os
import subprocess

import pytest
import torch

from tests.test_conv_split3_persist_cpu import LLVM
from tests.test_conv_split3_presplit_cpu import _layer

KERNELS = {246: "_ZN4pemp16conv_row3_kernelENS_8ConvArgsE", 249: "_ZN4pemp17conv_row3p_kernelENS_8ConvArgsE"}
STAGE_ROWS, BM, BN, NW = 288, 256, 128, 8


def _kernels():
    """test_conv_split3_persist_cpu._kernels on conv_row3.o"""
    import re
    from pemp_amd import build
    build.build()
    obj = os.path.join(build.OBJ, "conv_row3.o")
    tmp = os.path.join(build.OBJ, "conv_row3.gfx950")
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


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/clang-offload-bundler"), reason="needs the ROCm LLVM tools")
@pytest.mark.parametrize("tile", sorted(KERNELS))
def test_code_object_uses_no_scratch_and_keeps_two_waves_per_simd(tile):
    ks = _kernels()
    assert sorted(k for k in ks if "conv_row3" in k) == sorted(KERNELS.values()), sorted(ks)      # every instantiation of the file
    meta = ks[KERNELS[tile]]
    assert int(meta["private_segment_fixed_size"]) == 0 and int(meta["vgpr_spill_count"]) == 0, meta
    regs = (int(meta["vgpr_count"]) + 3) // 4 * 4 + int(meta["agpr_count"])
    assert regs <= 256, meta                                                       # two waves per SIMD
    assert int(meta["group_segment_fixed_size"]) == 0                              # all of it is dynamic: the launch passes it
    spare = -(-STAGE_ROWS * 12 // (NW * 64)) * NW * 64 - STAGE_ROWS * 12           # the last A round's quads without a stage row
    lds = (2 * STAGE_ROWS * 12 + 2 * BN * 12 + spare) * 16
    assert spare == 128 and lds == 161792 and lds <= 163840


def test_registry_names_the_id(hip_lib):
    from pemp_amd import ops
    assert ops.SPLIT3_ROW3_TILES == (246, 249) and ops.ROW3_STAGE_ROWS == STAGE_ROWS
    assert ops.TILES[249].persistent_of == 246 and ops.TILES[246].persistent_of is None
    bm, bn = C.c_int(-1), C.c_int(-1)
    for t in ops.SPLIT3_ROW3_TILES:
        assert ops.tile_shape(t) == (BM, BN) == ops.tile_shape(146)
        assert hip_lib.pemp_conv2d_tile_shape(t, C.byref(bm), C.byref(bn)) == 1 and (bm.value, bn.value) == (BM, BN)
        for reg in (ops.SPLIT3_TILES, ops.SPLIT3_PANEL_TILES, ops.SPLIT3_PRESPLIT_TILES, ops.SPLIT3_SPLITK_TILES, ops.TILE_VARIANTS):
            assert t not in reg
    for t in list(range(200, 246)) + [247, 248] + list(range(250, 300)):
        assert ops.tile_shape(t) is None and hip_lib.pemp_conv2d_tile_shape(t, None, None) == 0, t


def test_capacity_rule():
    from pemp_amd import ops
    # 256 + 2 d pixels and d zero rows per image-row boundary a range of that length can contain
    assert ops.row3_stage_rows(51, 2) == 272 and ops.row3_stage_rows(51, 1) == 264
    assert ops.row3_stage_rows(40, 3) == 283 and ops.row3_stage_rows(9, 1) == 287 and ops.row3_stage_rows(17, 1) == 274
    assert ops.row3_stage_rows(13, 2) == 300
    assert all(ops.row3_stage_rows(51, d) > STAGE_ROWS for d in (6, 12, 18))       # the dilated ASPP branches
    for w in range(1, 120):                                                        # the bound against a walk over every tile start
        for d in (1, 2, 3):
            worst = max(256 + 2 * d + d * ((m0 + 255 + d) // w - (m0 - d) // w) for m0 in range(0, 4 * w * 256, 256))
            assert worst <= ops.row3_stage_rows(w, d), (w, d)


def _offered(ops, p, w=51, **kw):
    args = dict(residual=None, pad_value=None, out_split3=False, also_split3=None, per_image_shift=False)
    args.update(kw)
    return ops._row3_ok(p, w, **args)


def test_ops_offers_the_id_where_the_kernel_takes_the_call(monkeypatch):
    from pemp_amd import ops
    monkeypatch.setattr(ops, "SPLIT3_ROW3", True)
    p = _layer(ops, 64, 128, 3)
    assert _offered(ops, p)
    t = torch.zeros(1)
    assert not _offered(ops, p, residual=t) and not _offered(ops, p, pad_value=t) and not _offered(ops, p, out_split3=True)
    assert not _offered(ops, p, also_split3=t) and not _offered(ops, p, per_image_shift=True)
    p2 = _layer(ops, 64, 128, 3)
    p2.pad = p2.dil = 2
    assert _offered(ops, p2) and not _offered(ops, p2, w=13)
    p2.pad = 1
    assert not _offered(ops, p2)                                                   # pad != dil
    p2.pad, p2.stride = 2, 2
    assert not _offered(ops, p2)
    assert not _offered(ops, _layer(ops, 64, 128, 5)) and not _offered(ops, _layer(ops, 64, 128, 1))
    monkeypatch.setattr(ops, "SPLIT3_ROW3", False)
    assert not _offered(ops, p)


def test_switch_is_read_from_the_environment():
    from pemp_amd import ops
    assert ops.SPLIT3_ROW3 == (os.environ.get("PEMP_SPLIT3_ROW3", "1") != "0")


def test_picks_get_a_key_of_their_own_and_the_hook_never_sees_the_id(monkeypatch):
    """conv2d's pick path up to the choice (the launch itself is replaced: the tensors live on the CPU)."""
    from pemp_amd import ops
    seen = []

    def choose(key, rows, launch, cands, default):
        seen.append((key, cands(), default))
        raise StopIteration

    monkeypatch.setattr(ops, "_choose_tile", choose)
    monkeypatch.setattr(ops._lib, "load", lambda: None)
    monkeypatch.setattr(ops, "_chk_dev", lambda *a: None)
    monkeypatch.setattr(ops, "SPLIT3_ROW3", True)
    xs = torch.zeros(ops.split3_shape(1, 20, 51, 64), dtype=torch.bfloat16)
    narrow = torch.zeros(ops.split3_shape(1, 20, 13, 64), dtype=torch.bfloat16)
    p = _layer(ops, 64, 128, 3)
    p2 = _layer(ops, 64, 128, 3)
    p2.pad = p2.dil = 2
    for x, prm, hook, on, want in ((xs, p, None, True, True), (xs, p2, None, True, True), (narrow, p2, None, True, False),
                                   (xs, p, lambda *a: 146, True, False), (xs, p, None, False, False)):
        monkeypatch.setattr(ops, "PICK_HOOK", hook)
        monkeypatch.setattr(ops, "SPLIT3_ROW3", on)
        with pytest.raises(StopIteration):
            ops.conv2d(x, prm, x_split3=True)
        key, cands, default = seen.pop()
        assert cands == [146, 149] + [246, 249] * int(want) and default == 146, (key, cands)
        # the key says whether the kernel takes the call -- with the hook in place too, so that a hooked pick is replayed untimed
        assert (key[-1] == 246) == (want or (hook is not None and on)), key
        assert 146 in key


def _desc(ConvDesc, cin=64, cout=128, k=3, flags=None, tile=246, n=1, h=5, w=5, stride=1, pad=1, dil=1, ldx=None, ldy=None):
    from pemp_amd._lib import CONV_IN_SPLIT3
    ho, wo = (h + 2 * pad - dil * (k - 1) - 1) // stride + 1, (w + 2 * pad - dil * (k - 1) - 1) // stride + 1
    return ConvDesc(n, h, w, cin, ldx or cin, ho, wo, cout, ldy or cout, k, k, stride, pad, dil, cout, k * k * cin,
                    CONV_IN_SPLIT3 if flags is None else flags, tile)


def library_refusals(hip_lib, tile=246):
    """[(what, return code, message)] of the calls on id ``tile`` that the entries must refuse; shared with the GPU test."""
    from pemp_amd._lib import ConvDesc, CONV_OUT_SPLIT3 as OUT, CONV_IN_SPLIT3 as IN, CONV_SHIFT_PER_IMAGE as PER_IMG, CONV_OUT_SPLIT3_ALSO as ALSO
    y, s, p = C.c_void_p(0x10000), C.c_void_p(0x4000000), C.c_void_p(0x8000000)
    arr = (C.c_void_p * 1)(p)

    def conv(d, residual=None):
        rc = hip_lib.pemp_conv2d_nhwc_f32(C.byref(d), p, p, y, None, None, residual, None)
        return rc, hip_lib.pemp_last_error().decode()

    D = lambda **kw: _desc(ConvDesc, tile=tile, **kw)
    got = [
        ("OUT_SPLIT3", *conv(D(flags=IN | OUT))),
        ("OUT_SPLIT3_ALSO", *conv(D(flags=IN | ALSO), residual=s)),
        ("a residual", *conv(D(), residual=s)),
        ("a per-image shift", *conv(D(flags=IN | PER_IMG))),
        ("stride 2", *conv(D(stride=2, h=9, w=9))),
        ("pad != dil", *conv(D(pad=1, dil=2, h=9, w=9))),
        ("pad != dil (no padding)", *conv(D(pad=0, h=9, w=9))),
        ("5x5", *conv(D(k=5, pad=2))),
        ("1x1", *conv(D(k=1, pad=0))),
        ("Cout % 128", *conv(D(cout=64))),
        ("Cin % 32", *conv(D(cin=48))),
        ("ldx != Cin", *conv(D(ldx=128))),
        ("without IN_SPLIT3", *conv(D(flags=0))),
        ("more than 288 stage rows", *conv(D(n=2, h=20, w=13, pad=2, dil=2))),
        ("a dilated ASPP branch", *conv(D(n=2, h=51, w=51, cin=256, cout=256, pad=6, dil=6))),
    ]
    d = D()
    rc = hip_lib.pemp_conv2d_padv_nhwc_f32(C.byref(d), p, p, y, None, None, None, C.c_void_p(0x8000000 + (1 << 20)), None)     # behind x
    got.append(("a padding vector", rc, hip_lib.pemp_last_error().decode()))
    rc = hip_lib.pemp_conv2d_splitk_nhwc_f32(C.byref(d), p, p, y, None, None, None, p, 1 << 20, None)
    got.append(("split-K / workspace", rc, hip_lib.pemp_last_error().decode()))
    rc = hip_lib.pemp_conv2d_group_nhwc_f32(1, C.byref(d), arr, arr, arr, None, None, None, None, None)
    got.append(("grouped", rc, hip_lib.pemp_last_error().decode()))
    return got


@pytest.mark.parametrize("tile", [246, 249])
def test_library_refuses_what_the_id_does_not_take(hip_lib, tile):
    for what, rc, msg in library_refusals(hip_lib, tile):
        assert rc == -1 and msg, (what, rc, msg)
    # ... and the geometry refusals say so
    by = {what: msg for what, _, msg in library_refusals(hip_lib, tile)}
    for what in ("stride 2", "pad != dil", "a residual", "more than 288 stage rows", "a dilated ASPP branch", "a padding vector", "OUT_SPLIT3"):
        assert "unsupported" in by[what], (what, by[what])
