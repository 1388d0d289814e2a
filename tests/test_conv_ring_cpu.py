"""The three-deep activation ring of the long-K 1x1 convs (conv_ring.hip, tile id 349; include/pemp_hip.h), on the CPU:

 * the code object of both instantiations: no scratch, no spilled register, two waves per SIMD, LDS within the CU's 160 KiB;
 * the registry: the id, its shape, the candidate sets and the pick key it is offered under, the A/B switch, the test hook;
 * ``ops._ring_ok`` against the library's own rule, on both sides of the C ABI;
 * what the entries refuse (nothing is launched, no pointer dereferenced)."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from tests.test_conv_split3_persist_cpu import LLVM
from tests.test_conv_split3_presplit_cpu import _layer

RING = 349
KERNELS = {0: "_ZN4pemp16conv_ring_kernelILi0EEEvNS_8ConvArgsE", 1: "_ZN4pemp16conv_ring_kernelILi1EEEvNS_8ConvArgsE"}      # OUT 0 / 1
BM, BN, NW = 256, 128, 8


def _kernels():
    """test_conv_split3_persist_cpu._kernels on conv_ring.o"""
    from pemp_amd import build
    build.build()
    obj = os.path.join(build.OBJ, "conv_ring.o")
    tmp = os.path.join(build.OBJ, "conv_ring.gfx950")
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
@pytest.mark.parametrize("out", sorted(KERNELS))
def test_code_object_uses_no_scratch_and_keeps_two_waves_per_simd(out):
    ks = _kernels()
    assert sorted(k for k in ks if "conv_ring" in k) == sorted(KERNELS.values()), sorted(ks)      # every instantiation of the file
    meta = ks[KERNELS[out]]
    assert int(meta["private_segment_fixed_size"]) == 0 and int(meta["vgpr_spill_count"]) == 0, meta
    regs = (int(meta["vgpr_count"]) + 3) // 4 * 4 + int(meta["agpr_count"])
    assert regs <= 256, meta                                                       # two waves per SIMD
    assert int(meta["group_segment_fixed_size"]) == 0                              # all of it is dynamic: the launch passes it
    lds = (3 * BM * 8 + 2 * BN * 12) * 16                                          # A [3][256][8] quads, B [2][128][12] quads
    assert lds == 147456 and lds <= 163840


def test_registry_names_the_id(hip_lib):
    from pemp_amd import ops
    assert ops.SPLIT3_RING_TILES == (RING,) and ops.RING_MIN_K == 128
    assert ops.TILES[RING].family == "split3" and not ops.TILES[RING].splitk and ops.TILES[RING].persistent_of == 46
    bm, bn = C.c_int(-1), C.c_int(-1)
    assert ops.tile_shape(RING) == (BM, BN) == ops.tile_shape(49)
    assert hip_lib.pemp_conv2d_tile_shape(RING, C.byref(bm), C.byref(bn)) == 1 and (bm.value, bn.value) == (BM, BN)
    for reg in (ops.SPLIT3_TILES, ops.SPLIT3_PANEL_TILES, ops.SPLIT3_PRESPLIT_TILES, ops.SPLIT3_ROW3_TILES, ops.SPLIT3_SPLITK_TILES,
                ops.TILE_VARIANTS, ops.SPLIT3_RES_S2_TILES, ops.SPLIT3_PERSISTENT):
        assert RING not in reg
    for t in list(range(300, RING)) + list(range(RING + 1, 400)):
        assert ops.tile_shape(t) is None and hip_lib.pemp_conv2d_tile_shape(t, None, None) == 0, t


def _offered(ops, p, **kw):
    args = dict(x_split3=False, residual=None, pad_value=None, also_split3=None, splitk=False)
    args.update(kw)
    return ops._ring_ok(p, **args)


def test_ops_offers_the_id_where_the_kernel_takes_the_call(monkeypatch):
    from pemp_amd import ops
    monkeypatch.setattr(ops, "SPLIT3_RING", True)
    monkeypatch.setattr(ops, "PICK_HOOK", None)
    p = _layer(ops, 1024, 256, 1)
    assert _offered(ops, p) and _offered(ops, _layer(ops, 128, 128, 1)) and _offered(ops, _layer(ops, 160, 512, 1))
    p.stride = 2
    assert _offered(ops, p)                                                        # any stride
    t = torch.zeros(1)
    assert not _offered(ops, p, residual=t) and not _offered(ops, p, pad_value=t) and not _offered(ops, p, also_split3=t)
    assert not _offered(ops, p, x_split3=True) and not _offered(ops, p, splitk=True) and not _offered(ops, p, res_s2=True)
    assert not _offered(ops, _layer(ops, 96, 256, 1))                              # three K steps: the ring does not fill
    assert not _offered(ops, _layer(ops, 1024, 192, 1)) and not _offered(ops, _layer(ops, 1024, 64, 1))      # Cout % 128
    assert not _offered(ops, _layer(ops, 128, 128, 3))                             # multi-tap
    padded = _layer(ops, 1024, 256, 1)
    padded.pad = 1
    assert not _offered(ops, padded)
    assert not _offered(ops, _layer(ops, 1024, 256, 1, split=False))               # no split weights: the fp32 chain
    monkeypatch.setattr(ops, "PICK_HOOK", lambda *a: 43)
    assert not _offered(ops, _layer(ops, 1024, 256, 1))                            # the hook decides among the other ids
    monkeypatch.setattr(ops, "PICK_HOOK", None)
    monkeypatch.setattr(ops, "SPLIT3_RING", False)
    assert not _offered(ops, _layer(ops, 1024, 256, 1))


def test_switch_is_read_from_the_environment():
    from pemp_amd import ops
    assert ops.SPLIT3_RING == (os.environ.get("PEMP_SPLIT3_RING", "1") != "0")


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
    monkeypatch.setattr(ops, "SPLIT3_PANEL", True)
    monkeypatch.setattr(ops, "EVAL_SPLITK", False)
    x = torch.zeros(1, 20, 51, 1024)
    res = torch.zeros(1, 20, 51, 256)
    long_k, short_k = _layer(ops, 1024, 256, 1), _layer(ops, 256, 256, 1)
    few = _layer(ops, 96, 256, 1)
    base = list(ops.SPLIT3_TILES)
    # (x, layer, kwargs, hook, switch) -> the id is offered?
    for xx, prm, kw, hook, on, want in ((x, long_k, {}, None, True, True),
                                       (x, long_k, dict(out_split3=True), None, True, True),
                                       (x, long_k, dict(per_image_shift=True, shift_override=torch.zeros(1, 256)), None, True, True),
                                       (x, long_k, dict(residual=res), None, True, False),
                                       (x, long_k, {}, lambda *a: 43, True, False),
                                       (x, long_k, dict(out_split3=True), lambda *a: 43, True, False),
                                       (x, long_k, {}, None, False, False),
                                       (x[..., :256], short_k, {}, None, True, True),
                                       (x[..., :96], few, {}, None, True, False)):
        monkeypatch.setattr(ops, "PICK_HOOK", hook)
        monkeypatch.setattr(ops, "SPLIT3_RING", on)
        with pytest.raises(StopIteration):
            ops.conv2d(xx, prm, **kw)
        key, cands, default = seen.pop()
        assert (RING in cands) == want and (RING in key) == want, (kw, key, cands)
        assert default == 43
        rest = [t for t in cands if t != RING]
        panel = hook is None and prm.kpad <= 256 and not kw.get("out_split3") and not kw.get("per_image_shift")
        assert rest == base + list(ops.SPLIT3_PANEL_TILES) * int(panel), (kw, cands)
        if want and panel:                       # the panel suffix stays last: the keys of calls without the id are what they were
            assert key[-2:] == (RING, 71) and cands[-3:] == [RING, 71, 72]
        elif want:
            assert key[-1] == RING and cands[-1] == RING


def _desc(ConvDesc, cin=128, cout=128, k=1, flags=0, tile=RING, n=1, h=5, w=5, stride=1, pad=0, dil=1, ldx=None, ldy=None):
    ho, wo = (h + 2 * pad - dil * (k - 1) - 1) // stride + 1, (w + 2 * pad - dil * (k - 1) - 1) // stride + 1
    return ConvDesc(n, h, w, cin, ldx or cin, ho, wo, cout, ldy or cout, k, k, stride, pad, dil, cout, k * k * cin, flags, tile)


def library_refusals(hip_lib):
    """[(what, return code, message)] of the calls on the id that the entries must refuse; shared with the GPU test."""
    from pemp_amd._lib import (ConvDesc, CONV_OUT_SPLIT3 as OUT, CONV_IN_SPLIT3 as IN, CONV_OUT_SPLIT3_ALSO as ALSO, CONV_RES_S2 as RES_S2,
                               CONV_STEM4 as STEM4, CONV_POOL3S2 as POOL)
    y, s, p = C.c_void_p(0x10000), C.c_void_p(0x4000000), C.c_void_p(0x8000000)
    arr = (C.c_void_p * 1)(p)
    err = lambda: hip_lib.pemp_last_error().decode()

    def conv(d, residual=None):
        rc = hip_lib.pemp_conv2d_nhwc_f32(C.byref(d), p, p, y, None, None, residual, None)
        return rc, err()

    D = lambda **kw: _desc(ConvDesc, **kw)
    got = [
        ("a residual", *conv(D(), residual=s)),
        ("OUT_SPLIT3_ALSO", *conv(D(flags=ALSO), residual=s)),
        ("IN_SPLIT3", *conv(D(flags=IN))),
        ("RES_S2", *conv(D(flags=RES_S2, h=9, w=9, stride=2), residual=s)),
        ("OUT_SPLIT3 with a residual", *conv(D(flags=OUT), residual=s)),
        ("OUT_SPLIT3 into a channel window", *conv(D(flags=OUT, ldy=256))),
        ("3x3", *conv(D(k=3, pad=1))),
        ("3x3 without padding", *conv(D(k=3, pad=0))),
        ("1x1 with padding", *conv(D(pad=1))),
        ("three K steps", *conv(D(cin=96))),
        ("one K step", *conv(D(cin=32))),
        ("Cout % 128", *conv(D(cout=192))),
        ("Cout 64", *conv(D(cout=64))),
        ("the stem", *_stem(hip_lib, ConvDesc, STEM4, p, y)),
        ("the fused stem", *_stem(hip_lib, ConvDesc, STEM4 | POOL, p, y)),
    ]
    d = D(k=3, pad=1)
    rc = hip_lib.pemp_conv2d_padv_nhwc_f32(C.byref(d), p, p, y, None, None, None, C.c_void_p(0x8000000 + (1 << 20)), None)     # behind x
    got.append(("a padding vector", rc, err()))
    d = D()
    rc = hip_lib.pemp_conv2d_padv_nhwc_f32(C.byref(d), p, p, y, None, None, None, C.c_void_p(0x8000000 + (1 << 20)), None)
    got.append(("a padding vector on the 1x1 conv", rc, err()))
    rc = hip_lib.pemp_conv2d_splitk_nhwc_f32(C.byref(d), p, p, y, None, None, None, p, 1 << 20, None)
    got.append(("split-K / workspace", rc, err()))
    rc = hip_lib.pemp_conv2d_group_nhwc_f32(1, C.byref(d), arr, arr, arr, None, None, None, None, None)
    got.append(("grouped", rc, err()))
    rc = hip_lib.pemp_split3_conv2d_stats_nhwc_f32(C.byref(d), p, p, y, s, None)
    got.append(("statistics (split3)", rc, err()))
    rc = hip_lib.pemp_conv2d_stats_nhwc_f32(C.byref(d), p, p, y, s, None, 0, None)
    got.append(("statistics (fp32 chain)", rc, err()))
    rc = hip_lib.pemp_conv2d_dropblock_nhwc_f32(C.byref(d), p, p, y, None, None, None, s, s, None, 0, None)
    got.append(("DropBlock", rc, err()))
    rc = hip_lib.pemp_conv2d_bf16_nhwc(C.byref(d), p, p, y, None, None, None, None, 0, None)
    got.append(("bf16", rc, err()))
    return got


def _stem(hip_lib, ConvDesc, flags, p, y):
    """the 7x7 / 2 / 3 NHWC4 stem (Kpad 224) on the id"""
    d = ConvDesc(1, 32, 32, 4, 4, 16, 16, 128, 128, 7, 7, 2, 3, 1, 128, 224, flags, RING)
    rc = hip_lib.pemp_conv2d_nhwc_f32(C.byref(d), p, p, y, None, None, None, None)
    return rc, hip_lib.pemp_last_error().decode()


UNSUPPORTED = ("a residual", "OUT_SPLIT3_ALSO", "IN_SPLIT3", "RES_S2", "OUT_SPLIT3 with a residual", "OUT_SPLIT3 into a channel window", "3x3",
               "3x3 without padding", "1x1 with padding", "three K steps", "one K step", "Cout % 128", "the stem", "the fused stem",
               "a padding vector", "split-K / workspace")


def test_library_refuses_what_the_id_does_not_take(hip_lib):
    got = library_refusals(hip_lib)
    for what, rc, msg in got:
        assert rc == -1 and msg, (what, rc, msg)
    by = {what: msg for what, _, msg in got}
    for what in UNSUPPORTED:                     # the id's own refusals say so
        assert "unsupported" in by[what], (what, by[what])


def test_ring_ok_agrees_with_the_library(hip_lib, monkeypatch):
    """The same geometries on both sides of the C ABI: where ``_ring_ok`` is false for a reason the descriptor shows, the entry refuses
    (dummy pointers: nothing may be launched); where it is true the descriptor passes every check up to the launch -- seen from here as
    an error that is NOT a refusal (no device), or as success."""
    from pemp_amd import ops
    from pemp_amd._lib import ConvDesc
    monkeypatch.setattr(ops, "SPLIT3_RING", True)
    monkeypatch.setattr(ops, "PICK_HOOK", None)
    p_, y_ = C.c_void_p(0x8000000), C.c_void_p(0x10000)
    for cin, cout, k, pad, stride in ((96, 256, 1, 0, 1), (32, 128, 1, 0, 1), (128, 192, 1, 0, 1), (128, 64, 1, 0, 1), (128, 128, 3, 1, 1),
                                      (128, 128, 3, 0, 1), (128, 128, 1, 1, 1), (128, 128, 1, 1, 2)):
        prm = _layer(ops, cin, cout, k)
        prm.pad, prm.stride = pad, stride
        assert not _offered(ops, prm), (cin, cout, k, pad, stride)
        d = _desc(ConvDesc, cin=cin, cout=cout, k=k, pad=pad, stride=stride, h=9, w=9)
        rc = hip_lib.pemp_conv2d_nhwc_f32(C.byref(d), p_, p_, y_, None, None, None, None)
        assert rc == -1 and "unsupported" in hip_lib.pemp_last_error().decode(), (cin, cout, k, pad, stride)
