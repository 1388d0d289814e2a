"""PFENet head-training kernels (csrc/pfenet_bwd.hip) without a GPU: every new entry point is declared, bound with the
declared number of arguments and exported, its argument checks answer before any device work, and the workspace size is the
documented one."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ("pemp_weighted_gap_bwd_f32", "pemp_adaptive_avgpool_bwd_multi_nhwc_f32", "pemp_resize_bilinear_ac_bwd_nhwc_f32",
       "pemp_pfenet_merge_support_bwd_workspace_bytes", "pemp_pfenet_merge_support_bwd_f32")


def _declared_args(name):
    with open(os.path.join(ROOT, "include", "pemp_hip.h")) as f:
        header = f.read()
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, f"{name} is not declared in include/pemp_hip.h"
    return [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]


def test_new_symbols_are_bound_as_declared(hip_lib):
    from pemp_amd import _lib
    for name in NEW:
        assert name in _lib.SYMBOLS, name
        assert len(_lib.SYMBOLS[name][1]) == len(_declared_args(name)), name
        assert getattr(hip_lib, name) is not None
    assert _lib.ABI_VERSION == 2 and hip_lib.pemp_abi_version() == 2          # additions only


def test_sources_and_wrappers_exist():
    from pemp_amd import build, train_ops as T
    assert "pfenet_bwd.hip" in build.SOURCES
    for fn in ("weighted_gap_bwd", "adaptive_avgpool_bwd_multi", "resize_bilinear_ac_bwd", "pfenet_merge_support_bwd"):
        assert callable(getattr(T, fn))


def test_argument_checks_answer_before_any_device_work(hip_lib):
    ptr, ints = ctypes.c_void_p * 1, ctypes.c_int * 1
    one = ctypes.c_void_p(64)                                                 # an aligned non-null address: never dereferenced
    assert hip_lib.pemp_weighted_gap_bwd_f32(None, None, None, 256, 1, 1, 13, 13, 256, None) == -1
    assert b"null pointer" in hip_lib.pemp_last_error()
    assert hip_lib.pemp_weighted_gap_bwd_f32(one, one, one, 256, 1, 1, 13, 13, 254, None) == -1          # C % 4
    assert hip_lib.pemp_weighted_gap_bwd_f32(one, one, one, 128, 1, 1, 13, 13, 256, None) == -1          # ldd < C
    assert hip_lib.pemp_adaptive_avgpool_bwd_multi_nhwc_f32(5, ptr(64), ints(256), ints(8), ints(8), one, 256, 1, 13, 13, 256, None) == -1
    assert b"bins" in hip_lib.pemp_last_error()
    assert hip_lib.pemp_adaptive_avgpool_bwd_multi_nhwc_f32(1, ptr(64), ints(128), ints(8), ints(8), one, 256, 1, 13, 13, 256, None) == -1
    assert hip_lib.pemp_adaptive_avgpool_bwd_multi_nhwc_f32(1, ptr(64), ints(256), ints(0), ints(8), one, 256, 1, 13, 13, 256, None) == -1
    assert hip_lib.pemp_adaptive_avgpool_bwd_multi_nhwc_f32(1, ptr(None), ints(256), ints(8), ints(8), one, 256, 1, 13, 13, 256, None) == -1
    assert hip_lib.pemp_resize_bilinear_ac_bwd_nhwc_f32(None, 0, 1, 1, None, 0, 0, 0, None, 0, 1, 1, 1, 1, 1, 1, 1, 1, None) == -1
    assert hip_lib.pemp_resize_bilinear_ac_bwd_nhwc_f32(one, 0, 1, 1, None, 0, 0, 0, one, 0, 1, 1, 1, 1, 0, 1, 1, 1, None) == -1
    assert hip_lib.pemp_resize_bilinear_ac_bwd_nhwc_f32(one, 0, 1, 1, one, 0, 0, 1, one, 0, 1, 1, 1, 1, 1, 1, 1, 1, None) == -1   # add stride 0
    assert hip_lib.pemp_pfenet_merge_support_bwd_f32(1, ptr(64), ints(256), ints(8), ints(8), ptr(64), ptr(64), 513, one, one, one, 0,
                                                     2, 256, 256, None) == -1
    assert b"workspace too small" in hip_lib.pemp_last_error()
    assert hip_lib.pemp_pfenet_merge_support_bwd_f32(1, ptr(64), ints(256), ints(8), ints(8), ptr(64), ptr(64), 128, one, one, one,
                                                     1 << 30, 2, 256, 256, None) == -1                    # ldw < Cin
    # part [bins][B][64 blocks][Cout] + csum [bins][B][Cout]
    assert hip_lib.pemp_pfenet_merge_support_bwd_workspace_bytes(4, 2, 256) == 4 * 2 * 65 * 256 * 4
    assert hip_lib.pemp_pfenet_merge_support_bwd_workspace_bytes(0, 2, 256) == 0
