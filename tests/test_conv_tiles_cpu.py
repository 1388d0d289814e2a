"""The conv engine's tile ids: the Python registry (ops.tile_shape) and the library's table (pemp_conv2d_tile_shape) name the
same ids and shapes, and the three CPU-side queries that decode an id -- pemp_conv2d_stats_rows,
pemp_conv2d_splitk_workspace_bytes, pemp_conv2d_hybrid_rows -- answer for every id 0..64 what they answered before the
dispatch was gathered into one table (tests/golden/conv_tile_queries.json, recorded from the commit before it with
``python tests/test_conv_tiles_cpu.py <out.json>``: a record of that library, never to be re-made from the one under test).
No GPU: the queries assume the MI355X's 256 CUs."""
import ctypes as C
import json
import os
import sys

IDS = range(65)
#: name -> (N, H, W, Cin, Cout, K, stride, pad, dil)
DESCS = {
    "3x3_64_256_338rows": (2, 13, 13, 64, 256, 3, 1, 1, 1),        # 6 tiles of 128 x 128, Kpad 576: every split-K id gets a workspace
    "1x1_32_256_one_episode": (2, 51, 51, 32, 256, 1, 1, 0, 1),    # 5202 rows: the hybrid launch splits (4096 rows on 64 x 64)
    "1x1_64_128_63rows": (1, 7, 9, 64, 128, 1, 1, 0, 1),           # Kpad 64: nothing to split along K; Cout below the widest tiles
    "3x3_64_64_layer1": (2, 101, 101, 64, 64, 3, 1, 1, 1),         # 20402 rows on 64 channels: hybrid rows again, 64-wide tiles only
    "3x3s2_256_512_dil": (8, 51, 51, 256, 512, 3, 2, 2, 2),        # strided + dilated, 5408 rows: a remainder round on the large tiles
}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_tile_queries.json")


def _desc(ConvDesc, spec, tile):
    n, h, w, cin, cout, k, s, p, d = spec
    ho, wo = (h + 2 * p - d * (k - 1) - 1) // s + 1, (w + 2 * p - d * (k - 1) - 1) // s + 1
    return ConvDesc(n, h, w, cin, cin, ho, wo, cout, cout, k, k, s, p, d, 0, k * k * cin, 0, tile)


def _queries(lib, ConvDesc):
    out = {}
    for name, spec in DESCS.items():
        rows, ws, hyb = [], [], []
        for t in IDS:
            d = _desc(ConvDesc, spec, t)
            rows.append(int(lib.pemp_conv2d_stats_rows(C.byref(d))))
            ws.append(int(lib.pemp_conv2d_splitk_workspace_bytes(C.byref(d))))
            hyb.append(int(lib.pemp_conv2d_hybrid_rows(C.byref(d))))
        out[name] = {"stats_rows": rows, "splitk_workspace_bytes": ws, "hybrid_rows": hyb}
    return out


def test_registry_and_library_name_the_same_tiles(hip_lib):
    from pemp_amd import ops
    known = []
    for t in IDS:
        bm, bn = C.c_int(-1), C.c_int(-1)
        rc = hip_lib.pemp_conv2d_tile_shape(t, C.byref(bm), C.byref(bn))
        if ops.tile_shape(t) is None:
            assert rc == 0 and (bm.value, bn.value) == (-1, -1), t
        else:
            assert rc == 1 and ops.tile_shape(t) == (bm.value, bn.value), t
            known.append(t)
    assert hip_lib.pemp_conv2d_tile_shape(23, None, None) == 1            # the outputs are optional
    # every id an entry point takes, and no other (0 = "pick for me" is not a tile)
    assert known == [1, 2, 3] + list(range(11, 18)) + list(range(21, 30)) + [31, 32, 34, 35, 36, 37] + [41, 42, 43, 44, 46, 47, 49] + [51, 52, 54, 56]
    assert set(ops.TILE_VARIANTS) | set(ops.SPLITK_TILES) | set(ops.SPLIT3_TILES) | set(ops.SPLIT3_SPLITK_TILES) | {1, 2} == set(known)
    for t, shape in ops.TILE_VARIANTS.items():
        assert ops.tile_shape(t) == shape
    for t in known:
        assert ops._tile_bn(t) == ops.tile_shape(t)[1]
    assert ops.tile_shape(47) == ops.tile_shape(43) and ops.tile_shape(49) == ops.tile_shape(46)      # persistent forms walk those shapes
    assert ops.tile_shape(29) == ops.tile_shape(23)                                                    # the hybrid launch's main member


def test_id_queries_answer_as_before_the_table(hip_lib):
    from pemp_amd._lib import ConvDesc
    with open(GOLDEN) as f:
        want = json.load(f)
    got = _queries(hip_lib, ConvDesc)
    assert set(got) == set(want)
    for name in DESCS:
        for q in ("stats_rows", "splitk_workspace_bytes", "hybrid_rows"):
            assert got[name][q] == want[name][q], (name, q)
    # the record exercises what it is meant to: a workspace for at least one split-K id of each family, hybrid rows somewhere
    ws = want["3x3_64_256_338rows"]["splitk_workspace_bytes"]
    assert all(ws[t] > 0 for t in (31, 32, 34, 35, 36, 37, 51, 52, 54, 56)) and sum(1 for v in ws if v) == 10
    assert want["1x1_32_256_one_episode"]["hybrid_rows"][29] == 4096 and want["3x3_64_64_layer1"]["hybrid_rows"][29] == 16384
    assert want["1x1_64_128_63rows"]["stats_rows"][0] == 1 and want["3x3_64_256_338rows"]["stats_rows"][26] == 2


if __name__ == "__main__":      # record the answers of whatever library this checkout has built
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from pemp_amd import _lib
    with open(sys.argv[1], "w") as f:
        json.dump(_queries(_lib.load(), _lib.ConvDesc), f, separators=(",", ":"))
        f.write("\n")
