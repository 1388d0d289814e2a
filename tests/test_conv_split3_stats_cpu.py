"""The statistics epilogue on the split3 family, CPU side: what pemp_split3_conv2d_stats_nhwc_f32 refuses before any launch
(the pointers are never dereferenced), what pemp_conv2d_stats_split3_rows answers, and the ``trunk_precision`` key of the three
head-training commands."""
import contextlib
import ctypes as C
import io

import pytest

OFFERED = (41, 42, 43, 44, 46)          # the unsplit split3 ids, on their own wave grids


def _desc(ConvDesc, cin, cout, k, flags, tile, n=2, h=13, w=13):
    return ConvDesc(n, h, w, cin, cin, h, w, cout, cout, k, k, 1, k // 2, 1, 0, k * k * cin, flags, tile)


def _call(lib, d, x=0x10000, w3=0x20000, y=0x30000, stats=0x40000):
    p = lambda v: C.c_void_p(v) if v else None
    return lib.pemp_split3_conv2d_stats_nhwc_f32(C.byref(d), p(x), p(w3), p(y), p(stats), None)


def test_entry_refuses_every_id_outside_the_offered_set(hip_lib):
    from pemp_amd._lib import ConvDesc
    for tile in [t for t in range(1, 65) if t not in OFFERED] + [71, 72, 146, 149]:
        assert _call(hip_lib, _desc(ConvDesc, 64, 256, 3, 0, tile)) == -1, tile
        assert b"conv2d_stats_split3" in hip_lib.pemp_last_error(), tile
    for tile in (23, 47, 49, 51, 56):                                   # the fp32 statistics id, persistent and split-K forms
        assert _call(hip_lib, _desc(ConvDesc, 64, 256, 1, 0, tile)) == -1, tile


def test_entry_refuses_flags_geometry_and_null_pointers(hip_lib):
    from pemp_amd import _lib
    from pemp_amd._lib import ConvDesc
    flags = {name: getattr(_lib, "CONV_" + name) for name in ("RELU", "SHIFT_PER_IMAGE", "OUT_SPLIT3", "IN_SPLIT3", "OUT_SPLIT3_ALSO", "STEM4")}
    assert len(set(flags.values())) == 6 and all(flags.values())
    for tile in (0,) + OFFERED:
        for name, f in flags.items():
            assert _call(hip_lib, _desc(ConvDesc, 64, 256, 3, f, tile)) == -1, (tile, name)
        assert _call(hip_lib, _desc(ConvDesc, 64, 96, 3, 0, tile)) == -1, tile            # Cout % 64
        assert _call(hip_lib, _desc(ConvDesc, 48, 256, 3, 0, tile)) == -1, tile           # Cin % 32
        for null in ("x", "w3", "y", "stats"):
            assert _call(hip_lib, _desc(ConvDesc, 64, 256, 3, 0, tile), **{null: 0}) == -1, (tile, null)
        assert _call(hip_lib, _desc(ConvDesc, 64, 256, 3, 0, tile), y=0x30004) == -1, tile    # misaligned
    from pemp_amd import ops
    for tile in OFFERED:                                                # Cout smaller than the id's BN
        bn = ops.tile_shape(tile)[1]
        if bn > 64:
            assert _call(hip_lib, _desc(ConvDesc, 64, bn // 2, 3, 0, tile)) == -1, tile
            assert _call(hip_lib, _desc(ConvDesc, 64, bn + 64, 3, 0, tile)) == -1, tile   # ... or no multiple of it


def test_rows_query(hip_lib):
    from pemp_amd import ops
    from pemp_amd._lib import ConvDesc
    cdiv = lambda a, b: (a + b - 1) // b
    for n, h, w in ((2, 13, 13), (1, 7, 9), (3, 9, 9)):
        m = n * h * w
        for tile in list(range(0, 65)) + [71, 72, 146, 149]:
            got = hip_lib.pemp_conv2d_stats_split3_rows(C.byref(_desc(ConvDesc, 64, 256, 3, 0, tile, n, h, w)))
            if tile in OFFERED:
                assert got == cdiv(m, ops.tile_shape(tile)[0]), tile
            elif tile == 0:
                assert got == cdiv(m, ops.tile_shape(43)[0])            # 0 runs as 43
            else:
                assert got == 0, tile
    assert hip_lib.pemp_conv2d_stats_split3_rows(None) == 0
    # the python side offers what the library answers for, and the fp32 statistics query is what it was
    assert sorted(ops.split3_stats_tiles(256)) == sorted(OFFERED)
    assert sorted(ops.split3_stats_tiles(64)) == [42, 43]
    assert hip_lib.pemp_conv2d_stats_rows(C.byref(_desc(ConvDesc, 64, 256, 3, 0, 43))) == 0


@pytest.mark.parametrize("name", ["canet", "pfenet", "rpmms"])
def test_print_config_shows_trunk_precision(name):
    import importlib
    entry = importlib.import_module(f"pemp_amd.entry.{name}")
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        entry.ex.run_commandline([name, "print_config"])
    text = buf.getvalue()
    assert "'trunk_precision'" in text and "'f32_chain'" in text
    net = getattr(entry, "net_ingredient", None)                        # a key of the command, not of the network
    assert net is None or "trunk_precision" not in net.cfg


def test_trunk_precision_is_checked_before_anything_is_built(monkeypatch):
    from pemp_amd import engine, train_engine
    from pemp_amd.train_canet import CANetTrainer
    with pytest.raises(ValueError):
        train_engine.check_trunk_precision("bf16")
    train_engine.check_trunk_precision("f32_chain")
    monkeypatch.setattr(engine, "SPLIT3", True)
    train_engine.check_trunk_precision("split3")
    monkeypatch.setattr(engine, "SPLIT3", False)                        # what PEMP_SPLIT3=0 sets
    train_engine.check_trunk_precision("f32_chain")
    with pytest.raises(ValueError, match="PEMP_SPLIT3"):
        train_engine.check_trunk_precision("split3")
    assert train_engine.TRUNK_PRECISIONS == ("f32_chain", "split3")
    import inspect
    from pemp_amd.train_pfenet import PFENetTrainer
    from pemp_amd.train_rpmms import RPMMsTrainer
    for cls in (CANetTrainer, PFENetTrainer, RPMMsTrainer):
        assert inspect.signature(cls.__init__).parameters["trunk_precision"].default == "f32_chain"
    # a trainer that trains its trunk has no such switch: the keyword raises before the model is looked at
    from pemp_amd.train_baseline import BaselineTrainer
    from pemp_amd.train_stage2 import Stage2Trainer
    for make in (lambda **kw: train_engine.Stage1Trainer(None, **kw), lambda **kw: BaselineTrainer(None, **kw),
                 lambda **kw: Stage2Trainer(None, None, **kw)):
        for value in ("split3", "f32_chain"):
            with pytest.raises(ValueError, match="trunk_precision"):
                make(trunk_precision=value)
