"""Tensor-level wrappers over the C ABI (include/pemp_hip.h).

PyTorch is plumbing here: it owns device memory and the current stream; every function passes
raw device pointers + the current HIP stream to libpemp_hip.so.  Activations are NHWC fp32
tensors ``[N,H,W,C]`` whose last-dim stride is 1; a channel slice of a wider buffer is passed
as a view (its pixel stride ``ld`` is taken from ``stride(2)``).
"""
import ctypes as C
import collections
import functools
import json
import os

import torch

from . import _lib
from ._lib import ConvDesc, CONV_RELU, CONV_SHIFT_PER_IMAGE, CONV_STEM4, CONV_POOL3S2, CONV_OUT_SPLIT3, CONV_IN_SPLIT3, CONV_OUT_SPLIT3_ALSO  # noqa: F401
from ._lib import CONV_RES_S2, CONV_RES_HEVEN, CONV_RES_WEVEN


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _chk_dev(*ts):
    for t in ts:
        if t is not None and (not t.is_cuda):
            raise _lib.PempHipError("pemp_amd ops need device (cuda/HIP) tensors; there is no CPU path")


def _nhwc(t, name, dtype=torch.float32):
    if t.dim() != 4 or t.dtype != dtype or t.stride(3) != 1:
        raise ValueError(f"{name}: expected {dtype} NHWC view with unit channel stride, got {tuple(t.shape)} {t.dtype} {t.stride()}")
    n, h, w, c = t.shape
    # strides of size-1 dims are arbitrary in torch: take the pixel stride from the first dim that moves
    if w > 1:
        ld = t.stride(2)
    elif h > 1:
        ld = t.stride(1)
    elif n > 1:
        ld = t.stride(0)
    else:
        ld = c
    if (w > 1 and h > 1 and t.stride(1) != w * ld) or (h * w > 1 and n > 1 and t.stride(0) != h * w * ld):
        raise ValueError(f"{name}: pixels must be densely packed with stride ld={ld}, got strides {t.stride()}")
    return ld


def conv_out_size(i, k, s, p, d):
    return (i + 2 * p - d * (k - 1) - 1) // s + 1


class ConvParams:
    """Device-resident, pre-packed parameters of one conv (+ folded per-channel affine)."""
    __slots__ = ("w", "scale", "shift", "cin", "cout", "kh", "kw", "stride", "pad", "dil", "kpad", "stem", "relu", "w3", "w3pool")

    def __init__(self, w, scale, shift, cin, cout, kh, kw, stride, pad, dil, kpad, stem, relu, w3=None, w3pool=None):
        # w3: the split form of w (pack_split3) -- when present, conv2d / conv2d_group run the split3 family (tile ids 41..56) and
        # conv2d_stats its statistics form (SPLIT3_STATS_TILES)
        # w3pool: the split form of a 7x7 / 2 / 3 NHWC4 stem's w, for the fused stem + max-pool launch (stem_pool); conv2d never
        # reads it: a stem on its own stays on the fp32 chain, w3 stays None
        self.w, self.scale, self.shift, self.w3, self.w3pool = w, scale, shift, w3, w3pool
        self.cin, self.cout, self.kh, self.kw = cin, cout, kh, kw
        self.stride, self.pad, self.dil, self.kpad, self.stem, self.relu = stride, pad, dil, kpad, stem, relu


#: ---- tile ids (the scheme: include/pemp_hip.h, at pemp_conv2d_tile_shape).  The last digit of an id is its SHAPE, the decade its
#: kernel family; csrc/conv_tiles.h holds the same table and tests/test_conv_tiles_cpu.py holds the two together.
_SHAPES = {1: (128, 128), 2: (128, 64), 3: (64, 64), 4: (128, 128), 5: (128, 64), 6: (256, 128), 7: (256, 256),     # 4..7: 8 waves
           8: (32, 64),        # four 16 x 32 wave tiles on v_mfma_f32_16x16x4_f32: finer granularity for launches of a few rounds
           9: (64, 64)}        # hybrid launch: the rows that fill whole rounds on 64 x 64, the rest on 16-row wave tiles, one grid
Tile = collections.namedtuple("Tile", "shape family splitk persistent_of")      # shape: (BM, BN)
SPLIT3_PERSISTENT = {47: 43, 49: 46}
TILES = {base + s: Tile(_SHAPES[s], family, base in (30, 50), None)
         for family, base, shapes in (("igemm", 0, (1, 2, 3)),               # register staging
                                      ("dma", 10, range(1, 8)),              # LDS-DMA staging, pointer-addressed
                                      ("dma2", 20, range(1, 10)),            # buffer-addressed LDS-DMA, barrier inside the MFMA stream
                                      ("dma2", 30, (1, 2, 4, 5, 6, 7)),      # ... with the last round of tiles split along K
                                      ("split3", 40, (1, 2, 3, 4, 6)),       # fp32 operands as three bf16 pieces
                                      ("split3", 50, (1, 2, 4, 6)))          # ... split-K
         for s in shapes}
TILES.update({t: TILES[of]._replace(persistent_of=of) for t, of in SPLIT3_PERSISTENT.items()})
#: the activation-stationary split3 form of short-K 1x1 convs (csrc/conv_panel.hip): a block keeps 128 rows x K of split activations in
#: registers and walks all of Cout, 128 (71) or 64 (72) columns at a time
TILES.update({70 + s: Tile(_SHAPES[s], "split3", False, None) for s in (1, 2)})
#: split3 with pre-split ACTIVATIONS (csrc/conv_dma2.hip, A3): the forms of 46 / 49 whose input was written split by its producer's
#: epilogue (conv2d(out_split3=True)), so that their K loop has no splitting left to do
TILES.update({146: Tile(_SHAPES[6], "split3", False, None), 149: Tile(_SHAPES[6], "split3", False, 146)})
#: ... and the tiles of 146 / 149 with ONE activation stage for the three taps of a kernel row (csrc/conv_row3.hip): 3x3 / stride 1 /
#: pad == dil convs whose stage fits 288 rows (``_row3_ok``); 249: the persistent form of 246
TILES.update({246: Tile(_SHAPES[6], "split3", False, None), 249: Tile(_SHAPES[6], "split3", False, 246)})
#: ... and the form of 49 on a three-deep activation ring (csrc/conv_ring.hip): 1x1 convs without padding on fp32 activations with
#: K >= 128 (``_ring_ok``), whose activations are a pure HBM stream and get two K steps to land instead of half a step
TILES.update({349: Tile(_SHAPES[6], "split3", False, 46)})
_NO_TILE = Tile(None, None, False, None)        # an id outside the registry: the library refuses it


def tile_shape(t):
    """(BM, BN) of tile id ``t``; None for an id no entry point takes (pemp_conv2d_tile_shape)."""
    return TILES.get(t, _NO_TILE).shape


#: kernel variants the autotuner may pick on the fp32 chain: id -> (BM, BN), in the order they are timed.  All of them accumulate
#: in the same K order, so they are bit-identical and the choice only affects speed.  (29 runs as 23 where the geometry has no
#: hybrid split.)
TILE_VARIANTS = {t: TILES[t].shape for t in (13, 14, 12, 11, 15, 3, 17, 16, 23, 24, 22, 21, 25, 27, 26, 28, 29)}
#: the split3 family (pemp_hip.h: fp32 operands split into three bf16 pieces on v_mfma_f32_32x32x16_bf16, fp32 accuracy; the
#: shapes of 21..24 / 26): the variants of a layer that carries split weights (ConvParams.w3) -- bit-identical among themselves,
#: not to the fp32-chain ids above.  51..56: their split-K forms (EVAL_SPLITK).  47 / 49: persistent forms of 43 / 46 (a resident
#: grid that walks the tiles and overlaps one tile's epilogue with the next one's operand DMA; single convs only, no grouped form).
SPLIT3_TILES = (43, 42, 41, 44, 46, 47, 49)
SPLIT3_SPLITK_TILES = (51, 52, 54, 56)
SPLIT3_DEFAULT_TILE = 43
#: ... and their activation-stationary forms for 1x1 convs with Kpad <= 256 (bit-identical to the ids above): a registry of
#: their own, offered to timing-based picks only, where ``_panel_ok`` holds (PEMP_SPLIT3_PANEL=0: never, the A/B switch)
SPLIT3_PANEL_TILES = (71, 72)
SPLIT3_PANEL = os.environ.get("PEMP_SPLIT3_PANEL", "1") != "0"
#: ... and the forms that read pre-split activations (bit-identical to the ids above on the fp32 tensor): the only ids of a call
#: with ``x_split3``, and of no other call -- a registry and a pick key of their own.  PEMP_SPLIT3_PRESPLIT=0: the engines never
#: hand a tensor over pre-split (the A/B switch)
SPLIT3_PRESPLIT_TILES = (146, 149)
SPLIT3_PRESPLIT = os.environ.get("PEMP_SPLIT3_PRESPLIT", "1") != "0"
#: ... and the row-stage forms of 146 / 149 (bit-identical to them): a registry of its own, offered to timing-based picks only, where
#: ``_row3_ok`` holds (PEMP_SPLIT3_ROW3=0: never, the A/B switch)
SPLIT3_ROW3_TILES = (246, 249)
SPLIT3_ROW3 = os.environ.get("PEMP_SPLIT3_ROW3", "1") != "0"
ROW3_STAGE_ROWS = 288
#: ... and the three-deep activation ring of 49 for long-K 1x1 convs (bit-identical to the ids above): a registry of its own, offered
#: to timing-based picks only, where ``_ring_ok`` holds (PEMP_SPLIT3_RING=0: never, the A/B switch)
SPLIT3_RING_TILES = (349,)
SPLIT3_RING = os.environ.get("PEMP_SPLIT3_RING", "1") != "0"
RING_MIN_K = 128
AUTOTUNE = True
#: test hook: ``PICK_HOOK(kind, cands, key) -> one of cands`` decides every kernel-variant pick INSTEAD of timing (kind "conv":
#: tile ids, "wgrad": block counts / (tile kind, block count) pairs), at any problem size.  Timing-based picks differ from box
#: to box and the split-K / weight-gradient splits change the rounding: a whole-step parity test pins them (tests/conftest.py
#: ``pinned_picks``: AUTOTUNE off = one fixed variant per layer) or sweeps them through this hook.
PICK_HOOK = None
SPLITK = os.environ.get("PEMP_CONV_SPLITK", "1") != "0"     # the training convs may pick the split-K variants (A/B switch)
DEFAULT_TILE = 13
_TILE_CACHE = {}     # (layer geometry, input shape) -> fastest variant; shared by every ConvParams object
#: optional JSON file the picks are loaded from / saved to (PEMP_TILE_CACHE=path): a profiling run can then replay a
#: previous process' choices instead of timing the variants again under the profiler
_TILE_CACHE_FILE = os.environ.get("PEMP_TILE_CACHE")
WGRAD_PICKS = {}     # train_ops.conv_wgrad's per-shape picks ((tile kind, block count)); persisted in the same file
if _TILE_CACHE_FILE and os.path.exists(_TILE_CACHE_FILE):
    with open(_TILE_CACHE_FILE) as _f:
        for _k, _v in json.load(_f).items():
            _key = json.loads(_k)
            if _key and _key[0] == "wgrad":
                WGRAD_PICKS[tuple(_key[1:])] = tuple(_v) if isinstance(_v, list) else int(_v)
            else:
                _TILE_CACHE[tuple(_key)] = int(_v)


def save_picks():
    """Write the conv tile picks and the weight-gradient picks to PEMP_TILE_CACHE (no-op without it): a later process --
    a profiling run, or a training run that must reproduce this one bit for bit -- replays them instead of timing again."""
    if not _TILE_CACHE_FILE:
        return
    out = {json.dumps([int(v) for v in k]): t for k, t in _TILE_CACHE.items()}
    out.update({json.dumps(["wgrad"] + [int(v) for v in k]): (list(t) if isinstance(t, tuple) else t) for k, t in WGRAD_PICKS.items()})
    with open(_TILE_CACHE_FILE, "w") as f:
        json.dump(out, f)


def concurrent_stream(device, priority=0, tries=6, us=200):
    """A new HIP stream that really runs beside the CURRENT one.  The runtime deals streams round-robin to a few hardware queues
    (four by default): the n-th stream a process creates can land on the queue of the stream it is meant to overlap with, and
    the two then run one after the other (seen: the training step lost its two-stream overlap, 16.6 -> 17.8 ms, whenever
    three other streams had been created first).  Candidates are created until two idle kernels of ``us`` microseconds, one
    on each stream, finish in clearly less than 2 x ``us``; the last candidate is returned if none does."""
    lib = _lib.load()
    cur = torch.cuda.current_stream(device)
    _lib.check(lib.pemp_spin_us(1, C.c_void_p(cur.cuda_stream)), "pemp_spin_us")      # the kernel's first launch (code load) is not timed
    cur.synchronize()
    keep = []                                   # rejected candidates stay alive until the choice is made (no index reuse)
    for _ in range(tries):
        cand = torch.cuda.Stream(device=device, priority=priority)
        keep.append(cand)
        cand.wait_stream(cur)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(cur)
        _lib.check(lib.pemp_spin_us(us, C.c_void_p(cur.cuda_stream)), "pemp_spin_us")
        _lib.check(lib.pemp_spin_us(us, C.c_void_p(cand.cuda_stream)), "pemp_spin_us")
        cur.wait_stream(cand)
        e1.record(cur)
        e1.synchronize()
        if e0.elapsed_time(e1) * 1e3 < 1.6 * us:
            return cand
    return keep[-1]


def export_picks():
    """Everything the autotuners have decided so far, as one picklable object (see ``tuned_by_rank0``)."""
    return {"tiles": dict(_TILE_CACHE), "wgrad": dict(WGRAD_PICKS)}


def import_picks(picks):
    _TILE_CACHE.update(picks["tiles"])
    WGRAD_PICKS.update(picks["wgrad"])


def tuned_by_rank0(warm):
    """Run ``warm()`` -- one untimed step that meets every conv / weight-gradient shape of the job -- so that only RANK 0
    times kernel variants: it warms first, its picks are broadcast (one ``broadcast_object_list`` of a few KB), the other
    ranks then warm with every shape already in the cache.  All ranks run the same variants afterwards (the split-K and
    weight-gradient split choices change the rounding: data-parallel replicas should not differ in them), and N - 1 ranks do
    not spend their warm-up on timing runs.  One process / no process group: just ``warm()``."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        warm()
        return
    rank = dist.get_rank()
    if rank == 0:
        warm()
    box = [export_picks() if rank == 0 else None]
    dist.broadcast_object_list(box, src=0)
    if rank != 0:
        import_picks(box[0])
        warm()


def _tunes(rows, least=1024):
    """Whether a variant pick happens now: the autotuner on a problem worth timing, or the test hook (any size)."""
    return (PICK_HOOK is not None or (AUTOTUNE and rows >= least)) and not torch.cuda.is_current_stream_capturing()


def _fits(ids, *couts):
    """The ids of ``ids``, in order, whose tile width divides every one of ``couts``."""
    return [t for t in ids if all(c % _tile_bn(t) == 0 for c in couts)]


def _choose_tile(key, rows, launch, cands, default):
    """The variant of a call that names none: the remembered pick for ``key``; else, where a pick happens now (``_tunes(rows)``),
    one of ``cands()`` by ``_pick_tile``; else ``default`` (not remembered: a later call may still tune)."""
    tile = _TILE_CACHE.get(key)
    if tile is None:
        tile = _pick_tile(launch, key, cands()) if _tunes(rows) else default
    return tile


def _pick_tile(launch, key, cands):
    """Time the candidate variants for this (layer, input shape) and remember the fastest: two rounds over all
    candidates (the minimum of a variant's two timings counts: a round can be disturbed by whatever else the GPU is
    finishing), then a run-off between the best three with more repetitions."""
    if PICK_HOOK is not None:
        best = PICK_HOOK("conv", list(cands), key)
        if best not in cands:
            raise ValueError(f"PICK_HOOK returned {best!r}, not one of {cands}")
        _TILE_CACHE[key] = best
        return best

    def timed(t, reps):
        launch(t)                                   # warm
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            launch(t)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    ms = {t: timed(t, 3) for t in cands}
    for t in cands:
        ms[t] = min(ms[t], timed(t, 3))
    top = sorted(cands, key=lambda t: ms[t])[:3]
    final = {t: min(timed(t, 8), timed(t, 8)) for t in top}
    best = min(top, key=lambda t: final[t])
    _TILE_CACHE[key] = best
    save_picks()
    return best


def _tile_bn(t):
    """BN of tile id ``t``."""
    return TILES[t].shape[1]


def _panel_ok(p, n, ho, wo, ldx, ldy, ldr, h, w, pad_value, splitk, per_image_shift):
    """Whether the ids of SPLIT3_PANEL_TILES take this call (conv_panel.hip: conv_panel_supported)."""
    lim = 1 << 31
    return (SPLIT3_PANEL and PICK_HOOK is None and p.kh == 1 and p.kw == 1 and p.pad == 0 and p.kpad <= 256 and p.cin % 32 == 0
            and pad_value is None and not splitk and not per_image_shift and n * h * w * ldx * 4 < lim
            and n * ho * wo * max(ldy, ldr) * 4 < lim)


#: the split3 ids with a strided-residual form (``conv2d(residual_stride=2)``, PEMP_CONV_RES_S2): 43 for any layer and any M, and the
#: panel ids where the variant is instantiated (``res_s2_tiles``).  The persistent, split-K and pre-split ids refuse the flag
SPLIT3_RES_S2_TILES = (43, 72, 71)


def res_s2_tiles(p):
    """The tile ids that take ``conv2d(residual_stride=2)`` for layer ``p``, in the order they are timed: 43; 72 for 1x1 / pad 0
    layers of K = 64 or 128; 71 at K = 64 (its K = 128 form would spill).  () for a layer without split weights."""
    if p.w3 is None or p.stem:
        return ()
    panel = p.kh == 1 and p.kw == 1 and p.pad == 0
    return tuple(t for t in SPLIT3_RES_S2_TILES
                 if t == 43 or (panel and p.cout % _tile_bn(t) == 0 and (p.kpad == 64 or (p.kpad == 128 and t == 72))))


def row3_stage_rows(w, dil):
    """Stage rows a 256-row tile of csrc/conv_row3.hip can need on maps of width ``w``: 256 + 2 d pixels and d zero rows per image-row
    boundary inside them (row3_stage_rows there)."""
    return 256 + 2 * dil + dil * ((255 + 2 * dil + w - 1) // w)


def _row3_ok(p, w, residual, pad_value, out_split3, also_split3, per_image_shift):
    """Whether the ids of SPLIT3_ROW3_TILES take this call with a pre-split input (conv_row3.hip: conv_row3_supported)."""
    return (SPLIT3_ROW3 and (p.kh, p.kw, p.stride) == (3, 3, 1) and p.pad == p.dil and residual is None
            and pad_value is None and not out_split3 and also_split3 is None and not per_image_shift
            and row3_stage_rows(w, p.dil) <= ROW3_STAGE_ROWS)


def _ring_ok(p, x_split3, residual, pad_value, also_split3, splitk, res_s2=False):
    """Whether the id of SPLIT3_RING_TILES takes this call of a split3 layer (conv_ring.hip: conv_ring_supported): a 1x1 conv without
    padding on fp32 activations, K = Cin >= 128, Cout in whole 128-column tiles; the fp32 or the pre-split output; no residual, second
    output, padding value, split-K.  (The operand sizes are conv2d's ``s3`` rule, which every split3 call passes first.)"""
    return (SPLIT3_RING and PICK_HOOK is None and p.w3 is not None and not p.stem and (p.kh, p.kw, p.pad) == (1, 1, 0)
            and p.cin % 32 == 0 and p.kpad == p.cin and p.kpad >= RING_MIN_K and p.cout % 128 == 0 and not x_split3 and residual is None
            and pad_value is None and also_split3 is None and not splitk and not res_s2 and p.cout * p.kpad * 6 < 1 << 31)


def pack_split3(w):
    """KRSC [Cout, Kpad] fp32 (Kpad % 32 == 0) -> its split3 form (pemp_pack_split3_bf16): bf16 [Cout, Kpad / 32, 3, 32], per row
    and 32-channel K step the planes h, m, l with w == h + m + l exactly."""
    co, kpad = w.shape
    if w.dtype != torch.float32 or not w.is_contiguous() or kpad % 32:
        raise ValueError("pack_split3: a contiguous fp32 [Cout, Kpad] with Kpad % 32 == 0")
    out = torch.empty((co, kpad // 32, 3, 32), dtype=torch.bfloat16, device=w.device)
    _lib.check(_lib.load().pemp_pack_split3_bf16(_p(w), _p(out), co, kpad, _stream()), "pemp_pack_split3_bf16")
    return out


def hybrid_rows(n, ho, wo, cout):
    """Rows of an [n, ho, wo, cout] conv output that the hybrid launch (tile id 29) gives to the 64 x 64 tile; 0 = no split."""
    d = ConvDesc(n, ho, wo, 32, 32, ho, wo, cout, cout, 1, 1, 1, 0, 1, 0, 32, 0, 29)
    return int(_lib.load().pemp_conv2d_hybrid_rows(C.byref(d)))


def pack_conv_weight(w_oihw, stem4=False):
    """[Cout,Cin,KH,KW] -> KRSC [Cout, Kpad] (Cin contiguous).  STEM4: Cin padded to 4, row padded x32."""
    co, ci, kh, kw = w_oihw.shape
    w = w_oihw.detach().permute(0, 2, 3, 1).contiguous().float()     # [co,kh,kw,ci]
    if stem4:
        if ci > 4:
            raise ValueError("stem4 packing needs Cin <= 4")
        k = kh * kw * 4
        kpad = (k + 31) // 32 * 32
        out = torch.zeros(co, kpad, dtype=torch.float32, device=w.device)
        tmp = torch.zeros(co, kh, kw, 4, dtype=torch.float32, device=w.device)
        tmp[..., :ci] = w
        out[:, :k] = tmp.reshape(co, k)
        return out, kpad
    return w.reshape(co, kh * kw * ci), kh * kw * ci


def split3_shape(n, h, w, c):
    """Shape of the pre-split form of an [n, h, w, c] fp32 activation tensor: bf16, per pixel and 32-channel group the planes h, m, l."""
    return (n, h, w, c // 32, 3, 32)


def _split3_dims(t, name):
    if t.dim() != 6 or t.dtype != torch.bfloat16 or tuple(t.shape[4:]) != (3, 32) or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous bf16 [N, H, W, C / 32, 3, 32] pre-split tensor, got {tuple(t.shape)} {t.dtype} {t.stride()}")
    return tuple(t.shape[:3]) + (t.shape[3] * 32,)


def _conv_geom(who, x, p, out, residual, dtype=torch.float32, out_dtype=None, x_split3=False, out_split3=False, residual_stride=1):
    """What every conv wrapper checks of its tensors: x an NHWC view of the layer's channel count, ``out`` (allocated when None)
    and ``residual`` NHWC views of the output's shape.  ``x_split3`` / ``out_split3``: that tensor is in the pre-split form
    (``split3_shape``: dense, so its per-pixel stride is the channel count).  ``residual_stride`` 2: the residual is [n, Hr, Wr, cout]
    on a grid twice as fine, ho == (Hr - 1) // 2 + 1 and wo likewise.  -> (n, h, w, cin, ldx, ho, wo, out, ldy, ldr)"""
    if x_split3:
        n, h, w, cin = _split3_dims(x, "x")
        ldx = cin
    else:
        ldx = _nhwc(x, "x", dtype)
        n, h, w, cin = x.shape
    if cin != p.cin:
        raise ValueError(f"{who}: input has {cin} channels, layer expects {p.cin}")
    ho = conv_out_size(h, p.kh, p.stride, p.pad, p.dil)
    wo = conv_out_size(w, p.kw, p.stride, p.pad, p.dil)
    if out_split3:
        if p.cout % 32:
            raise ValueError(f"{who}: a pre-split output needs Cout % 32 == 0, got {p.cout}")
        if out is None:
            out = torch.empty(split3_shape(n, ho, wo, p.cout), dtype=torch.bfloat16, device=x.device)
        if _split3_dims(out, "out") != (n, ho, wo, p.cout):
            raise ValueError(f"{who}: out shape {tuple(out.shape)} != {split3_shape(n, ho, wo, p.cout)}")
        if residual is not None:
            raise ValueError(f"{who}: no residual with a pre-split output")
        return n, h, w, cin, ldx, ho, wo, out, p.cout, 0
    if out is None:
        out = torch.empty((n, ho, wo, p.cout), dtype=out_dtype or dtype, device=x.device)
    ldy = _nhwc(out, "out", out_dtype or dtype)
    if tuple(out.shape) != (n, ho, wo, p.cout):
        raise ValueError(f"{who}: out shape {tuple(out.shape)} != {(n, ho, wo, p.cout)}")
    ldr = 0
    if residual is not None:
        ldr = _nhwc(residual, "residual", dtype)
        if residual_stride == 2:
            rn, hr, wr, rc = residual.shape
            if (rn, rc) != (n, p.cout) or (hr - 1) // 2 + 1 != ho or (wr - 1) // 2 + 1 != wo:
                raise ValueError(f"{who}: a stride-2 residual of shape {tuple(residual.shape)} does not cover the output {tuple(out.shape)}")
        elif tuple(residual.shape) != tuple(out.shape):
            raise ValueError(f"{who}: residual shape mismatch")
    elif residual_stride != 1:
        raise ValueError(f"{who}: residual_stride without a residual")
    return n, h, w, cin, ldx, ho, wo, out, ldy, ldr


def conv2d(x, p, out=None, residual=None, shift_override=None, per_image_shift=False, relu=None, tile=0,
           pad_value=None, splitk=False, dropblock=None, out_split3=False, x_split3=False, also_split3=None, residual_stride=1):
    """y = act(scale * conv(x, w) + shift (+ residual)).  x: NHWC view, returns NHWC tensor/view ``out``.
    ``residual_stride`` 2: ``residual`` is [n, Hr, Wr, cout] on a grid twice as fine as the output (ho == (Hr - 1) // 2 + 1, wo
    likewise) and output pixel (i, j) adds its pixel (2 i, 2 j) -- bit-identical to the same id on ``residual[:, ::2, ::2]``, without
    the gather.  Split3 layers only, and only the ids of ``res_s2_tiles``; no pre-split operand, padding value, split-K or DropBlock.
    ``out_split3``: ``out`` is written PRE-SPLIT (bf16 ``split3_shape``: the split3 pieces of the fp32 result, for ONE reader that
    takes it with ``x_split3``); split3 layers only, no residual / split-K / DropBlock, never the panel ids.
    ``x_split3``: ``x`` is such a tensor (a ``pad_value`` then the same split of the [Cin] vector, bf16 [Cin / 32, 3, 32]); multi-tap
    split3 layers with Cout % 128 == 0 only, no per-image shift / split-K / DropBlock -- the ids of SPLIT3_PRESPLIT_TILES, bit-
    identical to the layer on the fp32 tensor.
    ``also_split3`` (a bf16 ``split3_shape`` tensor of the output's size): ``out`` is written as fp32 as usual AND the same values
    go to this tensor pre-split, for readers that take it with ``x_split3`` beside readers of the fp32 form; calls with ``x_split3``
    only (the ids of SPLIT3_PRESPLIT_TILES), no residual, not with ``out_split3``; the two outputs must not overlap.
    ``pad_value`` [Cin]: what out-of-image taps read instead of zero (multi-tap convs; see fold_input_affine).
    ``splitk``: the autotuner may also pick the split-K variants (training path: they are not bit-identical to the rest).
    ``dropblock`` (mask fp32 [N,Ho,Wo], kept count int32 [1]) -- a DropBlock2D record of train_ops.dropblock_mask: the layer's
    scaling of the output rows happens in the conv's epilogue (pemp_conv2d_dropblock_nhwc_f32; same arithmetic as
    train_ops.pixel_scale on the conv's result)."""
    if out_split3 or x_split3:       # what the library refuses for these forms (csrc/conv_igemm.hip: conv2d_impl)
        what = "a pre-split output" if out_split3 else "a pre-split input"
        if p.w3 is None or p.stem:
            raise ValueError(f"conv2d: {what} needs a split3 layer (ConvParams.w3), not the fp32 chain or a stem")
        if splitk or dropblock is not None:
            raise ValueError(f"conv2d: {what} has no split-K / DropBlock form")
        if out_split3 and tile and (tile not in SPLIT3_TILES + SPLIT3_PRESPLIT_TILES + SPLIT3_RING_TILES):
            raise ValueError(f"conv2d: a pre-split output needs an unsplit split3 tile id, got {tile}")
        if x_split3 and (p.kh * p.kw == 1 or per_image_shift or p.cin % 32 or p.cout % 128):
            raise ValueError("conv2d: a pre-split input needs a multi-tap conv with Cin % 32 == 0 and Cout % 128 == 0, no per-image shift")
    if also_split3 is not None and (not x_split3 or out_split3 or residual is not None):
        raise ValueError("conv2d: a second, pre-split output needs a pre-split input (x_split3), no out_split3, no residual")
    if (tile in SPLIT3_PRESPLIT_TILES + SPLIT3_ROW3_TILES) != bool(x_split3) and (tile or not x_split3):
        raise ValueError(f"conv2d: the tile ids {SPLIT3_PRESPLIT_TILES + SPLIT3_ROW3_TILES} and x_split3 come together (tile {tile})")
    res_s2 = residual_stride == 2
    if residual_stride not in (1, 2):
        raise ValueError(f"conv2d: residual_stride must be 1 or 2, got {residual_stride}")
    if res_s2:                       # what the library refuses for this form (csrc/conv_igemm.hip: conv2d_impl)
        if p.w3 is None or p.stem or x.dtype != torch.float32:
            raise ValueError("conv2d: a stride-2 residual needs a split3 layer (ConvParams.w3) on fp32 activations")
        if residual is None or out_split3 or x_split3 or also_split3 is not None or pad_value is not None or splitk or dropblock is not None:
            raise ValueError("conv2d: a stride-2 residual comes with a residual and without pre-split operands, padding value, split-K or DropBlock")
        if tile and tile not in res_s2_tiles(p):
            raise ValueError(f"conv2d: a stride-2 residual needs one of the tile ids {res_s2_tiles(p)} for this layer, got {tile}")
    if x.dtype == torch.bfloat16 and not x_split3:
        return _conv2d_bf16(x, p, out, residual, shift_override, per_image_shift, relu, tile, pad_value)
    n, h, w, cin, ldx, ho, wo, out, ldy, ldr = _conv_geom("conv2d", x, p, out, residual, x_split3=x_split3, out_split3=out_split3,
                                                          residual_stride=residual_stride)
    if also_split3 is not None and _split3_dims(also_split3, "also_split3") != (n, ho, wo, p.cout):
        raise ValueError(f"conv2d: also_split3 shape {tuple(also_split3.shape)} != {split3_shape(n, ho, wo, p.cout)}")
    lib = _lib.load()
    _chk_dev(x, p.w, out, residual, also_split3)
    if also_split3 is not None:
        residual = also_split3              # the library takes it in the residual slot (PEMP_CONV_OUT_SPLIT3_ALSO: never read)
    shift = p.shift if shift_override is None else shift_override
    if pad_value is not None:
        _chk_dev(pad_value)
        if x_split3:
            if tuple(pad_value.shape) != (cin // 32, 3, 32) or pad_value.dtype != torch.bfloat16 or not pad_value.is_contiguous():
                raise ValueError(f"conv2d: with x_split3, pad_value must be a contiguous bf16 [{cin // 32}, 3, 32] split vector")
        elif pad_value.numel() != cin or pad_value.dtype != torch.float32 or not pad_value.is_contiguous():
            raise ValueError(f"conv2d: pad_value must be a contiguous fp32 [{cin}] vector")
    flags = (CONV_OUT_SPLIT3 if out_split3 else 0) | (CONV_IN_SPLIT3 if x_split3 else 0) | (CONV_OUT_SPLIT3_ALSO if also_split3 is not None else 0)
    if (p.relu if relu is None else relu):
        flags |= CONV_RELU
    if per_image_shift:
        flags |= CONV_SHIFT_PER_IMAGE
    if p.stem:
        flags |= CONV_STEM4
    if res_s2:
        flags |= CONV_RES_S2 | (CONV_RES_HEVEN if residual.shape[1] % 2 == 0 else 0) | (CONV_RES_WEVEN if residual.shape[2] % 2 == 0 else 0)
    splitk = ((splitk and SPLITK) or (EVAL_SPLITK and n * ho * wo <= EVAL_SPLITK_MAX_ROWS)) and not p.stem \
        and not out_split3 and not x_split3 and not res_s2
    # split3: the layer carries split weights (inference engines; the layer's geometry decided it) and plain epilogue.  A call
    # outside the buffer-addressed kernels (an input of 2 GiB or more; a padding vector that does not sit far enough behind a
    # small map under a large dilation) runs the fp32 chain, whose pointer-addressed fall-back takes it
    if x_split3:
        s3 = _presplit_ok(x, p, pad_value)
    else:
        s3 = p.w3 is not None and dropblock is None and dma2_supported(x, p) and _group_member_ok(x, p, pad_value)
    if (out_split3 or x_split3) and not s3:
        raise ValueError("conv2d: pre-split activations need a geometry of the buffer-addressed kernels (<= 32 taps, operands < 2 GiB, "
                         "a padding value behind the activations)")
    if res_s2 and not (s3 and residual.numel() // p.cout * ldr < 1 << 31):
        raise ValueError("conv2d: a stride-2 residual needs a geometry of the buffer-addressed kernels and a residual below 2^31 elements")

    if dropblock is not None:
        dmask, dcnt = dropblock
        _chk_dev(dmask, dcnt)
        if (pad_value is not None or p.stem or dmask.dtype != torch.float32 or not dmask.is_contiguous() or dmask.numel() != n * ho * wo
                or dcnt.dtype != torch.int32 or not dma2_supported(x, p)):
            # outside the buffer-addressed kernels: conv, then the layer's own pass
            from . import train_ops
            y = conv2d(x, p, out=out, residual=residual, shift_override=shift_override, per_image_shift=per_image_shift, relu=relu,
                       tile=tile, pad_value=pad_value, splitk=splitk)
            return train_ops.pixel_scale(y, dmask, dcnt, out=y)

    def launch(t):
        d = ConvDesc(n, h, w, cin, ldx, ho, wo, p.cout, ldy, p.kh, p.kw, p.stride, p.pad, p.dil, ldr, p.kpad, flags, t)
        tl = TILES.get(t, _NO_TILE)
        pw, sk = p.w3 if tl.family == "split3" else p.w, tl.splitk
        if dropblock is not None:
            ws, ws_bytes = _splitk_ws(lib, d, x.device) if sk else (None, 0)
            _check_sk(lib, lib.pemp_conv2d_dropblock_nhwc_f32(C.byref(d), _p(x), _p(pw), _p(out), _p(p.scale), _p(shift), _p(residual),
                                                              _p(dropblock[0]), _p(dropblock[1]), C.c_void_p(ws), ws_bytes, _stream()),
                      ws, "pemp_conv2d_dropblock_nhwc_f32")
            return
        if sk and pad_value is not None:
            ws, ws_bytes = _splitk_ws(lib, d, x.device)
            _check_sk(lib, lib.pemp_conv2d_padv_splitk_nhwc_f32(C.byref(d), _p(x), _p(pw), _p(out), _p(p.scale), _p(shift), _p(residual),
                                                                _p(pad_value), C.c_void_p(ws), ws_bytes, _stream()), ws,
                      "pemp_conv2d_padv_splitk_nhwc_f32")
        elif sk:
            ws, ws_bytes = _splitk_ws(lib, d, x.device)
            _check_sk(lib, lib.pemp_conv2d_splitk_nhwc_f32(C.byref(d), _p(x), _p(pw), _p(out), _p(p.scale), _p(shift), _p(residual),
                                                           C.c_void_p(ws), ws_bytes, _stream()), ws, "pemp_conv2d_splitk_nhwc_f32")
        elif pad_value is None:
            _lib.check(lib.pemp_conv2d_nhwc_f32(C.byref(d), _p(x), _p(pw), _p(out), _p(p.scale), _p(shift),
                                                _p(residual), _stream()), "pemp_conv2d_nhwc_f32")
        else:
            _lib.check(lib.pemp_conv2d_padv_nhwc_f32(C.byref(d), _p(x), _p(pw), _p(out), _p(p.scale), _p(shift),
                                                     _p(residual), _p(pad_value), _stream()), "pemp_conv2d_padv_nhwc_f32")

    if tile == 0:
        key = (p.cin, p.cout, p.kh, p.kw, p.stride, p.pad, p.dil, (6 if dropblock is not None else 4) if splitk else int(p.stem) + (7 if dropblock is not None else 0),
               n, h, w, int(residual is not None and also_split3 is None), int(pad_value is not None)) + ((3,) if s3 else ())    # 3: split3 picks
        if x_split3 or out_split3:
            # keys of their own: a pick made on the fp32 tensor is never replayed on the split one, nor the reverse
            # (a pre-split output: 17 where it was 16 -- the persistent ids 47 / 49 / 149 run producer kernels of their own now and are
            # offered; a pick remembered under 16 was made without them and is not replayed.  64: with the second output)
            key += (146,) * int(x_split3) + (17,) * int(out_split3) + (64,) * int(also_split3 is not None)
            # ... and a call that the row-stage id takes under a key of its own (246): an older pick, made without that candidate, is
            # never replayed on it.  The id is offered to timing-based picks only (the test hook decides among the other ids)
            row3 = bool(x_split3) and _row3_ok(p, w, residual, pad_value, out_split3, also_split3, per_image_shift)
            if row3:
                key += (246,)
            # ... and a producer call that the ring id takes, likewise (349; ``_ring_ok`` is false under the hook)
            ring = _ring_ok(p, x_split3, residual, pad_value, also_split3, splitk)
            if ring:
                key += (349,)
            cands = lambda: _fits(list(SPLIT3_PRESPLIT_TILES if x_split3 else SPLIT3_TILES) +
                                  (list(SPLIT3_ROW3_TILES) if row3 and PICK_HOOK is None else []) +
                                  (list(SPLIT3_RING_TILES) if ring else []), p.cout)
        elif res_s2:
            # a key of its own (128): a pick made with a dense residual is never replayed on the strided one, nor the reverse.  Only
            # the ids that take the flag are offered; the panel ones under their usual rule (and the residual's own extent < 2 GiB)
            panel = _panel_ok(p, n, ho, wo, ldx, ldy, ldr, h, w, pad_value, splitk, per_image_shift) \
                and residual.numel() // p.cout * ldr * 4 < 1 << 31
            key += (128,) + ((71,) if panel else ())
            cands = lambda: _fits([t for t in res_s2_tiles(p) if panel or t not in SPLIT3_PANEL_TILES], p.cout)
        elif s3:
            # a pick among candidates that include the panel ids is remembered under a key of its own (71): a call of the same
            # geometry that they do not take (a per-image shift, operands of 2 GiB) must never replay it
            panel = _panel_ok(p, n, ho, wo, ldx, ldy, ldr, h, w, pad_value, splitk, per_image_shift)
            # ... and the ring id under a suffix of its own (349), in front of the panel one: an older pick is never replayed on the new
            # candidate set, and a pick that includes the id never on a call that the id refuses (a residual, a padding value)
            ring = _ring_ok(p, x_split3, residual, pad_value, also_split3, splitk)
            if ring:
                key += (349,)
            if panel:
                key += (71,)
            cands = lambda: _fits(list(SPLIT3_TILES) + (list(SPLIT3_SPLITK_TILES) if splitk else []) +
                                  (list(SPLIT3_RING_TILES) if ring else []) + (list(SPLIT3_PANEL_TILES) if panel else []), p.cout)
        else:
            def cands():
                ids = list(GROUP_TILES if dropblock is not None else TILE_VARIANTS) + (list(SPLITK_TILES) if splitk else [])
                if 29 in ids and not (hybrid_rows(n, ho, wo, p.cout) and dma2_supported(x, p)):
                    ids.remove(29)         # no hybrid launch for this geometry / layer: id 29 would run as 23 (or 13)
                return _fits(ids, p.cout)
        tile = _choose_tile(key, n * ho * wo, launch, cands,
                            SPLIT3_PRESPLIT_TILES[0] if x_split3 else SPLIT3_DEFAULT_TILE if s3 else DEFAULT_TILE + (10 if dropblock is not None else 0))
    launch(tile)
    return out


def stem_pool_supported(p):
    """Whether ``p`` is a stem the fused launch of ``stem_pool`` takes: 7x7 / stride 2 / pad 3 on NHWC4 with split weights."""
    return (p.stem and p.w3pool is not None and (p.kh, p.kw, p.stride, p.pad, p.dil) == (7, 7, 2, 3, 1) and p.kpad == 224
            and p.cout % 64 == 0)


def stem_pool(x, p, out=None):
    """max_pool2d(act(scale * conv(x, w) + shift), 3, stride 2, pad 1, ceil_mode) of the 7x7 / 2 / 3 NHWC4 stem in ONE launch
    (pemp_conv2d_nhwc_f32 with CONV_POOL3S2; split3 arithmetic on ``p.w3pool``): the conv's own output is never written.  x: NHWC4;
    returns the pooled NHWC tensor / view ``out`` (a channel window of a wider buffer is fine)."""
    lib = _lib.load()
    if not stem_pool_supported(p):
        raise ValueError("stem_pool: a 7x7 / stride 2 / pad 3 NHWC4 stem with split weights (ConvParams.w3pool)")
    _chk_dev(x, p.w3pool, out)
    ldx = _nhwc(x, "x")
    n, h, w, cin = x.shape
    if cin != p.cin or x.dtype != torch.float32:
        raise ValueError(f"stem_pool: fp32 NHWC4 input expected, got {cin} channels of {x.dtype}")
    ho, wo = conv_out_size(h, 7, 2, 3, 1), conv_out_size(w, 7, 2, 3, 1)
    hp, wp = _pool_out(ho, 3, 2, 1, True), _pool_out(wo, 3, 2, 1, True)
    if out is None:
        out = torch.empty((n, hp, wp, p.cout), dtype=torch.float32, device=x.device)
    ldy = _nhwc(out, "out")
    if tuple(out.shape) != (n, hp, wp, p.cout) or out.dtype != torch.float32:
        raise ValueError(f"stem_pool: out shape {tuple(out.shape)} != {(n, hp, wp, p.cout)} (fp32)")
    flags = CONV_STEM4 | CONV_POOL3S2 | (CONV_RELU if p.relu else 0)
    d = ConvDesc(n, h, w, cin, ldx, ho, wo, p.cout, ldy, 7, 7, 2, 3, 1, 0, p.kpad, flags, SPLIT3_DEFAULT_TILE)
    _lib.check(lib.pemp_conv2d_nhwc_f32(C.byref(d), _p(x), _p(p.w3pool), _p(out), _p(p.scale), _p(p.shift), None, _stream()),
               "pemp_conv2d_nhwc_f32")
    return out


def _conv2d_bf16(x, p, out, residual, shift_override, per_image_shift, relu, tile, pad_value):
    """The bf16-operand variant of ``conv2d`` (pemp_conv2d_bf16_nhwc; the side figure of bench.py, never the default path): x,
    p.w, residual and pad_value are bf16, accumulation is fp32, ``out`` is bf16 -- or fp32 when an fp32 ``out`` is given (the
    encoder's last layer)."""
    lib = _lib.load()
    _chk_dev(x, p.w, out, residual, pad_value)
    if p.w.dtype != torch.bfloat16 or p.stem:
        raise ValueError("conv2d (bf16 input): the layer's weights must be packed as bf16 (engine precision 'bf16'); no stem")
    n, h, w, cin, ldx, ho, wo, out, ldy, ldr = _conv_geom("conv2d", x, p, out, residual, torch.bfloat16,
                                                          None if out is None else out.dtype)
    out_f32 = out.dtype == torch.float32
    if pad_value is not None and (pad_value.numel() != cin or pad_value.dtype != torch.bfloat16 or not pad_value.is_contiguous()):
        raise ValueError(f"conv2d: pad_value must be a contiguous bf16 [{cin}] vector")
    shift = p.shift if shift_override is None else shift_override
    flags = (CONV_RELU if (p.relu if relu is None else relu) else 0) | (CONV_SHIFT_PER_IMAGE if per_image_shift else 0)

    def launch(t):
        d = ConvDesc(n, h, w, cin, ldx, ho, wo, p.cout, ldy, p.kh, p.kw, p.stride, p.pad, p.dil, ldr, p.kpad, flags, t)
        _lib.check(lib.pemp_conv2d_bf16_nhwc(C.byref(d), _p(x), _p(p.w), _p(out), _p(p.scale), _p(shift), _p(residual), _p(pad_value),
                                             1 if out_f32 else 0, _stream()), "pemp_conv2d_bf16_nhwc")

    if tile == 0:
        key = (p.cin, p.cout, p.kh, p.kw, p.stride, p.pad, p.dil, 5, n, h, w, int(residual is not None), int(pad_value is not None))   # 5: bf16
        tile = _choose_tile(key, n * ho * wo, launch, lambda: _fits(GROUP_TILES, p.cout), 24 if p.cout % 128 == 0 else 23)
    launch(tile)
    return out


def convert(x, out):
    """Element-wise fp32 -> bf16 (round to nearest even) or bf16 -> fp32 between two contiguous tensors of one shape."""
    lib = _lib.load()
    _chk_dev(x, out)
    if not x.is_contiguous() or not out.is_contiguous() or x.numel() != out.numel() or x.numel() % 4:
        raise ValueError("convert: contiguous tensors of the same size (a multiple of 4 elements)")
    if x.dtype == torch.float32 and out.dtype == torch.bfloat16:
        _lib.check(lib.pemp_convert_f32_bf16(_p(x), _p(out), x.numel(), _stream()), "convert_f32_bf16")
    elif x.dtype == torch.bfloat16 and out.dtype == torch.float32:
        _lib.check(lib.pemp_convert_bf16_f32(_p(x), _p(out), x.numel(), _stream()), "convert_bf16_f32")
    else:
        raise ValueError(f"convert: {x.dtype} -> {out.dtype} is not one of fp32 <-> bf16")
    return out


#: tile variants a grouped launch may use (conv_dma2.hip only)
GROUP_TILES = (23, 22, 25, 21, 24, 26, 27)
GROUP_MAX = 4


def _group_member_ok(x, p, pad_value):
    """What conv_dma2_supported (csrc/conv_dma2.hip) checks for one member of a grouped launch."""
    n, h, w, _ = x.shape
    ldx = _nhwc(x, "x")
    taps = p.kh * p.kw
    tapmax = (p.dil * (p.kh - 1) * w + p.dil * (p.kw - 1)) * ldx * 4
    xbytes = (n * h * w + p.pad * w + p.pad) * ldx * 4 + tapmax
    if p.stem or taps > 32 or xbytes >= 2 ** 31 or p.w.numel() * 4 >= 2 ** 31:
        return False
    if pad_value is not None:
        off = pad_value.data_ptr() - x.data_ptr()
        d = off + (p.pad * w + p.pad) * ldx * 4
        if off < n * h * w * ldx * 4 or d < tapmax or d + p.cin * 4 >= 2 ** 31:
            return False
    return True


def _presplit_ok(x, p, pad_value):
    """conv_dma2_supported for a pre-split input (6 bytes per element; ``pad_value`` the split vector)."""
    n, h, w = x.shape[:3]
    row = p.cin * 6
    tapmax = (p.dil * (p.kh - 1) * w + p.dil * (p.kw - 1)) * row
    if p.kh * p.kw > 32 or (n * h * w + p.pad * w + p.pad) * row + tapmax >= 2 ** 31 or p.w3.numel() * 2 >= 2 ** 31:
        return False
    if pad_value is not None:
        off = pad_value.data_ptr() - x.data_ptr()
        d = off + (p.pad * w + p.pad) * row
        if off < n * h * w * row or d < tapmax or d + row >= 2 ** 31:
            return False
    return True


def conv2d_group(xs, ps, outs, pad_values=None, residuals=None, tile=0):
    """Up to four INDEPENDENT convs in one launch (pemp_conv2d_group_nhwc_f32): member i computes ``outs[i] = act(scale *
    conv(xs[i], ps[i].w) + shift (+ residuals[i]))`` exactly as ``conv2d`` would -- bit-identical -- but the members' tiles share
    one grid.  ``pad_values``: per member or None (all or none).  The tile variant is timed once per group signature."""
    lib = _lib.load()
    n = len(ps)
    if not 1 <= n <= GROUP_MAX or len(xs) != n or len(outs) != n:
        raise ValueError(f"conv2d_group: 1..{GROUP_MAX} members with one input and one output each")
    pad_values = list(pad_values) if pad_values is not None else [None] * n
    residuals = list(residuals) if residuals is not None else [None] * n
    descs, keys = [], []
    for x, p, out, pv, res in zip(xs, ps, outs, pad_values, residuals):
        _chk_dev(x, p.w, out, pv, res)
        if p.stem:
            raise ValueError("conv2d_group: no stem convs")
        if out is None:
            raise ValueError("conv2d_group: every member needs its output")
        nb, h, w, cin, ldx, ho, wo, out, ldy, ldr = _conv_geom("conv2d_group", x, p, out, res)
        descs.append((nb, h, w, cin, ldx, ho, wo, p.cout, ldy, p.kh, p.kw, p.stride, p.pad, p.dil, ldr, p.kpad, CONV_RELU if p.relu else 0))
        keys += [p.cin, p.cout, p.kh, p.stride, p.pad, p.dil, nb, h, w, int(res is not None), int(pv is not None)]
    s3 = all(p.w3 is not None for p in ps)
    if not all(_group_member_ok(x, p, pv) for x, p, pv in zip(xs, ps, pad_values)) or (not s3 and any(p.w3 is not None for p in ps)):
        # a member outside the buffer-addressed kernels (tiny maps under a large dilation: the padding vector is not far enough
        # behind the activations; 2 GiB operands; > 32 taps), or members of both the split3 and the fp32-chain family: every member
        # through its own launch -- same results
        for x, p, out, pv, res in zip(xs, ps, outs, pad_values, residuals):
            conv2d(x, p, out=out, residual=res, pad_value=pv if p.kh * p.kw > 1 else None)
        return outs
    arr = lambda ts: (C.c_void_p * n)(*[(t.data_ptr() if t is not None else None) for t in ts])
    xa, wa, ya = arr(xs), arr([p.w3 if s3 else p.w for p in ps]), arr(outs)
    sa, ha, ra, pa = arr([p.scale for p in ps]), arr([p.shift for p in ps]), arr(residuals), arr(pad_values)
    ptr = lambda a: C.cast(a, C.POINTER(C.c_void_p))

    def launch(t):
        da = (ConvDesc * n)(*[ConvDesc(*d, t) for d in descs])
        _lib.check(lib.pemp_conv2d_group_nhwc_f32(n, da, ptr(xa), ptr(wa), ptr(ya), ptr(sa), ptr(ha), ptr(ra), ptr(pa), _stream()),
                   "pemp_conv2d_group_nhwc_f32")

    if tile == 0:
        key = (-8 if s3 else -7,) + tuple(keys)     # -7: a grouped launch, -8: of the split3 family (the cache file stores keys as integer lists)
        couts = [p.cout for p in ps]
        if s3:
            cands = lambda: _fits([t for t in SPLIT3_TILES if t not in SPLIT3_PERSISTENT], *couts)
        else:
            cands = lambda: _fits(GROUP_TILES + (28,), *couts)
        tile = _choose_tile(key, max(d[0] * d[5] * d[6] for d in descs), launch, cands, SPLIT3_DEFAULT_TILE if s3 else DEFAULT_TILE + 10)
    launch(tile)
    return outs


#: split-K variants (ids 31..37 = the shapes of 21..27; pemp_hip.h): NOT bit-identical to the others.  The training convs may pick
#: them, and so may the evaluation path for SMALL row counts (one or two episodes per step: 5202 rows leave two thirds of the
#: chip idle on the 3x3 layers otherwise) -- see EVAL_SPLITK
SPLITK_TILES = (31, 32, 34, 35, 36, 37)
#: evaluation convs of at most EVAL_SPLITK_MAX_ROWS output rows may use the split-K variants.  OFF by default: every evaluation
#: variant is then bit-identical, a one-episode step equals the batched step bit for bit, and metrics cannot differ between
#: processes or ranks through the (timing-based) variant pick.  ON (PEMP_EVAL_SPLITK=1, ``with ops.eval_splitk():``,
#: ``Evaluator(splitk=True)``): one-episode steps are ~1.15x faster and agree with the exact path to rounding
#: (tests/test_eval_protocol_gpu.py states the bounds); the split-K hand-off uses device-scope write-through stores and sc1 loads
#: (csrc/conv_dma2.hip), not the fence pair of the HIP memory model.  Multi-rank jobs broadcast rank 0's picks (tuned_by_rank0).
EVAL_SPLITK = os.environ.get("PEMP_EVAL_SPLITK", "0") == "1"
EVAL_SPLITK_MAX_ROWS = int(os.environ.get("PEMP_EVAL_SPLITK_MAX_ROWS", "12000"))
#: Uncached split-K workspaces, one per (device, scope).  A workspace must never serve two launches that can run beside each
#: other, so everything that runs on its own stream has its own SCOPE: 0 = the main chain (training step, evaluation engine),
#: k = evaluation lane k (networks._HeadMixin.lane sets SK_SCOPE).  The size is fixed (every variant fits) and a workspace is
#: never freed or moved: captured hipGraphs hold its address.
_SK_WS = {}
SK_SCOPE = 0
_SK_WS_BYTES = 72 << 20            # 256 partial tiles of 256 x 256 floats + counters


class eval_splitk:
    """``with ops.eval_splitk(True):`` -- evaluation convs issued (or recorded into a hipGraph) inside the block may use the
    split-K variants for small row counts; restores the previous setting on exit."""

    def __init__(self, on=True):
        self.on = bool(on)

    def __enter__(self):
        global EVAL_SPLITK
        self.prev, EVAL_SPLITK = EVAL_SPLITK, self.on
        return self

    def __exit__(self, *exc):
        global EVAL_SPLITK
        EVAL_SPLITK = self.prev
        return False


def _splitk_ws(lib, desc, device):
    """-> (pointer, bytes) of the uncached workspace (pemp_uncached_alloc) of this device and the current scope."""
    need = lib.pemp_conv2d_splitk_workspace_bytes(C.byref(desc))
    if need == 0:
        return None, 0
    if need > _SK_WS_BYTES:
        raise RuntimeError(f"conv split-K: a launch asks for {need} bytes of workspace, the fixed size is {_SK_WS_BYTES}")
    idx = device.index if device.index is not None else torch.cuda.current_device()
    ent = _SK_WS.get((idx, SK_SCOPE))
    if ent is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the conv split-K workspace must exist before a hipGraph is recorded: run the step eagerly once")
        with torch.cuda.device(device):
            ptr = lib.pemp_uncached_alloc(_SK_WS_BYTES)
        if not ptr:
            _lib.check(-1, "pemp_uncached_alloc")
        ent = _SK_WS[(idx, SK_SCOPE)] = (ptr, _SK_WS_BYTES)
    return ent


def _check_sk(lib, rc, ws, what):
    """A split-K launch that failed may have left arrival counters non-zero (no block would ever be "last" again): clear
    them before the failure is raised."""
    if rc and ws:
        lib.pemp_splitk_reset(C.c_void_p(ws), _stream())
    _lib.check(rc, what)


def _stats_rows(m, tile):
    """Partial rows the stats / bnbwd epilogues of variant ``tile`` write: one per row tile (pemp_conv2d_stats_rows)."""
    bm = TILES[tile].shape[0]
    return (m + bm - 1) // bm


def _train_tiles(cout):
    """What the statistics / BatchNorm-backward convs may pick for ``cout`` channels, split-K forms included."""
    return _fits(list(range(21, 28)) + list(SPLITK_TILES), cout)


def _stats_launch(lib, fn, what, desc, x, *operands):
    """launch(t) of a statistics-epilogue entry ``fn(desc(t), operands..., ws, ws_bytes, stream)``."""
    def launch(t):
        d = ConvDesc(*desc, t)
        ws, ws_bytes = _splitk_ws(lib, d, x.device) if TILES.get(t, _NO_TILE).splitk else (None, 0)
        _check_sk(lib, fn(C.byref(d), *operands, C.c_void_p(ws), ws_bytes, _stream()), ws, what)
    return launch


#: the split3 ids that have a statistics epilogue (pemp_split3_conv2d_stats_nhwc_f32): the unsplit ids on their own wave grids.
#: No persistent, panel, pre-split or split-K form; the library's rows query is the authority (``split3_stats_tiles``).
SPLIT3_STATS_TILES = (43, 42, 41, 44, 46)


@functools.lru_cache(maxsize=None)
def _split3_stats_offered():
    lib = _lib.load()
    d = lambda t: ConvDesc(1, 8, 8, 32, 32, 8, 8, 256, 256, 1, 1, 1, 0, 1, 0, 32, 0, t)
    return tuple(t for t in SPLIT3_STATS_TILES if lib.pemp_conv2d_stats_split3_rows(C.byref(d(t))) > 0)


def split3_stats_tiles(cout):
    """The ids of SPLIT3_STATS_TILES the library offers (pemp_conv2d_stats_split3_rows answers for them) whose BN divides ``cout``."""
    return _fits(_split3_stats_offered(), cout)


def _conv2d_stats_split3(x, p, out, tile):
    """conv2d_stats for a layer that carries split weights (ConvParams.w3): pemp_split3_conv2d_stats_nhwc_f32."""
    lib = _lib.load()
    _chk_dev(x, p.w3, out)
    n, h, w, cin, ldx, ho, wo, out, ldy, _ = _conv_geom("conv2d_stats", x, p, out, None)
    m = n * ho * wo
    part = torch.empty(((m + 63) // 64, 2, p.cout), dtype=torch.float32, device=x.device)     # the smallest row tile has 64 rows
    desc = lambda t: ConvDesc(n, h, w, cin, ldx, ho, wo, p.cout, ldy, p.kh, p.kw, p.stride, p.pad, p.dil, 0, p.kpad, 0, t)

    def launch(t):
        _lib.check(lib.pemp_split3_conv2d_stats_nhwc_f32(C.byref(desc(t)), _p(x), _p(p.w3), _p(out), _p(part), _stream()),
                   "pemp_split3_conv2d_stats_nhwc_f32")

    if tile == 0:
        # a key of its own: 2 = the stats epilogue, the trailing 3 = on the split3 family -- never the key of an fp32 statistics
        # pick (no trailing 3) nor of a plain split3 pick (0 / 4 / 6 / 7 where this one has 2)
        key = (p.cin, p.cout, p.kh, p.kw, p.stride, p.pad, p.dil, 2, n, h, w, 0, 0, 3)
        tile = _choose_tile(key, m, launch, lambda: split3_stats_tiles(p.cout), SPLIT3_DEFAULT_TILE)
    launch(tile)
    return out, part[:int(lib.pemp_conv2d_stats_split3_rows(C.byref(desc(tile))))]


def conv2d_stats(x, p, out=None, tile=0):
    """z = conv(x, w) with the per-32-row partial sums of z and z^2 left by the epilogue (pemp_conv2d_stats_nhwc_f32):
    -> (z, partials [row tiles of the chosen variant, 2, Cout]).  Raises PempHipError where the buffer-addressed kernels do not apply
    (callers then use conv2d + bn_stats); ``stats_supported`` says so beforehand.
    A layer with split weights (``p.w3``) runs the split3 form (pemp_split3_conv2d_stats_nhwc_f32; ids of SPLIT3_STATS_TILES): z is
    then bit-identical to ``conv2d(x, p, tile=id)`` of the same id, not to the fp32 chain."""
    if p.w3 is not None and not p.stem and p.scale is None:
        return _conv2d_stats_split3(x, p, out, tile)
    lib = _lib.load()
    _chk_dev(x, p.w, out)
    n, h, w, cin, ldx, ho, wo, out, ldy, _ = _conv_geom("conv2d_stats", x, p, out, None)
    if p.stem or p.scale is not None:
        raise ValueError("conv2d_stats: plain (non-stem, unscaled) convs only")
    m = n * ho * wo
    part = torch.empty(((m + 63) // 64, 2, p.cout), dtype=torch.float32, device=x.device)     # the smallest row tile has 64 rows
    launch = _stats_launch(lib, lib.pemp_conv2d_stats_nhwc_f32, "pemp_conv2d_stats_nhwc_f32",
                           (n, h, w, cin, ldx, ho, wo, p.cout, ldy, p.kh, p.kw, p.stride, p.pad, p.dil, 0, p.kpad, 0),
                           x, _p(x), _p(p.w), _p(out), _p(part))
    if tile == 0:
        key = (p.cin, p.cout, p.kh, p.kw, p.stride, p.pad, p.dil, 2, n, h, w, 0, 0)     # 2: the stats epilogue
        tile = _choose_tile(key, m, launch, lambda: _train_tiles(p.cout) if SPLITK else _fits(range(21, 28), p.cout), DEFAULT_TILE + 10)
    launch(tile)
    return out, part[:_stats_rows(m, tile)]


def conv2d_bnbwd(x, p, bn, residual=None, out=None, tile=0):
    """g = mask(conv(x, w) + residual) -- the gradient at the output of a train-mode BatchNorm(+ReLU), masked by that
    BatchNorm's ReLU -- with the per-32-row partial sums of g and g * xhat left by the epilogue
    (pemp_conv2d_bnbwd_nhwc_f32).  ``bn``: dict with z (the BatchNorm's input, NHWC like the result), mean, invstd and
    mask (int32 [M, C/32] sign bits from train_ops.bn_apply, or None for a BatchNorm without ReLU).
    -> (g, partials [row tiles of the chosen variant, 2, Cout])."""
    lib = _lib.load()
    z, mask = bn["z"], bn.get("mask")
    _chk_dev(x, p.w, out, residual, z, mask, bn["mean"], bn["invstd"])
    n, h, w, cin, ldx, ho, wo, out, ldy, ldr = _conv_geom("conv2d_bnbwd", x, p, out, residual)
    if p.stem or p.scale is not None or p.shift is not None:
        raise ValueError("conv2d_bnbwd: plain (non-stem, no affine) convs only")
    if tuple(z.shape) != tuple(out.shape):
        raise ValueError(f"conv2d_bnbwd: the BatchNorm input is {tuple(z.shape)}, the gradient {tuple(out.shape)}")
    ldz = _nhwc(z, "z")
    m = n * ho * wo
    if mask is not None and (mask.dtype != torch.int32 or not mask.is_contiguous() or mask.numel() != m * (p.cout // 32)):
        raise ValueError("conv2d_bnbwd: mask must be a contiguous int32 [M, Cout/32] tensor")
    part = torch.empty(((m + 63) // 64, 2, p.cout), dtype=torch.float32, device=x.device)
    launch = _stats_launch(lib, lib.pemp_conv2d_bnbwd_nhwc_f32, "pemp_conv2d_bnbwd_nhwc_f32",
                           (n, h, w, cin, ldx, ho, wo, p.cout, ldy, p.kh, p.kw, p.stride, p.pad, p.dil, ldr, p.kpad, 0),
                           x, _p(x), _p(p.w), _p(out), _p(residual), _p(mask), _p(z), ldz, _p(bn["mean"]), _p(bn["invstd"]), _p(part))
    if tile == 0:
        key = (p.cin, p.cout, p.kh, p.kw, p.stride, p.pad, p.dil, 3, n, h, w, int(residual is not None), 0)   # 3: this epilogue
        tile = _choose_tile(key, m, launch, lambda: _train_tiles(p.cout) if SPLITK else _fits(range(21, 28), p.cout), DEFAULT_TILE + 10)
    launch(tile)
    return out, part[:_stats_rows(m, tile)]


def dma2_supported(x, p):
    """Whether the buffer-addressed conv kernels apply to this (input, layer): what conv_dma2_supported checks in
    csrc/conv_dma2.hip (no padding value involved)."""
    n, h, w, cin = x.shape
    return (not p.stem and p.kh * p.kw <= 32 and cin % 32 == 0 and p.cout % 64 == 0
            and x.numel() * 4 < 2 ** 31 - (1 << 20) and p.w.numel() * 4 < 2 ** 31)


def stats_supported(x, p):
    """Whether conv2d_stats applies to this (input, layer) -- for a layer with split weights (``p.w3``): whether its split3 form
    does (the split weights below 2 GiB as well, and an id offered for the layer's Cout)."""
    if p.scale is not None or not dma2_supported(x, p):
        return False
    return p.w3 is None or (p.w3.numel() * 2 < 2 ** 31 and bool(split3_stats_tiles(p.cout)))


def fold_input_affine(p, s, t):
    """Fold a per-input-channel affine x -> s*x + t that sits IN FRONT of the (zero-padded) conv ``p`` into the conv
    itself (ASPPV2: BatchNorm before the dilated convs, networks/backbones.py:330-357).  Returns (ConvParams, pad_value):
    conv_W(s*x + t, pad 0) = conv_{W*s}(x, pad -t/s) + sum_taps W t, so out-of-image taps must read -t/s -- the value
    that is 0 in the affine's output space.  Needs s != 0 (returns None otherwise) and no output scale on ``p``."""
    if p.stem or p.scale is not None or bool((s == 0).any()) or not bool(torch.isfinite(t / s).all()):
        return None
    taps = p.kh * p.kw
    w = p.w[:, :taps * p.cin].view(p.cout, taps, p.cin)
    shift = (w.double() * t.double().view(1, 1, -1)).sum(dim=(1, 2)).float()
    if p.shift is not None:
        shift = shift + p.shift
    wf = (w * s.view(1, 1, -1)).reshape(p.cout, taps * p.cin).contiguous()
    q = ConvParams(wf, None, shift.contiguous(), p.cin, p.cout, p.kh, p.kw, p.stride, p.pad, p.dil, p.kpad, False, p.relu,
                   pack_split3(wf) if p.w3 is not None else None)
    return q, (-t / s).contiguous()


def pack_input(img_nchw, prior=None, out=None):
    """[N,3,H,W] (+ [N,1,H,W] prior) -> NHWC4."""
    lib = _lib.load()
    _chk_dev(img_nchw, prior)
    n, c, h, w = img_nchw.shape
    if c != 3 or img_nchw.dtype != torch.float32 or not img_nchw.is_contiguous():
        raise ValueError("pack_input: expected contiguous fp32 [N,3,H,W]")
    if prior is not None and (prior.dtype != torch.float32 or not prior.is_contiguous() or prior.numel() != n * h * w):
        raise ValueError("pack_input: prior must be contiguous fp32 [N,1,H,W]")
    if out is None:
        out = torch.empty((n, h, w, 4), dtype=torch.float32, device=img_nchw.device)
    _lib.check(lib.pemp_pack_input_nhwc4_f32(_p(img_nchw), _p(prior), _p(out), n, h, w, _stream()), "pack_input")
    return out


def _pool_out(i, k, s, p, ceil):
    num = i + 2 * p - k
    o = (-(-num // s) if ceil else num // s) + 1
    if ceil and (o - 1) * s >= i + p:
        o -= 1
    return o


def maxpool2d(x, k, s, p, ceil_mode=False, out=None):
    lib = _lib.load()
    _chk_dev(x)
    ldx = _nhwc(x, "x")
    n, h, w, c = x.shape
    ho, wo = _pool_out(h, k, s, p, ceil_mode), _pool_out(w, k, s, p, ceil_mode)
    if out is None:
        out = torch.empty((n, ho, wo, c), dtype=torch.float32, device=x.device)
    ldy = _nhwc(out, "out")
    _lib.check(lib.pemp_maxpool2d_nhwc_f32(_p(x), _p(out), n, h, w, c, ldx, ho, wo, ldy, k, s, p, _stream()), "maxpool2d")
    return out


def global_avgpool(x, out=None):
    lib = _lib.load()
    _chk_dev(x)
    ldx = _nhwc(x, "x")
    n, h, w, c = x.shape
    if out is None:
        out = torch.empty((n, c), dtype=torch.float32, device=x.device)
    _lib.check(lib.pemp_global_avgpool_nhwc_f32(_p(x), _p(out), n, h * w, c, ldx, _stream()), "global_avgpool")
    return out


def channel_affine_multi(x, scales, shifts, outs):
    """outs[b] = x * scales[b] + shifts[b] (per channel), up to 4 branches sharing one read of x."""
    lib = _lib.load()
    _chk_dev(x, *outs)
    nb = len(outs)
    if x.dim() == 2:
        m, c, ldx = x.shape[0], x.shape[1], x.stride(0)
        ldy = [o.stride(0) for o in outs]
    else:
        ldx = _nhwc(x, "x")
        m, c = x.shape[0] * x.shape[1] * x.shape[2], x.shape[3]
        ldy = [_nhwc(o, "out") for o in outs]
    arr = C.c_void_p * nb
    _lib.check(lib.pemp_channel_affine_multi_f32(
        _p(x), ldx, m, c, nb, arr(*[s.data_ptr() for s in scales]), arr(*[s.data_ptr() for s in shifts]),
        arr(*[o.data_ptr() for o in outs]), (C.c_int * nb)(*ldy), _stream()), "channel_affine_multi")
    return outs


def _ws(nbytes, device, cache=None, key=None):
    if cache is not None:
        t = cache.get(key)
        if t is None or t.numel() < nbytes:
            t = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
            cache[key] = t
        return t
    return torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)


def mpm_protos(sup_feat, sup_mask, ctr, B, S, p, ws_cache=None, out=None):
    """sup_feat [B*S,h,w,c] NHWC; sup_mask [B*S,2,H,W]; ctr [c,2p] -> protos [B,2p,c]."""
    lib = _lib.load()
    _chk_dev(sup_feat, sup_mask, ctr)
    ldf = _nhwc(sup_feat, "sup_feat")
    bs, h, w, c = sup_feat.shape
    H, W = sup_mask.shape[-2:]
    if bs != B * S or sup_mask.numel() != bs * 2 * H * W or not sup_mask.is_contiguous() or sup_mask.dtype != torch.float32:
        raise ValueError("mpm_protos: sup_mask must be contiguous fp32 [B*S,2,H,W]")
    if tuple(ctr.shape) != (c, 2 * p) or not ctr.is_contiguous():
        raise ValueError(f"mpm_protos: ctr must be contiguous [{c},{2 * p}]")
    nbytes = lib.pemp_mpm_workspace_bytes(B, S, h * w, c, p)
    ws = _ws(nbytes, sup_feat.device, ws_cache, ("mpm", B, S, h, w, c, p))
    if out is None:
        out = torch.empty((B, 2 * p, c), dtype=torch.float32, device=sup_feat.device)
    _lib.check(lib.pemp_mpm_protos_f32(_p(sup_feat), ldf, _p(sup_mask), _p(ctr), _p(out), _p(ws), ws.numel(),
                                       B, S, h, w, H, W, c, p, _stream()), "mpm_protos")
    return out


def masked_avg_pool(sup_feat, sup_mask, B, S, full_res, ws_cache=None, out=None):
    """-> protos [B,2,c] (row 0 fg, row 1 bg).  full_res=True is the Baseline form."""
    lib = _lib.load()
    _chk_dev(sup_feat, sup_mask)
    ldf = _nhwc(sup_feat, "sup_feat")
    bs, h, w, c = sup_feat.shape
    H, W = sup_mask.shape[-2:]
    if bs != B * S or sup_mask.numel() != bs * 2 * H * W or not sup_mask.is_contiguous() or sup_mask.dtype != torch.float32:
        raise ValueError("masked_avg_pool: sup_mask must be contiguous fp32 [B*S,2,H,W]")
    nbytes = lib.pemp_map_workspace_bytes(B, S, h * w, c)
    ws = _ws(nbytes, sup_feat.device, ws_cache, ("map", B, S, h, w, c))
    if out is None:
        out = torch.empty((B, 2, c), dtype=torch.float32, device=sup_feat.device)
    _lib.check(lib.pemp_masked_avg_pool_f32(_p(sup_feat), ldf, _p(sup_mask), _p(out), _p(ws), ws.numel(),
                                            B, S, h, w, H, W, c, 1 if full_res else 0, _stream()), "masked_avg_pool")
    return out


def cosine_proto_max(qry_feat, protos, dist_scalar, want_resp=False, pred=None, resp=None):
    """qry_feat [B,h,w,c]; protos [B,2p,c] -> pred [B,2,h,w] (+ resp uint8 [B,h,w])."""
    lib = _lib.load()
    _chk_dev(qry_feat, protos)
    ldf = _nhwc(qry_feat, "qry_feat")
    b, h, w, c = qry_feat.shape
    if protos.shape[0] != b or protos.shape[2] != c or not protos.is_contiguous():
        raise ValueError("cosine_proto_max: protos must be contiguous [B,2p,c]")
    p = protos.shape[1] // 2
    if pred is None:
        pred = torch.empty((b, 2, h, w), dtype=torch.float32, device=qry_feat.device)
    if want_resp and resp is None:
        resp = torch.empty((b, h, w), dtype=torch.uint8, device=qry_feat.device)
    _lib.check(lib.pemp_cosine_proto_max_f32(_p(qry_feat), ldf, _p(protos), _p(pred), _p(resp if want_resp else None),
                                             b, h * w, c, p, float(dist_scalar), _stream()), "cosine_proto_max")
    return (pred, resp) if want_resp else pred


def bank_index(index, n_queries, n_classes):
    """The ``index`` argument of ``cosine_bank_max`` checked on the host: a Python sequence or a CPU integer tensor of
    ``n_queries`` class numbers in ``0 .. n_classes - 1`` -> CPU int32 tensor.  A device tensor is refused: its values could
    only be checked with a synchronisation."""
    if isinstance(index, torch.Tensor):
        if index.device.type != "cpu":
            raise ValueError(f"cosine_bank_max: index must be a Python sequence or a CPU tensor (it is checked on the host), "
                             f"got a tensor on {index.device}")
        if index.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
            raise ValueError(f"cosine_bank_max: index must hold integers, got {index.dtype}")
        idx = index.reshape(-1).to(torch.int64)
        if index.dim() != 1:
            raise ValueError(f"cosine_bank_max: index must have shape [{n_queries}], got {tuple(index.shape)}")
    else:
        vals = list(index)
        if any(int(v) != v for v in vals):
            raise ValueError("cosine_bank_max: index must hold integers")
        idx = torch.tensor([int(v) for v in vals], dtype=torch.int64)
    if idx.numel() != n_queries:
        raise ValueError(f"cosine_bank_max: index has {idx.numel()} entries for {n_queries} queries")
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n_classes):
        raise ValueError(f"cosine_bank_max: index values must lie in 0..{n_classes - 1}, got {idx.tolist()}")
    return idx.to(torch.int32)


def cosine_bank_max(qry_feat, bank, dist_scalar, index=None, want_resp=False, pred=None, resp=None):
    """qry_feat [N,h,w,c] (NHWC view); bank [K,2p,c] (prototypes of K enrolled classes, the layout of ``mpm_protos`` /
    ``masked_avg_pool``).  ``index`` None: every query against every class -> pred [N,K,2,h,w] (+ resp uint8 [N,K,h,w]);
    ``index`` (a Python sequence or a CPU integer tensor [N], checked here against 0 <= i < K, then uploaded as int32):
    query b against class index[b] -> pred [N,2,h,w] (+ resp [N,h,w]).  One launch; [b,k] is bit for bit
    ``cosine_proto_max(qry_feat[b:b+1], bank[k:k+1])[0]``."""
    _bank_shapes(qry_feat, bank)
    if index is not None:
        index = bank_index(index, qry_feat.shape[0], bank.shape[0])
    _lib.load()
    _chk_dev(qry_feat, bank)
    if index is not None:
        index = index.to(qry_feat.device, non_blocking=True)
    return _cosine_bank(qry_feat, bank, dist_scalar, index, want_resp, pred, resp)


def _bank_shapes(qry_feat, bank):
    ldf = _nhwc(qry_feat, "qry_feat")
    c = qry_feat.shape[3]
    if bank.dim() != 3 or bank.dtype != torch.float32 or not bank.is_contiguous() or bank.shape[0] < 1 \
            or bank.shape[1] < 2 or bank.shape[1] % 2:
        raise ValueError(f"cosine_bank_max: bank must be contiguous fp32 [K,2p,c], got {tuple(bank.shape)} {bank.dtype}")
    if bank.shape[2] != c:
        raise ValueError(f"cosine_bank_max: bank has c = {bank.shape[2]}, the features have c = {c}")
    return ldf


def _cosine_bank(qry_feat, bank, dist_scalar, index_dev, want_resp=False, pred=None, resp=None):
    """The launch of ``cosine_bank_max``.  ``index_dev``: None or an int32 DEVICE tensor [N] whose values the caller has
    checked on the host (``bank_index``) -- the static index buffer of a captured graph comes in here."""
    lib = _lib.load()
    _chk_dev(qry_feat, bank, index_dev)
    ldf = _bank_shapes(qry_feat, bank)
    n, h, w, c = qry_feat.shape
    k, p = bank.shape[0], bank.shape[1] // 2
    index = index_dev
    if index is not None and (index.dtype != torch.int32 or tuple(index.shape) != (n,) or not index.is_contiguous()):
        raise ValueError(f"cosine_bank_max: the device index must be contiguous int32 [{n}]")
    lead = (n,) if index is not None else (n, k)
    if pred is None:
        pred = torch.empty(lead + (2, h, w), dtype=torch.float32, device=qry_feat.device)
    if want_resp and resp is None:
        resp = torch.empty(lead + (h, w), dtype=torch.uint8, device=qry_feat.device)
    _lib.check(lib.pemp_cosine_bank_max_f32(_p(qry_feat), ldf, _p(bank), _p(index), _p(pred), _p(resp if want_resp else None),
                                            n, k, h * w, c, p, float(dist_scalar), _stream()), "cosine_bank_max")
    return (pred, resp) if want_resp else pred


def upsample_bilinear_ac(pred, out_hw):
    lib = _lib.load()
    _chk_dev(pred)
    b, c, h, w = pred.shape
    ho, wo = int(out_hw[0]), int(out_hw[1])
    out = torch.empty((b, c, ho, wo), dtype=torch.float32, device=pred.device)
    _lib.check(lib.pemp_upsample_bilinear_ac_f32(_p(pred.contiguous()), _p(out), b, c, h, w, ho, wo, _stream()),
               "upsample_bilinear_ac")
    return out


def upsample_nearest_u8_i64(resp, out_hw):
    lib = _lib.load()
    _chk_dev(resp)
    b, h, w = resp.shape
    ho, wo = int(out_hw[0]), int(out_hw[1])
    out = torch.empty((b, ho, wo), dtype=torch.int64, device=resp.device)
    _lib.check(lib.pemp_upsample_nearest_u8_i64(_p(resp.contiguous()), _p(out), b, h, w, ho, wo, _stream()),
               "upsample_nearest")
    return out


def cedt_weight(target, sigma=5.0, ws_cache=None):
    """CELossDT weight map (core/losses.py:23-41) on the device: target int64 [B,H,W] -> fp32 [B,H,W]."""
    lib = _lib.load()
    _chk_dev(target)
    if target.dtype != torch.int64 or not target.is_contiguous() or target.dim() != 3:
        raise ValueError("cedt_weight: target must be contiguous int64 [B,H,W]")
    b, h, w = target.shape
    out = torch.empty((b, h, w), dtype=torch.float32, device=target.device)
    ws = _ws(lib.pemp_cedt_workspace_bytes(b, h, w), target.device, ws_cache, ("cedt", b, h, w))
    _lib.check(lib.pemp_cedt_weight_f32(_p(target), _p(out), _p(ws), ws.numel(), b, h, w, float(sigma), _stream()), "cedt_weight")
    return out


def argmax_masks(pred):
    """pred [B,2,h,w] -> masks [B,2,h,w] fp32: channel 0 = (argmax == 1), channel 1 = (argmax == 0) (panet.py:169-171)."""
    lib = _lib.load()
    _chk_dev(pred)
    b, c, h, w = pred.shape
    if c != 2 or not pred.is_contiguous() or pred.dtype != torch.float32:
        raise ValueError("argmax_masks: pred must be contiguous fp32 [B,2,h,w]")
    masks = torch.empty_like(pred)
    _lib.check(lib.pemp_argmax_masks_f32(_p(pred), _p(masks), b, h * w, _stream()), "argmax_masks")
    return masks


def eval_tail(pred, target, want_logits=False, ws_cache=None, out_hw=None, weight=None):
    """pred [B,2,h,w]; target int64 [B,Ho,Wo] (or None with ``out_hw``: argmax only, statistics are zero)
    -> (argmax uint8 [B,Ho,Wo], stats f64 [B,8], logits|None)."""
    lib = _lib.load()
    _chk_dev(pred, target)
    b, c, h, w = pred.shape
    if c != 2 or not pred.is_contiguous():
        raise ValueError("eval_tail: pred must be contiguous [B,2,h,w]")
    if target is None:
        ho, wo = int(out_hw[0]), int(out_hw[1])
    else:
        if target.dtype != torch.int64 or not target.is_contiguous() or target.shape[0] != b:
            raise ValueError("eval_tail: target must be contiguous int64 [B,Ho,Wo]")
        ho, wo = target.shape[-2:]
    am = torch.empty((b, ho, wo), dtype=torch.uint8, device=pred.device)
    stats = torch.empty((b, 8), dtype=torch.float64, device=pred.device)
    logits = torch.empty((b, 2, ho, wo), dtype=torch.float32, device=pred.device) if want_logits else None
    nbytes = lib.pemp_eval_tail_workspace_bytes(b, ho, wo)
    ws = _ws(nbytes, pred.device, ws_cache, ("tail", b, ho, wo))
    if weight is not None and (weight.dtype != torch.float32 or not weight.is_contiguous() or tuple(weight.shape) != (b, ho, wo)):
        raise ValueError("eval_tail: weight must be contiguous fp32 [B,Ho,Wo]")
    _lib.check(lib.pemp_eval_tail_weighted_f32(_p(pred), _p(target), _p(weight), _p(am), _p(logits), _p(stats), _p(ws),
                                               ws.numel(), b, h, w, ho, wo, _stream()), "eval_tail")
    return am, stats, logits


def nway_tail(pred, out_hw=None, target=None, want=None, want_margin=False, ws_cache=None):
    """The K binary maps of an all-classes bank call fused into one label map: pred fp32 [N,K,2,h,w] (``segment_lowres``
    without an index) -> (labels uint8 [N,Ho,Wo], margin fp32 [N,Ho,Wo] | None, stats f64 [N,8] | None).  Class k claims a
    pixel of the upsampled logits iff its foreground logit exceeds its background logit; the label is 0 where no class
    claims, else 1 + the claiming k with the largest margin (foreground - background; the lowest k wins equal margins):
    slot numbers, ``bank.labels`` maps them.  ``margin`` (``want_margin``): the winner's, or the largest (<= 0) where nobody
    claims.  ``target`` int64 [N,Ho,Wo] (gives the output size; ``out_hw`` otherwise) comes with ``want``, the slot scored per
    query -- a Python sequence or a CPU tensor, checked here (``bank_index``) and uploaded, or a device int32 [N] -- and gives
    ``stats`` in ``eval_tail``'s layout: the CE of the wanted class's own logits, tp/fp/fn of ``labels == want + 1``."""
    lib = _lib.load()
    if pred.dim() != 5 or pred.dtype != torch.float32 or not pred.is_contiguous() or pred.shape[2] != 2 or min(pred.shape) < 1:
        raise ValueError(f"nway_tail: pred must be contiguous fp32 [N,K,2,h,w], got {tuple(pred.shape)} {pred.dtype}")
    n, k, _, h, w = pred.shape
    if k > 255:
        raise ValueError(f"nway_tail: K = {k}: the labels are uint8 with 0 for no class, so K <= 255")
    if (target is None) != (want is None):
        raise ValueError("nway_tail: target and want come together")
    if target is None:
        if out_hw is None:
            raise ValueError("nway_tail: out_hw is needed without a target")
        ho, wo = int(out_hw[0]), int(out_hw[1])
        if ho < 1 or wo < 1:
            raise ValueError(f"nway_tail: out_hw = {(ho, wo)}")
    else:
        if target.dtype != torch.int64 or not target.is_contiguous() or target.dim() != 3 or target.shape[0] != n:
            raise ValueError(f"nway_tail: target must be contiguous int64 [{n},Ho,Wo]")
        ho, wo = (int(v) for v in target.shape[-2:])
        if out_hw is not None and (int(out_hw[0]), int(out_hw[1])) != (ho, wo):
            raise ValueError(f"nway_tail: out_hw = {tuple(out_hw)} against a target of {(ho, wo)}")
        if isinstance(want, torch.Tensor) and want.device.type != "cpu":
            if want.dtype != torch.int32 or tuple(want.shape) != (n,) or not want.is_contiguous():
                raise ValueError(f"nway_tail: a device want must be contiguous int32 [{n}]")
        else:
            want = bank_index(want, n, k).to(pred.device, non_blocking=True)
    _chk_dev(pred, target, want)
    labels = torch.empty((n, ho, wo), dtype=torch.uint8, device=pred.device)
    margin = torch.empty((n, ho, wo), dtype=torch.float32, device=pred.device) if want_margin else None
    stats = torch.empty((n, 8), dtype=torch.float64, device=pred.device) if target is not None else None
    ws = _ws(lib.pemp_nway_tail_workspace_bytes(n, ho, wo), pred.device, ws_cache, ("nway", n, ho, wo))
    _lib.check(lib.pemp_nway_tail_f32(_p(pred), _p(target), _p(want), _p(labels), _p(margin), _p(stats), _p(ws), ws.numel(),
                                      n, k, h, w, ho, wo, _stream()), "nway_tail")
    return labels, margin, stats


def _ragged_plan(what, n, sizes, targets, device):
    """The shared front of the ragged tails: checks ``sizes`` / ``targets`` (every refusal is a ValueError raised before any
    device work), plans one ``pemp_tail_item`` per image on the host and uploads the descriptors as ONE non-blocking copy.
    -> (items on the host, items on the device, [(Ho, Wo)], [pix_off] + [total], packed target | None, workspace bytes)."""
    if (sizes is None) == (targets is None):
        raise ValueError(f"{what}: give either sizes or targets")
    if targets is not None:
        targets = list(targets)
        if len(targets) != n:
            raise ValueError(f"{what}: {len(targets)} targets for {n} images")
        for i, t in enumerate(targets):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[0] != 1):
                raise ValueError(f"{what}: target {i} must be an int64 tensor [Ho,Wo] or [1,Ho,Wo], got "
                                 f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__} {getattr(t, 'dtype', '')}")
        hw = [(int(t.shape[-2]), int(t.shape[-1])) for t in targets]
    else:
        sizes = list(sizes)
        if len(sizes) != n:
            raise ValueError(f"{what}: {len(sizes)} sizes for {n} images")
        if any(len(tuple(s)) != 2 for s in sizes):
            raise ValueError(f"{what}: every size is a (Ho, Wo) pair, got {sizes}")
        hw = [(int(s[0]), int(s[1])) for s in sizes]
    for i, (ho, wo) in enumerate(hw):
        if ho < 1 or wo < 1:
            raise ValueError(f"{what}: image {i} has the size {(ho, wo)}")
    if device.type != "cuda":
        raise _lib.PempHipError("pemp_amd ops need device (cuda/HIP) tensors; there is no CPU path")
    lib = _lib.load()
    items = (_lib.TailItem * n)()
    for it, (ho, wo) in zip(items, hw):
        it.Ho, it.Wo = ho, wo
    nbytes = lib.pemp_tail_ragged_workspace_bytes(items, n)
    if nbytes == 0:
        raise ValueError(f"{what}: {lib.pemp_last_error().decode(errors='replace')}")
    offs = [0]
    for ho, wo in hw:                                               # pix_off: the running sum of Ho * Wo
        offs.append(offs[-1] + ho * wo)
    items_dev = torch.frombuffer(items, dtype=torch.uint8).to(device, non_blocking=True)
    packed = None
    if targets is not None:
        if all(t.device.type == "cpu" for t in targets):
            # every label uploaded into its place in the packed buffer.  (Packing on the host first and uploading once was
            # measured at 12 ms per 25 PASCAL-sized labels, against 1.3 ms for the 25 uploads: profiles/ragged_tail_bench.txt)
            packed = torch.empty(offs[-1], dtype=torch.int64, device=device)
            for i, t in enumerate(targets):
                packed[offs[i]:offs[i + 1]].copy_(t.reshape(-1), non_blocking=True)
        else:
            packed = torch.cat([t.to(device, non_blocking=True).reshape(-1) for t in targets])
    return items, items_dev, hw, offs, packed, nbytes


def _ragged_views(packed, hw):
    return [flat.view(ho, wo) for flat, (ho, wo) in zip(packed.split([ho * wo for ho, wo in hw]), hw)]


def eval_tail_ragged(pred, targets=None, sizes=None, ws_cache=None, views=True):
    """``eval_tail`` for a batch whose images each have their own output size, in ONE launch pair: pred [B,2,h,w];
    ``targets``, a list of B int64 tensors [Ho_i,Wo_i] or [1,Ho_i,Wo_i] (device tensors are flattened and concatenated, CPU
    tensors are uploaded each into its place in the packed buffer), or ``sizes``, a list of B (Ho, Wo): arg-max only.
    -> (am_list, stats f64 [B,8] | None without targets, am_packed uint8 [sum Ho_i * Wo_i]); ``am_list[i]`` is a
    [Ho_i,Wo_i] view into ``am_packed`` (``views`` off: None -- a caller that wants the rows alone saves the B views).  Per image
    every result is bit for bit ``eval_tail``'s on that image alone."""
    if pred.dim() != 4 or pred.shape[1] != 2 or pred.dtype != torch.float32 or not pred.is_contiguous() or min(pred.shape) < 1:
        raise ValueError(f"eval_tail_ragged: pred must be contiguous fp32 [B,2,h,w], got {tuple(pred.shape)} {pred.dtype}")
    b, _, h, w = pred.shape
    items, items_dev, hw, offs, target, nbytes = _ragged_plan("eval_tail_ragged", b, sizes, targets, pred.device)
    lib = _lib.load()
    am = torch.empty(offs[-1], dtype=torch.uint8, device=pred.device)
    stats = torch.empty((b, 8), dtype=torch.float64, device=pred.device) if target is not None else None
    ws = _ws(nbytes, pred.device, ws_cache, ("tail_ragged", b))       # one per B: it grows to the largest size mix seen
    _lib.check(lib.pemp_eval_tail_ragged_f32(_p(pred), _p(target), items, _p(items_dev), b, h, w, _p(am), _p(stats), _p(ws),
                                             ws.numel(), _stream()), "eval_tail_ragged")
    return (_ragged_views(am, hw) if views else None), stats, am


def nway_tail_ragged(pred, sizes=None, targets=None, want=None, want_margin=False, ws_cache=None, views=True):
    """``nway_tail`` for a batch whose images each have their own output size, in ONE launch pair: pred fp32 [N,K,2,h,w];
    ``sizes`` (a list of N (Ho, Wo)) or ``targets`` (a list of N int64 tensors, as in ``eval_tail_ragged``) with ``want``
    (``nway_tail``'s).  -> (labels_list, margin_list | None, stats f64 [N,8] | None): the maps of image i are [Ho_i,Wo_i]
    views into one packed buffer each (``views`` off: the packed buffers themselves).  Per image every result is bit for bit
    ``nway_tail``'s on that image alone."""
    if pred.dim() != 5 or pred.dtype != torch.float32 or not pred.is_contiguous() or pred.shape[2] != 2 or min(pred.shape) < 1:
        raise ValueError(f"nway_tail_ragged: pred must be contiguous fp32 [N,K,2,h,w], got {tuple(pred.shape)} {pred.dtype}")
    n, k, _, h, w = pred.shape
    if k > 255:
        raise ValueError(f"nway_tail_ragged: K = {k}: the labels are uint8 with 0 for no class, so K <= 255")
    if (targets is None) != (want is None):
        raise ValueError("nway_tail_ragged: targets and want come together")
    if want is not None:
        if isinstance(want, torch.Tensor) and want.device.type != "cpu":
            if want.dtype != torch.int32 or tuple(want.shape) != (n,) or not want.is_contiguous():
                raise ValueError(f"nway_tail_ragged: a device want must be contiguous int32 [{n}]")
        else:
            want = bank_index(want, n, k)
    items, items_dev, hw, offs, target, nbytes = _ragged_plan("nway_tail_ragged", n, sizes, targets, pred.device)
    if want is not None:
        want = want.to(pred.device, non_blocking=True)
    lib = _lib.load()
    labels = torch.empty(offs[-1], dtype=torch.uint8, device=pred.device)
    margin = torch.empty(offs[-1], dtype=torch.float32, device=pred.device) if want_margin else None
    stats = torch.empty((n, 8), dtype=torch.float64, device=pred.device) if target is not None else None
    ws = _ws(nbytes, pred.device, ws_cache, ("tail_ragged", n))
    _lib.check(lib.pemp_nway_tail_ragged_f32(_p(pred), _p(target), _p(want), items, _p(items_dev), n, k, h, w, _p(labels),
                                             _p(margin), _p(stats), _p(ws), ws.numel(), _stream()), "nway_tail_ragged")
    if not views:
        return labels, margin, stats
    return _ragged_views(labels, hw), (_ragged_views(margin, hw) if want_margin else None), stats


#: the N-way confusion tails count in (K + 1)^2 <= 4096 bins of LDS per block
CONFUSION_MAX_K = 63


def _confusion_args(what, pred, want):
    """The checks both confusion wrappers share, all on the host: -> (n, k, h, w, want as a host int32 tensor from
    ``bank_index``, a checked device tensor, or None)."""
    if pred.dim() != 5 or pred.dtype != torch.float32 or not pred.is_contiguous() or pred.shape[2] != 2 or min(pred.shape) < 1:
        raise ValueError(f"{what}: pred must be contiguous fp32 [N,K,2,h,w], got {tuple(pred.shape)} {pred.dtype}")
    n, k, _, h, w = pred.shape
    if k > CONFUSION_MAX_K:
        raise ValueError(f"{what}: K = {k}: a block counts in (K + 1)^2 <= 4096 bins, so K <= {CONFUSION_MAX_K}")
    if want is not None:
        if isinstance(want, torch.Tensor) and want.device.type != "cpu":
            if want.dtype != torch.int32 or tuple(want.shape) != (n,) or not want.is_contiguous():
                raise ValueError(f"{what}: a device want must be contiguous int32 [{n}]")
        else:
            want = bank_index(want, n, k)
    return n, k, h, w, want


def nway_confusion(pred, target, want=None, want_labels=False, ws_cache=None):
    """The N-way label map of ``nway_tail`` counted against a target in one launch: pred fp32 [N,K,2,h,w], target int64
    [N,Ho,Wo] -> (conf int64 [N,K+1,K+1], labels uint8 [N,Ho,Wo] | None).  ``conf[n, t, p]`` is the number of counted pixels of
    image n with target class t and label p (0: no class, 1 + slot otherwise).  ``want`` None: the target holds slot labels
    0..K (``slot_targets`` makes them from dataset class ids).  ``want`` (``nway_tail``'s: a Python sequence or a CPU tensor,
    checked here, or a device int32 [N]): the target is the binary mask 0 / 1 / 255 of the query's own class, 1 standing for
    slot ``want[n]``.  255 and every other value that is no class of the table is ignored (the values are not checked here:
    that would need a synchronisation).  Without ``want_labels`` nothing is written per pixel; with it the labels are
    ``nway_tail``'s bit for bit.  K <= 63.  The counts are integers: exact, and identical from run to run.  ``ws_cache`` is
    taken as the other tails take it and not used: this tail has no workspace."""
    lib = _lib.load()
    n, k, h, w, want = _confusion_args("nway_confusion", pred, want)
    if not isinstance(target, torch.Tensor) or target.dtype != torch.int64 or not target.is_contiguous() or target.dim() != 3 \
            or target.shape[0] != n or min(target.shape) < 1:
        raise ValueError(f"nway_confusion: target must be contiguous int64 [{n},Ho,Wo]")
    ho, wo = (int(v) for v in target.shape[-2:])
    _chk_dev(pred, target)
    if want is not None:
        want = want.to(pred.device, non_blocking=True)
    conf = torch.empty((n, k + 1, k + 1), dtype=torch.int64, device=pred.device)
    labels = torch.empty((n, ho, wo), dtype=torch.uint8, device=pred.device) if want_labels else None
    # no workspace: the blocks flush into conf with integer atomics (pemp_nway_confusion_workspace_bytes is 0 at every size)
    _lib.check(lib.pemp_nway_confusion_f32(_p(pred), _p(target), _p(want), _p(labels), _p(conf), _p(None), 0, n, k, h, w, ho, wo,
                                           _stream()), "nway_confusion")
    return conf, labels


def nway_confusion_ragged(pred, targets, want=None, want_labels=False, ws_cache=None, views=True):
    """``nway_confusion`` for a batch whose images each have their own size, in ONE launch: pred fp32 [N,K,2,h,w]; ``targets`` a
    list of N int64 tensors [Ho_i,Wo_i] or [1,Ho_i,Wo_i] on the host or the device (``eval_tail_ragged``'s); ``want`` as in
    ``nway_confusion``.  -> (conf int64 [N,K+1,K+1], labels | None): with ``want_labels`` a list of N uint8 [Ho_i,Wo_i] views
    into one packed buffer (``views`` off: the packed buffer itself).  Per image the table and the labels are the fixed-size
    call's on that image alone."""
    n, k, h, w, want = _confusion_args("nway_confusion_ragged", pred, want)
    if targets is None:
        raise ValueError("nway_confusion_ragged: targets are needed (a confusion table counts against them)")
    items, items_dev, hw, offs, target, _ = _ragged_plan("nway_confusion_ragged", n, None, targets, pred.device)
    if want is not None:
        want = want.to(pred.device, non_blocking=True)
    lib = _lib.load()
    conf = torch.empty((n, k + 1, k + 1), dtype=torch.int64, device=pred.device)
    labels = torch.empty(offs[-1], dtype=torch.uint8, device=pred.device) if want_labels else None
    _lib.check(lib.pemp_nway_confusion_ragged_f32(_p(pred), _p(target), _p(want), items, _p(items_dev), n, k, h, w, _p(labels),
                                                  _p(conf), _p(None), 0, _stream()), "nway_confusion_ragged")
    if labels is None or not views:
        return conf, labels
    return conf, _ragged_views(labels, hw)


def slot_targets(target_ids, bank_labels):
    """Ground truth in dataset class ids -> the slot labels ``nway_confusion`` counts against: an integer tensor of ids in
    0..255 (any shape, any device) through a 256-entry table -> int64 of the same shape; the id ``bank_labels[s]`` becomes
    ``s + 1``, an id the bank does not hold becomes 0 (background) and 255 stays 255 (ignored).  A plain gather, no kernel."""
    ids = [int(v) for v in bank_labels]
    if any(v != b for v, b in zip(ids, bank_labels)) or any(not 1 <= v <= 254 for v in ids) or len(set(ids)) != len(ids):
        raise ValueError(f"slot_targets: bank_labels must be distinct class ids in 1..254, got {list(bank_labels)}")
    if not isinstance(target_ids, torch.Tensor) or target_ids.dtype not in (torch.uint8, torch.int16, torch.int32, torch.int64):
        raise ValueError("slot_targets: target_ids must be a uint8, int16, int32 or int64 tensor of ids in 0..255")
    table = torch.zeros(256, dtype=torch.int64)
    table[torch.tensor(ids, dtype=torch.int64)] = torch.arange(1, len(ids) + 1)
    table[255] = 255
    return table.to(target_ids.device)[target_ids.long()]


#: PEMP_RAGGED_TAIL=0 withholds the ragged tails from the evaluators: ``tail_rows`` then makes one fixed-size launch pair per
#: distinct label size (A/B switch; scratch/ragged_tail_bench.py measures both)
RAGGED_TAIL = os.environ.get("PEMP_RAGGED_TAIL", "1") != "0"


def tail_rows(pred, labels, want=None, ws_cache=None):
    """The statistics rows of a batch of episodes whose query labels keep their own sizes: pred [B,2,h,w] (``want`` None:
    the eval tail) or [B,K,2,h,w] (``want``: the scored slot per query, the N-way tail), ``labels`` a list of B int64
    tensors [1,Ho_i,Wo_i] on the host or the device.  -> stats f64 [B,8] on the GPU, rows in the given order: one ragged
    launch pair, or with ``RAGGED_TAIL`` off one fixed-size launch pair per distinct label size.  Either way row i is the
    fixed-size tail's on episode i alone."""
    if RAGGED_TAIL:
        if want is None:
            return eval_tail_ragged(pred, labels, ws_cache=ws_cache, views=False)[1]
        return nway_tail_ragged(pred, targets=labels, want=want, ws_cache=ws_cache, views=False)[2]
    stats = torch.empty((len(labels), 8), dtype=torch.float64, device=pred.device)
    by_size = {}
    for i, lab in enumerate(labels):
        by_size.setdefault(tuple(lab.shape[-2:]), []).append(i)
    for idx in by_size.values():
        sel = torch.tensor(idx, device=pred.device)
        tgt = torch.cat([labels[i].to(pred.device, non_blocking=True) for i in idx])
        if want is None:
            st = eval_tail(pred.index_select(0, sel), tgt, ws_cache=ws_cache)[1]
        else:
            st = nway_tail(pred.index_select(0, sel), target=tgt, want=[want[i] for i in idx], ws_cache=ws_cache)[2]
        stats.index_copy_(0, sel, st)
    return stats


def cm_reduce(x, mask_in, stride, want_argmax=False):
    """ResNetCM.comm statistics: x NHWC [N,h,w,C] (or None: pool the mask only); mask_in [N,Hm,Wm]
    -> (mask_out [N,h,w], stat [N,2,C] | None) (+ argmax int32 [N,C] with ``want_argmax``: the first maximal pixel,
    which train_ops.cm_bwd_add can use instead of searching for it again)."""
    lib = _lib.load()
    _chk_dev(x, mask_in)
    hm, wm = mask_in.shape[-2:]
    n = mask_in.shape[0]
    if x is None:
        h, w, c, ldx, stat = (hm + 2 - 3) // stride + 1, (wm + 2 - 3) // stride + 1, 0, 0, None
    else:
        ldx = _nhwc(x, "x")
        n, h, w, c = x.shape
        stat = torch.empty((n, 2, c), dtype=torch.float32, device=x.device)
    mask_out = torch.empty((n, h, w), dtype=torch.float32, device=mask_in.device)
    if want_argmax:
        arg = torch.empty((n, c), dtype=torch.int32, device=x.device)
        _lib.check(lib.pemp_cm_reduce_arg_f32(_p(x), ldx, _p(mask_in.contiguous()), _p(mask_out), _p(stat), _p(arg), n, hm, wm,
                                              h, w, c, stride, _stream()), "cm_reduce_arg")
        return mask_out, stat, arg
    _lib.check(lib.pemp_cm_reduce_f32(_p(x), ldx, _p(mask_in.contiguous()), _p(mask_out), _p(stat), n, hm, wm, h, w, c,
                                      stride, _stream()), "cm_reduce")
    return mask_out, stat


def cm_linear(stat, group, lin_w, lin_b, n_groups):
    """ResNetCM.comm after the statistics: stat [N,2,C] (or [N,2C]) -> (agg [G,2C] episode means, feat [G,2])."""
    lib = _lib.load()
    _chk_dev(stat, group, lin_w, lin_b)
    n = stat.shape[0]
    c2 = stat.numel() // n
    if group.dtype != torch.int32 or group.numel() != n or tuple(lin_w.shape) != (2, c2):
        raise ValueError("cm_linear: group must be int32 [N], lin_w [2, 2C]")
    agg = torch.empty((n_groups, c2), dtype=torch.float32, device=stat.device)
    feat = torch.empty((n_groups, 2), dtype=torch.float32, device=stat.device)
    _lib.check(lib.pemp_cm_linear_f32(_p(stat.contiguous()), _p(group), _p(lin_w.contiguous()), _p(lin_b.contiguous()), _p(agg),
                                      _p(feat), n, n_groups, c2, _stream()), "cm_linear")
    return agg, feat


def cm_bias(feat, group, wext, alpha=None, base=None):
    """Per-image bias of the two communication channels: [N, Cout] = base + alpha * (feat[group] @ wext^T).
    ``wext`` [Cout, 2] may be a strided column slice of the [Cout, C+2] weight matrix."""
    lib = _lib.load()
    _chk_dev(feat, group, wext, alpha, base)
    cout = wext.shape[0]
    if wext.dim() != 2 or wext.shape[1] != 2 or wext.stride(1) != 1:
        raise ValueError("cm_bias: wext must be [Cout, 2] with unit column stride")
    n = group.numel()
    out = torch.empty((n, cout), dtype=torch.float32, device=feat.device)
    _lib.check(lib.pemp_cm_bias_f32(_p(feat), _p(group), _p(wext), wext.stride(0), _p(alpha), _p(base), _p(out), n, cout,
                                    _stream()), "cm_bias")
    return out


# -- PFENet inference (csrc/pfenet.hip) ---------------------------------------------------------------------------------------
def prior_mask(qry, sup, mask, S, out=None, ws_cache=None):
    """PFENet's prior (networks/pfenet.py:201-227): qry NHWC [B,h,w,C], sup NHWC [B*S,h,w,C], mask fp32 [B*S,h,w] (support masks
    at feature resolution) -> [B,h,w] (the min-max normalised max cosine, averaged over the S shots)."""
    lib = _lib.load()
    _chk_dev(qry, sup, mask, out)
    ldq, lds = _nhwc(qry, "qry"), _nhwc(sup, "sup")
    b, h, w, c = qry.shape
    if tuple(sup.shape) != (b * S, h, w, c) or tuple(mask.shape) != (b * S, h, w) or not mask.is_contiguous() \
            or mask.dtype != torch.float32:
        raise ValueError(f"prior_mask: sup {tuple(sup.shape)} / mask {tuple(mask.shape)} do not match qry {tuple(qry.shape)} x S={S}")
    if out is None:
        out = torch.empty((b, h, w), dtype=torch.float32, device=qry.device)
    if tuple(out.shape) != (b, h, w) or not out.is_contiguous():
        raise ValueError("prior_mask: out must be contiguous [B,h,w]")
    ws = _ws(lib.pemp_prior_mask_workspace_bytes(b, S, h * w), qry.device, ws_cache, ("prior", b, S, h * w))
    _lib.check(lib.pemp_prior_mask_f32(_p(qry), ldq, _p(sup), lds, _p(mask), _p(out), _p(ws), ws.numel(), b, S, h * w, c,
                                       _stream()), "prior_mask")
    return out


def _round64(n):
    return -(-int(n) // 64) * 64


def _prior_bank_masks(mask, K, S):
    if mask.dim() != 3 or mask.dtype != torch.float32 or not mask.is_contiguous() or mask.shape[0] != K * S or K < 1 or S < 1:
        raise ValueError(f"prior_bank_pack: mask must be contiguous fp32 [K*S,h,w] with K*S = {K * S}, got {tuple(mask.shape)} "
                         f"{mask.dtype}")


def prior_bank_count(mask, K, S, out=None):
    """Rows a packed bank slot needs per (class, shot): mask fp32 [K*S,h,w] -> int32 [K,S] on the device (the pixels with
    m != 0, plus one if a pixel with m == 0 exists).  The count-only form of ``prior_bank_pack``."""
    _prior_bank_masks(mask, K, S)
    lib = _lib.load()
    _chk_dev(mask, out)
    if out is None:
        out = torch.empty((K, S), dtype=torch.int32, device=mask.device)
    if tuple(out.shape) != (K, S) or out.dtype != torch.int32 or not out.is_contiguous():
        raise ValueError(f"prior_bank_count: out must be contiguous int32 [{K},{S}]")
    _lib.check(lib.pemp_prior_bank_pack_f32(None, 0, _p(mask), None, None, _p(out), K * S, mask.shape[1] * mask.shape[2], 0, 0,
                                            _stream()), "prior_bank_count")
    return out


def _prior_bank_store(rows, norms, count, what):
    """The packed bank's tensors checked -> (K, S, cap, C)."""
    if rows.dim() != 4 or rows.dtype != torch.float32 or not rows.is_contiguous() or min(rows.shape) < 1:
        raise ValueError(f"{what}: rows must be contiguous fp32 [K,S,cap,C], got {tuple(rows.shape)} {rows.dtype}")
    K, S, cap, C = rows.shape
    if cap % 64:
        raise ValueError(f"{what}: cap must be a multiple of 64, got {cap}")
    if C % 32:
        raise ValueError(f"{what}: C must be a multiple of 32, got {C}")
    if tuple(norms.shape) != (K, S, cap) or norms.dtype != torch.float32 or not norms.is_contiguous():
        raise ValueError(f"{what}: norms must be contiguous fp32 [{K},{S},{cap}], got {tuple(norms.shape)} {norms.dtype}")
    if tuple(count.shape) != (K, S) or count.dtype != torch.int32 or not count.is_contiguous():
        raise ValueError(f"{what}: count must be contiguous int32 [{K},{S}], got {tuple(count.shape)} {count.dtype}")
    return K, S, cap, C


def prior_bank_pack(sup, mask, K, S, cap=None, rows=None, norms=None, count=None):
    """The support side of ``prior_mask`` stored per (class, shot): sup NHWC [K*S,h,w,C], mask fp32 [K*S,h,w] ->
    (rows [K,S,cap,C], norms [K,S,cap], count int32 [K,S]).  Slot (k, s) holds fl(m * s) of the pixels with m != 0 in pixel
    order, then one all-zero row if a pixel with m == 0 exists; slots beyond ``count`` are not written (a new store is zeroed).
    A row that does not fit into ``cap`` is dropped and ``count`` says so: compare it with ``cap`` (``cap`` None without
    ``rows``: h * w rounded up to 64, which always fits)."""
    lds = _nhwc(sup, "sup")
    ks, h, w, C = sup.shape
    _prior_bank_masks(mask, K, S)
    if tuple(mask.shape) != (ks, h, w):
        raise ValueError(f"prior_bank_pack: mask {tuple(mask.shape)} does not match sup {tuple(sup.shape)}")
    if rows is None:
        cap = _round64(h * w) if cap is None else int(cap)
        if cap < 64 or cap % 64:
            raise ValueError(f"prior_bank_pack: cap must be a multiple of 64, got {cap}")
        if C % 32:
            raise ValueError(f"prior_bank_pack: C must be a multiple of 32, got {C}")
        rows = torch.zeros((K, S, cap, C), dtype=torch.float32, device=sup.device)
        norms = torch.zeros((K, S, cap), dtype=torch.float32, device=sup.device)
        count = torch.ones((K, S), dtype=torch.int32, device=sup.device)
    if norms is None or count is None:
        raise ValueError("prior_bank_pack: rows, norms and count go together")
    k2, s2, cap, c2 = _prior_bank_store(rows, norms, count, "prior_bank_pack")
    if (k2, s2) != (K, S) or c2 != C:
        raise ValueError(f"prior_bank_pack: the store is [K={k2},S={s2},cap,C={c2}], the supports are K={K}, S={S}, C={C}")
    lib = _lib.load()
    _chk_dev(sup, mask, rows, norms, count)
    _lib.check(lib.pemp_prior_bank_pack_f32(_p(sup), lds, _p(mask), _p(rows), _p(norms), _p(count), K * S, h * w, C, cap, _stream()),
               "prior_bank_pack")
    return rows, norms, count


def prior_bank(qry, rows, norms, count, index=None, out=None, ws_cache=None):
    """``prior_mask`` of N queries against a packed bank (``prior_bank_pack``): qry NHWC [N,h,w,C].  ``index`` None: every
    query against every class -> [N,K,h,w]; ``index`` (a Python sequence or a CPU integer tensor [N], checked here against
    0 <= i < K, then uploaded as int32): query n against class index[n] -> [N,h,w].  [n, k] is bit for bit
    ``prior_mask(qry[n:n+1], sup[k*S:(k+1)*S], mask[k*S:(k+1)*S], S)[0]`` on the supports class k was packed from."""
    _prior_bank_shapes(qry, rows, norms, count)
    if index is not None:
        index = bank_index(index, qry.shape[0], rows.shape[0])
    _lib.load()
    _chk_dev(qry, rows, norms, count, out)
    if index is not None:
        index = index.to(qry.device, non_blocking=True)
    return _prior_bank(qry, rows, norms, count, index, out, ws_cache)


def _prior_bank_shapes(qry, rows, norms, count):
    ldq = _nhwc(qry, "qry")
    K, S, cap, C = _prior_bank_store(rows, norms, count, "prior_bank")
    if qry.shape[3] != C:
        raise ValueError(f"prior_bank: the bank has C = {C}, the features have C = {qry.shape[3]}")
    return ldq


def _prior_bank(qry, rows, norms, count, index_dev, out=None, ws_cache=None):
    """The launch of ``prior_bank``.  ``index_dev``: None or an int32 DEVICE tensor [N] whose values the caller has checked on
    the host (``bank_index``) -- the static index buffer of a captured graph comes in here."""
    ldq = _prior_bank_shapes(qry, rows, norms, count)
    n, h, w, C = qry.shape
    K, S, cap = rows.shape[:3]
    index = index_dev
    if index is not None and (not isinstance(index, torch.Tensor) or not index.is_cuda or index.dtype != torch.int32
                              or tuple(index.shape) != (n,) or not index.is_contiguous()):
        raise ValueError(f"prior_bank: the device index must be a contiguous int32 tensor [{n}] on the GPU")
    lead = (n,) if index is not None else (n, K)
    lib = _lib.load()
    _chk_dev(qry, rows, norms, count, out)
    if out is None:
        out = torch.empty(lead + (h, w), dtype=torch.float32, device=qry.device)
    if tuple(out.shape) != lead + (h, w) or not out.is_contiguous():
        raise ValueError(f"prior_bank: out must be contiguous {list(lead + (h, w))}")
    pairs = n if index is not None else n * K
    ws = _ws(lib.pemp_prior_bank_workspace_bytes(pairs, S, h * w), qry.device, ws_cache, ("prior_bank", pairs, S, h * w))
    _lib.check(lib.pemp_prior_bank_f32(_p(qry), ldq, _p(rows), _p(norms), _p(count), _p(index), _p(out), _p(ws), ws.numel(), n, K, S,
                                       h * w, C, cap, _stream()), "prior_bank")
    return out


def bank_gather_rows(src, index_dev, n, out=None):
    """Rows of a contiguous fp32 table src [K,C] by a bank's selection: ``index_dev`` int32 [n] on the device -> [n,C] =
    src[index[i]]; None -> [n,K,C], every row for every one of the n queries."""
    if src.dim() != 2 or src.dtype != torch.float32 or not src.is_contiguous():
        raise ValueError(f"bank_gather_rows: src must be contiguous fp32 [K,C], got {tuple(src.shape)} {src.dtype}")
    K, C = src.shape
    if index_dev is not None and (index_dev.dtype != torch.int32 or tuple(index_dev.shape) != (n,) or not index_dev.is_contiguous()):
        raise ValueError(f"bank_gather_rows: the device index must be contiguous int32 [{n}]")
    lead = (n,) if index_dev is not None else (n, K)
    lib = _lib.load()
    _chk_dev(src, index_dev, out)
    if out is None:
        out = torch.empty(lead + (C,), dtype=torch.float32, device=src.device)
    if tuple(out.shape) != lead + (C,) or not out.is_contiguous():
        raise ValueError(f"bank_gather_rows: out must be contiguous {list(lead + (C,))}")
    _lib.check(lib.pemp_bank_gather_rows_f32(_p(src), _p(index_dev), _p(out), n, K, C, _stream()), "bank_gather_rows")
    return out


def adaptive_avgpool(x, size, out=None):
    """nn.AdaptiveAvgPool2d(size) on an NHWC view (``out``: an NHWC view, e.g. a channel slice of a wider buffer)."""
    lib = _lib.load()
    _chk_dev(x, out)
    ldx = _nhwc(x, "x")
    n, h, w, c = x.shape
    ho, wo = (size, size) if isinstance(size, int) else size
    if out is None:
        out = torch.empty((n, ho, wo, c), dtype=torch.float32, device=x.device)
    if tuple(out.shape) != (n, ho, wo, c):
        raise ValueError(f"adaptive_avgpool: out {tuple(out.shape)} != {(n, ho, wo, c)}")
    _lib.check(lib.pemp_adaptive_avgpool_nhwc_f32(_p(x), ldx, _p(out), _nhwc(out, "out"), n, h, w, c, ho, wo, _stream()),
               "adaptive_avgpool")
    return out


def _strides4(t, name):
    """(image stride, pixel stride, channel stride) of a 4-D [N, H, W, C] fp32 view whose pixels are evenly spaced."""
    if t.dim() != 4 or t.dtype != torch.float32:
        raise ValueError(f"{name}: expected a 4-D fp32 [N,H,W,C] view, got {tuple(t.shape)} {t.dtype}")
    n, h, w, c = t.shape
    sn, sh, sw, sc = t.stride()
    sp = sw if w > 1 else (sh if h > 1 else 1)
    if (w > 1 and h > 1 and sh != w * sp) or sp <= 0 or sc <= 0 or sn < 0:
        raise ValueError(f"{name}: pixels must be evenly spaced (strides {t.stride()})")
    return sn, sp, sc


def resize_bilinear_ac(x, size, out=None, binarize=False):
    """F.interpolate(x, size, mode="bilinear", align_corners=True) on a [N,H,W,C] view with any strides of the form (image,
    pixel, channel): NHWC channel slices, an [N,H,W,1] view of a mask plane, an NCHW result seen as [N,H,W,C].  ``binarize``:
    read x as (x == 1).  ``out`` None: a new contiguous NHWC tensor."""
    lib = _lib.load()
    _chk_dev(x, out)
    n, hi, wi, c = x.shape
    ho, wo = (size, size) if isinstance(size, int) else size
    if out is None:
        out = torch.empty((n, ho, wo, c), dtype=torch.float32, device=x.device)
    if tuple(out.shape) != (n, ho, wo, c):
        raise ValueError(f"resize_bilinear_ac: out {tuple(out.shape)} != {(n, ho, wo, c)}")
    xn, xp, xc = _strides4(x, "x")
    yn, yp, yc = _strides4(out, "out")
    _lib.check(lib.pemp_resize_bilinear_ac_nhwc_f32(_p(x), xn, xp, xc, _p(out), yn, yp, yc, n, c, hi, wi, ho, wo, int(binarize),
                                                    _stream()), "resize_bilinear_ac")
    return out


def weighted_gap(feat, mask, S, out=None):
    """PFENet's Weighted_GAP (networks/pfenet.py:15-20) averaged over the S shots (:229-233): feat NHWC [B*S,h,w,C], mask
    [B*S,h,w] -> [B,C]."""
    lib = _lib.load()
    _chk_dev(feat, mask, out)
    ldf = _nhwc(feat, "feat")
    n, h, w, c = feat.shape
    if n % S or tuple(mask.shape) != (n, h, w) or not mask.is_contiguous():
        raise ValueError("weighted_gap: mask must be contiguous [B*S,h,w]")
    if out is None:
        out = torch.empty((n // S, c), dtype=torch.float32, device=feat.device)
    if tuple(out.shape) != (n // S, c) or not out.is_contiguous():
        raise ValueError("weighted_gap: out must be contiguous [B,C]")
    _lib.check(lib.pemp_weighted_gap_f32(_p(feat), ldf, _p(mask), _p(out), n // S, S, h, w, c, _stream()), "weighted_gap")
    return out


def scale_add(x, mask=None, residual=None, out=None):
    """out = x * mask[pixel] (+ residual) on NHWC views; ``mask`` contiguous [N,H,W] or None."""
    lib = _lib.load()
    _chk_dev(x, mask, residual, out)
    ldx = _nhwc(x, "x")
    n, h, w, c = x.shape
    if out is None:
        out = torch.empty((n, h, w, c), dtype=torch.float32, device=x.device)
    if tuple(out.shape) != tuple(x.shape) or (residual is not None and tuple(residual.shape) != tuple(x.shape)):
        raise ValueError("scale_add: shape mismatch")
    if mask is not None and (mask.numel() != n * h * w or not mask.is_contiguous()):
        raise ValueError("scale_add: mask must be contiguous [N,H,W]")
    ldr = _nhwc(residual, "residual") if residual is not None else 0
    _lib.check(lib.pemp_scale_add_nhwc_f32(_p(x), ldx, _p(mask), _p(residual), ldr, _p(out), _nhwc(out, "out"), n * h * w, c,
                                           _stream()), "scale_add")
    return out


# -- CANet inference (csrc/canet.hip) -----------------------------------------------------------------------------------------
def canet_support_vector(feat, sup_mask, S, out=None):
    """CANet's support vector (networks/canet.py:175-178): feat NHWC [B*S,h,w,C], sup_mask contiguous fp32 [B*S,2,H,W] (plane 0
    is sampled nearest to h x w) -> [B,C] = mean over the shots of sum(f m) / (sum(m) + 1e-5)."""
    lib = _lib.load()
    _chk_dev(feat, sup_mask, out)
    ldf = _nhwc(feat, "feat")
    n, h, w, c = feat.shape
    if sup_mask.dim() != 4 or n % S or sup_mask.shape[0] != n or sup_mask.shape[1] != 2 or not sup_mask.is_contiguous() \
            or sup_mask.dtype != torch.float32:
        raise ValueError(f"canet_support_vector: sup_mask must be contiguous fp32 [B*S,2,H,W] for feat {tuple(feat.shape)}, S={S}")
    H, W = sup_mask.shape[-2:]
    if out is None:
        out = torch.empty((n // S, c), dtype=torch.float32, device=feat.device)
    if tuple(out.shape) != (n // S, c) or not out.is_contiguous() or out.dtype != torch.float32:
        raise ValueError("canet_support_vector: out must be contiguous fp32 [B,C]")
    _lib.check(lib.pemp_canet_support_vector_f32(_p(feat), ldf, _p(sup_mask), _p(out), n // S, S, h, w, H, W, c, _stream()),
               "canet_support_vector")
    return out


def pack_canet_zweights(w_oihw):
    """The z slice of layer55's weight [Cout,Cin_z,3,3] -> contiguous fp32 [9,Cout,Cin_z] (tap-major, Cin contiguous): the
    operand of ``canet_zterm``.  Packed once, when the engine is built."""
    co, ci, kh, kw = w_oihw.shape
    if (kh, kw) != (3, 3):
        raise ValueError("pack_canet_zweights: a 3x3 kernel is expected")
    return w_oihw.detach().float().permute(2, 3, 0, 1).reshape(9, co, ci).contiguous()


def canet_zterm(wz, z, h, w, dil, out=None, taps=None):
    """The support half of CANet's layer55 (canet.py:179-181) without the broadcast: wz [9,Cout,Cin] (pack_canet_zweights),
    z [B,Cin] -> R NHWC [B,h,w,Cout], the sum over the in-image taps of W_z[tap] z: the ``residual`` of the conv over the query
    channels.  ``taps``: the [B,9,Cout] intermediate (a scratch buffer; returned values are the per-tap products)."""
    lib = _lib.load()
    _chk_dev(wz, z, out, taps)
    if wz.dim() != 3 or wz.shape[0] != 9 or not wz.is_contiguous() or wz.dtype != torch.float32:
        raise ValueError("canet_zterm: wz must be contiguous fp32 [9,Cout,Cin]")
    _, cout, cin = wz.shape
    if z.dim() != 2 or z.shape[1] != cin or not z.is_contiguous() or z.dtype != torch.float32:
        raise ValueError(f"canet_zterm: z must be contiguous fp32 [B,{cin}]")
    b = z.shape[0]
    if taps is None:
        taps = torch.empty((b, 9, cout), dtype=torch.float32, device=z.device)
    if tuple(taps.shape) != (b, 9, cout) or not taps.is_contiguous() or taps.dtype != torch.float32:
        raise ValueError("canet_zterm: taps must be contiguous fp32 [B,9,Cout]")
    if out is None:
        out = torch.empty((b, h, w, cout), dtype=torch.float32, device=z.device)
    if tuple(out.shape) != (b, h, w, cout):
        raise ValueError(f"canet_zterm: out {tuple(out.shape)} != {(b, h, w, cout)}")
    if len({t.data_ptr() for t in (wz, z, taps, out)}) != 4:
        raise ValueError("canet_zterm: wz, z, taps and out must be four different buffers")
    _lib.check(lib.pemp_canet_zterm_f32(_p(wz), _p(z), _p(taps), _p(out), _nhwc(out, "out"), b, h, w, cin, cout, int(dil), _stream()),
               "canet_zterm")
    return out


def canet_block_input(x, out, history=None, slot=None, with_history=None):
    """Input of a CANet residual block (canet.py:103-104,193): out[..., :C] = relu(x); with a history also out[..., C:C+2] =
    relu(history), from ``history`` [B,2,h,w] (slot None) or from row ``slot[b]`` (device int32 [B]; < 0: zeros) of a table
    ``history`` [nslots,2,h,w].  ``with_history`` True with ``history`` None writes zeros (the loader's first history)."""
    lib = _lib.load()
    _chk_dev(x, out, history, slot)
    ldx, ldy = _nhwc(x, "x"), _nhwc(out, "out")
    n, h, w, c = x.shape
    nhist = 2 if (history is not None or with_history) else 0
    if tuple(out.shape[:3]) != (n, h, w) or out.shape[3] < c + nhist:
        raise ValueError(f"canet_block_input: out {tuple(out.shape)} does not take {c} + {nhist} channels of {tuple(x.shape)}")
    nslots = 0
    if history is not None:
        if history.dim() != 4 or tuple(history.shape[1:]) != (2, h, w) or not history.is_contiguous() or history.dtype != torch.float32:
            raise ValueError(f"canet_block_input: history must be contiguous fp32 [rows,2,{h},{w}], got {tuple(history.shape)}")
        nslots = history.shape[0]
        if slot is None and nslots != n:
            raise ValueError(f"canet_block_input: a history tensor has one row per image ({n}), got {nslots}")
    if slot is not None and (history is None or slot.dtype != torch.int32 or tuple(slot.shape) != (n,) or not slot.is_contiguous()):
        raise ValueError("canet_block_input: slot must be a contiguous int32 [B] beside a history table")
    _lib.check(lib.pemp_canet_block_input_f32(_p(x), ldx, _p(history), _p(slot), nslots, _p(out), ldy, n, h * w, c, nhist, _stream()),
               "canet_block_input")
    return out


def canet_history_update(logits, table=None, slot=None, out=None):
    """softmax over the two channels of ``logits`` [B,2,h,w] (entry/canet.py:52) -> row ``slot[b]`` of ``table`` [nslots,2,h,w]
    for every slot[b] >= 0 (entry/canet.py:77-80) and / or ``out`` [B,2,h,w].  No slot may be named twice in one call."""
    lib = _lib.load()
    _chk_dev(logits, table, slot, out)
    if logits.dim() != 4 or logits.shape[1] != 2 or not logits.is_contiguous() or logits.dtype != torch.float32:
        raise ValueError("canet_history_update: logits must be contiguous fp32 [B,2,h,w]")
    b, _, h, w = logits.shape
    if (table is None) != (slot is None) or (table is None and out is None):
        raise ValueError("canet_history_update: a table comes with its slots; a table or ``out`` is needed")
    nslots = 0
    if table is not None:
        if table.dim() != 4 or tuple(table.shape[1:]) != (2, h, w) or not table.is_contiguous() or table.dtype != torch.float32:
            raise ValueError(f"canet_history_update: table must be contiguous fp32 [nslots,2,{h},{w}]")
        if slot.dtype != torch.int32 or tuple(slot.shape) != (b,) or not slot.is_contiguous():
            raise ValueError("canet_history_update: slot must be a contiguous int32 [B]")
        nslots = table.shape[0]
    if out is not None and (tuple(out.shape) != tuple(logits.shape) or not out.is_contiguous() or out.dtype != torch.float32):
        raise ValueError("canet_history_update: out must be contiguous fp32 [B,2,h,w]")
    _lib.check(lib.pemp_canet_history_update_f32(_p(logits), _p(table), _p(slot), nslots, _p(out), b, h * w, _stream()),
               "canet_history_update")
    return out if out is not None else table


# -- RPMMs inference (csrc/rpmms.hip) -----------------------------------------------------------------------------------------
RPMMS_COLS = 10                 # the three mixtures K = 1 | 3 | 6 side by side
RPMMS_GROUPS = ((0, 1), (1, 3), (4, 6))          # (first column, K) of every mixture


def rpmms_em_work_floats(B, h, w, C=256):
    """Size of ``rpmms_em``'s ping-pong workspace (include/pemp_hip.h: 2 halves x B x 2 sides x G slices x (10 C + 16))."""
    g = min(16, -(-(h * w) // 64))
    return 2 * B * 2 * g * (RPMMS_COLS * C + 16)


def rpmms_em(feat, mask, mu0, out=None, work=None, iters=10):
    """The PMMs EM (networks/rpmms.py:65-86,101-117) of all three mixtures, foreground and background, in one pass per iteration
    over the support features: feat NHWC [B,h,w,256], mask contiguous fp32 [B,h,w] (the foreground plane at feature size), mu0
    contiguous fp32 [10,256] -> mu [B,2,10,256] (side 0: foreground, 1: background)."""
    lib = _lib.load()
    _chk_dev(feat, mask, mu0, out, work)
    ldf = _nhwc(feat, "feat")
    b, h, w, c = feat.shape
    if tuple(mask.shape) != (b, h, w) or not mask.is_contiguous() or mask.dtype != torch.float32:
        raise ValueError(f"rpmms_em: mask must be contiguous fp32 [{b},{h},{w}], got {tuple(mask.shape)}")
    if tuple(mu0.shape) != (RPMMS_COLS, c) or not mu0.is_contiguous() or mu0.dtype != torch.float32:
        raise ValueError(f"rpmms_em: mu0 must be contiguous fp32 [{RPMMS_COLS},{c}]")
    if out is None:
        out = torch.empty((b, 2, RPMMS_COLS, c), dtype=torch.float32, device=feat.device)
    if tuple(out.shape) != (b, 2, RPMMS_COLS, c) or not out.is_contiguous() or out.dtype != torch.float32:
        raise ValueError(f"rpmms_em: out must be contiguous fp32 [{b},2,{RPMMS_COLS},{c}]")
    need = rpmms_em_work_floats(b, h, w, c)
    if work is None:
        work = torch.empty(need, dtype=torch.float32, device=feat.device)
    if work.numel() < need or not work.is_contiguous() or work.dtype != torch.float32:
        raise ValueError(f"rpmms_em: work must be a contiguous fp32 buffer of at least {need} elements")
    _lib.check(lib.pemp_rpmms_em_f32(_p(feat), ldf, _p(mask), _p(mu0), _p(work), _p(out), b, h, w, c, int(iters), _stream()), "rpmms_em")
    return out


def _rpmms_groups_out(who, out, b, h, w, c, need):
    """``out`` [3,B,h,w,ld]: one NHWC buffer per mixture, ld >= need -> (pixel stride, mixture stride)."""
    if out.dim() != 5 or tuple(out.shape[:4]) != (3, b, h, w) or out.shape[4] < need or out.dtype != torch.float32:
        raise ValueError(f"{who}: out must be fp32 [3,{b},{h},{w},>={need}], got {tuple(out.shape)}")
    st = out.stride()
    if st[4] != 1 or st[2] != w * st[3] or st[1] != h * w * st[3]:
        raise ValueError(f"{who}: out must be a channel slice of a dense [3,B,h,w,ld] buffer")
    return st[3], st[0]


def rpmms_prob_map(qry, mu, out):
    """The probability maps of the three mixtures (rpmms.py:119-139): qry NHWC [B,h,w,256], mu [B,2,10,256] (``rpmms_em``) ->
    out[g, b, y, x, 256] = P_b, out[g, b, y, x, 257] = P_f; ``out`` [3,B,h,w,ld >= 258], other channels untouched."""
    lib = _lib.load()
    _chk_dev(qry, mu, out)
    ldq = _nhwc(qry, "qry")
    b, h, w, c = qry.shape
    if tuple(mu.shape) != (b, 2, RPMMS_COLS, c) or not mu.is_contiguous() or mu.dtype != torch.float32:
        raise ValueError(f"rpmms_prob_map: mu must be contiguous fp32 [{b},2,{RPMMS_COLS},{c}]")
    ldo, gstride = _rpmms_groups_out("rpmms_prob_map", out, b, h, w, c, c + 2)
    _lib.check(lib.pemp_rpmms_prob_map_f32(_p(qry), ldq, _p(mu), _p(out), ldo, gstride, b, h * w, c, _stream()), "rpmms_prob_map")
    return out


def rpmms_proto_sum(wz, mu, base, bias, out, dil=2, taps=None):
    """Per mixture the sum over its prototypes of layer55(cat(query, prototype)) (rpmms.py:237-244): wz [9,256,256]
    (``pack_canet_zweights`` of the prototype half of the weights), mu [B,2,10,256], base NHWC [B,h,w,256] (the conv of the
    query with the query half, no bias, no ReLU), bias [256] -> out[g, b, y, x, :256]; ``out`` [3,B,h,w,ld >= 256].  ``taps``: the
    [B,10,9,256] intermediate (a scratch buffer)."""
    lib = _lib.load()
    _chk_dev(wz, mu, base, bias, out, taps)
    ldb = _nhwc(base, "base")
    b, h, w, c = base.shape
    if tuple(wz.shape) != (9, c, c) or not wz.is_contiguous() or wz.dtype != torch.float32:
        raise ValueError(f"rpmms_proto_sum: wz must be contiguous fp32 [9,{c},{c}]")
    if tuple(mu.shape) != (b, 2, RPMMS_COLS, c) or not mu.is_contiguous() or mu.dtype != torch.float32:
        raise ValueError(f"rpmms_proto_sum: mu must be contiguous fp32 [{b},2,{RPMMS_COLS},{c}]")
    if tuple(bias.shape) != (c,) or not bias.is_contiguous() or bias.dtype != torch.float32:
        raise ValueError(f"rpmms_proto_sum: bias must be contiguous fp32 [{c}]")
    if taps is None:
        taps = torch.empty((b, RPMMS_COLS, 9, c), dtype=torch.float32, device=base.device)
    if tuple(taps.shape) != (b, RPMMS_COLS, 9, c) or not taps.is_contiguous() or taps.dtype != torch.float32:
        raise ValueError(f"rpmms_proto_sum: taps must be contiguous fp32 [{b},{RPMMS_COLS},9,{c}]")
    ldo, gstride = _rpmms_groups_out("rpmms_proto_sum", out, b, h, w, c, c)
    _lib.check(lib.pemp_rpmms_proto_sum_f32(_p(wz), _p(mu), _p(base), ldb, _p(bias), _p(taps), _p(out), ldo, gstride, b, h, w, c,
                                            int(dil), _stream()), "rpmms_proto_sum")
    return out


# -- RPMMs support banks (pemp_amd.bank.RPMMsBank): what a class's support leaves behind, and a query's meeting with it ----------
def _rpmms_bank_store(who, mu, taps, c):
    if mu.dim() != 4 or tuple(mu.shape[1:]) != (2, RPMMS_COLS, c) or mu.shape[0] < 1 or not mu.is_contiguous() \
            or mu.dtype != torch.float32:
        raise ValueError(f"{who}: mu must be contiguous fp32 [K,2,{RPMMS_COLS},{c}], got {tuple(mu.shape)} {mu.dtype}")
    k = mu.shape[0]
    if taps is not None and (tuple(taps.shape) != (k, RPMMS_COLS, 9, c) or not taps.is_contiguous() or taps.dtype != torch.float32):
        raise ValueError(f"{who}: taps must be contiguous fp32 [{k},{RPMMS_COLS},9,{c}], got {tuple(taps.shape)} {taps.dtype}")
    return k


def rpmms_proto_taps(wz, mu, out=None):
    """The tap products of ``rpmms_proto_sum`` on their own, for the K classes of a bank: wz [9,256,256], mu [K,2,10,256] ->
    taps [K,10,9,256], bit for bit the ``taps`` scratch ``rpmms_proto_sum`` leaves for the same mu."""
    if wz.dim() != 3 or wz.shape[0] != 9 or wz.shape[1] != wz.shape[2] or not wz.is_contiguous() or wz.dtype != torch.float32:
        raise ValueError(f"rpmms_proto_taps: wz must be contiguous fp32 [9,C,C], got {tuple(wz.shape)} {wz.dtype}")
    c = wz.shape[1]
    k = _rpmms_bank_store("rpmms_proto_taps", mu, out, c)
    lib = _lib.load()
    _chk_dev(wz, mu, out)
    if out is None:
        out = torch.empty((k, RPMMS_COLS, 9, c), dtype=torch.float32, device=mu.device)
    _lib.check(lib.pemp_rpmms_proto_taps_f32(_p(wz), _p(mu), _p(out), k, c, _stream()), "rpmms_proto_taps")
    return out


def rpmms_bank_l56(qry, base, bias, mu, taps, out, index=None, dil=2):
    """``rpmms_proto_sum`` + ``rpmms_prob_map`` of N queries against the K classes of a bank in one launch: qry, base NHWC
    [N,h,w,256] (layer5 of the queries and their conv with the query half of layer55), bias [256], mu [K,2,10,256], taps
    [K,10,9,256] (``rpmms_proto_taps``).  ``index`` None: every query against every class, ``out`` [3,N*K,h,w,ld >= 258], pair
    n * K + k; ``index`` (a Python sequence or a CPU integer tensor [N], checked here against 0 <= i < K, then uploaded as int32):
    query n against class index[n], ``out`` [3,N,h,w,ld].  Channels 258.. are not written.  A pair is bit for bit the two
    episode kernels on (qry[n], base[n], mu[k], taps[k])."""
    _rpmms_bank_shapes(qry, base, bias, mu, taps)
    if index is not None:
        index = bank_index(index, qry.shape[0], mu.shape[0])
    _lib.load()
    _chk_dev(qry, base, bias, mu, taps, out)
    if index is not None:
        index = index.to(qry.device, non_blocking=True)
    return _rpmms_bank_l56(qry, base, bias, mu, taps, out, index, dil)


def _rpmms_bank_shapes(qry, base, bias, mu, taps):
    ldq, ldb = _nhwc(qry, "qry"), _nhwc(base, "base")
    c = qry.shape[3]
    if tuple(base.shape) != tuple(qry.shape):
        raise ValueError(f"rpmms_bank_l56: base {tuple(base.shape)} must have qry's shape {tuple(qry.shape)}")
    if tuple(bias.shape) != (c,) or not bias.is_contiguous() or bias.dtype != torch.float32:
        raise ValueError(f"rpmms_bank_l56: bias must be contiguous fp32 [{c}]")
    if taps is None:
        raise ValueError("rpmms_bank_l56: taps must be given (rpmms_proto_taps)")
    _rpmms_bank_store("rpmms_bank_l56", mu, taps, c)
    return ldq, ldb


def _rpmms_bank_l56(qry, base, bias, mu, taps, out, index_dev, dil=2):
    """The launch of ``rpmms_bank_l56``.  ``index_dev``: None or an int32 DEVICE tensor [N] whose values the caller has checked
    on the host (``bank_index``) -- the static index buffer of a captured graph comes in here."""
    ldq, ldb = _rpmms_bank_shapes(qry, base, bias, mu, taps)
    n, h, w, c = qry.shape
    k = mu.shape[0]
    index = index_dev
    if index is not None and (not isinstance(index, torch.Tensor) or not index.is_cuda or index.dtype != torch.int32
                              or tuple(index.shape) != (n,) or not index.is_contiguous()):
        raise ValueError(f"rpmms_bank_l56: the device index must be a contiguous int32 tensor [{n}] on the GPU")
    pairs = n if index is not None else n * k
    ldo, gstride = _rpmms_groups_out("rpmms_bank_l56", out, pairs, h, w, c, c + 2)
    lib = _lib.load()
    _chk_dev(qry, base, bias, mu, taps, index, out)
    _lib.check(lib.pemp_rpmms_bank_l56_f32(_p(qry), ldq, _p(base), ldb, _p(bias), _p(mu), _p(taps), _p(index), _p(out), ldo, gstride,
                                           n, k, h, w, c, int(dil), _stream()), "rpmms_bank_l56")
    return out
