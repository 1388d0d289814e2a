"""Execution engine: walks a parameter tree (pemp_amd.networks.backbones), packs it once into
device-resident KRSC weights + folded per-channel affines, and runs the encoder as a chain of
libpemp_hip.so launches on NHWC activations.

Eval-mode arithmetic only in this round (BatchNorm folded with running statistics exactly like
ATen's eval kernel: alpha = weight * rsqrt(var + eps), beta = bias - mean * alpha; DropBlock and
Dropout2d are identities).  Also what the model engines (canet_engine, pfenet_engine, rpmms_engine) and networks/ share:
the episode packer, the padded-Cin and 2-class packers, the bottleneck walker of both ResNet trunks.
"""
import copy
import os

import torch
import torch.nn as nn

from . import ops
from .ops import ConvParams

BN_EPS = 1e-5

#: The inference engines' convs run on the split3 family (ops.SPLIT3_TILES: fp32 operands as three bf16 pieces on the bf16 MFMA
#: pipe, fp32-accurate) wherever the layer's geometry admits it; False: the fp32-chain kernels.  Read when an engine is built
#: (the models' ``precision("f32_chain")`` builds one with it off).  PEMP_SPLIT3=0 switches the default off.
SPLIT3 = os.environ.get("PEMP_SPLIT3", "1") != "0"


def split3_admits(cp):
    """``with_split3``'s geometry rule for ConvParams.w3: an fp32 non-stem layer of <= 32 taps with Cin % 32 == 0, Cout % 64 == 0
    and an unpadded K."""
    return (cp.w.dtype == torch.float32 and not cp.stem and cp.kh * cp.kw <= 32 and cp.cin % 32 == 0 and cp.cout % 64 == 0
            and cp.kpad == cp.kh * cp.kw * cp.cin)


def with_split3(cp):
    """Attach the split form of the weights when SPLIT3 is on: as ConvParams.w3 to an fp32 layer whose geometry the split3 kernels
    take (<= 32 taps, Cin % 32, Cout % 64), and as ConvParams.w3pool to the 7x7 / stride 2 / pad 3 NHWC4 stem, which then runs
    fused with its max-pool (ops.stem_pool; a stem launched on its own by ops.conv2d stays on the fp32 chain, its w3 stays None).
    Every other layer stays on the fp32 chain."""
    if not SPLIT3 or cp.w.dtype != torch.float32:
        return cp
    if cp.stem:
        if (cp.kh, cp.kw, cp.stride, cp.pad, cp.dil) == (7, 7, 2, 3, 1) and cp.kpad == 224 and cp.cout % 64 == 0:
            cp.w3pool = ops.pack_split3(cp.w)
    elif split3_admits(cp):
        cp.w3 = ops.pack_split3(cp.w)
    return cp


def bn_affine(bn):
    """(alpha, beta) of an eval-mode BatchNorm2d, fp32, on the BN's device."""
    invstd = 1.0 / torch.sqrt(bn.running_var.detach().float() + bn.eps)
    alpha = bn.weight.detach().float() * invstd
    beta = bn.bias.detach().float() - bn.running_mean.detach().float() * alpha
    return alpha.contiguous(), beta.contiguous()


def conv_params(conv, bn=None, relu=False, stem4=False, in_slice=None, dtype=torch.float32):
    """Pack one nn.Conv2d (+ following BN) for pemp_conv2d_nhwc_f32 (``dtype`` bfloat16: the weights of the bf16 side-figure
    variant; the folded affine stays fp32)."""
    w = conv.weight.detach()
    if in_slice is not None:
        w = w[:, in_slice[0]:in_slice[1]]
    packed, kpad = ops.pack_conv_weight(w, stem4=stem4)
    cout, cin = w.shape[0], w.shape[1]
    scale = shift = None
    if bn is not None:
        scale, shift = bn_affine(bn)
        if conv.bias is not None:
            shift = shift + conv.bias.detach().float() * scale
    elif conv.bias is not None:
        shift = conv.bias.detach().float().contiguous()
    return with_split3(ConvParams(packed.contiguous().to(dtype), scale, shift, 4 if stem4 else cin, cout, conv.kernel_size[0],
                                  conv.kernel_size[1], conv.stride[0], conv.padding[0], conv.dilation[0], kpad, stem4, relu))


def pack_padded_in(conv, cin_pad, relu):
    """[Cout, C, k, k] -> KRSC over ``cin_pad`` input channels (zero weights on the padding channels: the conv engine takes
    Cin % 32 == 0)."""
    w = conv.weight.detach().float()
    co, ci, kh, kw = w.shape
    wp = torch.zeros((co, kh, kw, cin_pad), dtype=torch.float32, device=w.device)
    wp[..., :ci] = w.permute(0, 2, 3, 1)
    return with_split3(ConvParams(wp.reshape(co, kh * kw * cin_pad).contiguous(), None, conv.bias.detach().float().contiguous(),
                                  cin_pad, co, kh, kw, 1, conv.padding[0], conv.dilation[0], kh * kw * cin_pad, False, relu))


def classifier2(conv):
    """A C -> 2 1x1 classifier conv packed with 62 zero output channels (the conv engine takes Cout % 64 == 0)."""
    cin, dev = conv.weight.shape[1], conv.weight.device
    w = torch.zeros((64, cin), dtype=torch.float32, device=dev)
    w[:2] = conv.weight.detach().float()[:, :, 0, 0]
    b = torch.zeros(64, dtype=torch.float32, device=dev)
    b[:2] = conv.bias.detach().float()
    return with_split3(ConvParams(w.contiguous(), None, b.contiguous(), cin, 64, 1, 1, 1, 0, 1, cin, False, False))


def logits_nchw(c, pred):
    """The two live channels of ``classifier2``'s [B,h,w,64] output -> NCHW logits ``pred`` [B,2,h,w] (identity resize: exact)."""
    ops.resize_bilinear_ac(c[..., :2], tuple(c.shape[1:3]), out=pred.permute(0, 2, 3, 1))
    return pred


def pack_episode(arena, groups, priors=None):
    """Image groups [n_i,3,H,W] (supports first, then queries), each with its prior planes [n_i,H,W] when ``priors`` is given
    -> the arena's NHWC4 input buffer ``x4`` [sum n_i,H,W,4], one ``ops.pack_input`` per group."""
    H, W = groups[0].shape[-2:]
    x4 = arena.get("x4", (sum(g.shape[0] for g in groups), H, W, 4), torch.float32)
    o = 0
    for i, g in enumerate(groups):
        ops.pack_input(g.contiguous(), None if priors is None else priors[i], out=x4[o:o + g.shape[0]])
        o += g.shape[0]
    return x4


#: Steps of at most this many feature rows (one or two episodes: 5202 rows per 1-shot episode) issue their INDEPENDENT convs
#: as ONE grouped launch (ops.conv2d_group): the dilated ASPP branches, a stage's downsample conv beside its conv1.  A
#: 5202-row conv is 41-82 tiles on 256 CUs; grouped, the members fill the chip without splitting K and without a launch +
#: drain each.  Same tiles, same K order: results do not change.  PEMP_EVAL_GROUP_ROWS=0 switches it off.
GROUP_MAX_ROWS = int(os.environ.get("PEMP_EVAL_GROUP_ROWS", "12000"))


#: Output widths at which a single-reader conv -> 3x3 conv pair hands its intermediate tensor over PRE-SPLIT (the producer's epilogue
#: writes the split3 pieces, the consumer's K loop has no splitting left: ops.conv2d out_split3 / x_split3, DESIGN.md "Pre-split
#: activations").  A width is listed where the consumer's pre-split form beat the layer's best fp32-input id when measured.
PRESPLIT_WIDTHS = (128, 256)
#: ... and only where the consumer has at least this many 256 x 128 tiles (None: one per CU).  The pre-split form has that one block
#: shape; a one-episode step (5202 rows: 42 tiles on 256 CUs) ran 13 % slower with it than on the small tiles of the fp32-input ids.
PRESPLIT_MIN_TILES = None


def presplit_pair(prod, cons, x, rows, enabled=True):
    """Whether ``prod`` (fed ``x``) may hand its output to its ONLY reader ``cons`` (``rows`` output rows) pre-split: both split3
    layers on fp32 activations, ``cons`` multi-tap with a pre-split form for its width, enough tiles to fill the chip.
    PEMP_SPLIT3_PRESPLIT=0 withholds it."""
    if not (enabled and ops.SPLIT3_PRESPLIT and x.dtype == torch.float32 and x.is_cuda and prod.w3 is not None and cons.w3 is not None
            and not prod.stem and cons.kh * cons.kw > 1 and cons.cin % 32 == 0 and cons.cout % 128 == 0 and cons.cout in PRESPLIT_WIDTHS):
        return False
    least = torch.cuda.get_device_properties(x.device).multi_processor_count if PRESPLIT_MIN_TILES is None else PRESPLIT_MIN_TILES
    return -(-rows // 256) * (cons.cout // 128) >= least


#: p3's output has five readers: the three dilated ASPP branches, the 1x1 branch and the global pool.  With this on, p3 writes it
#: twice -- fp32 and pre-split (ops.conv2d also_split3) -- and the dilated branches read the split copy; the other readers keep the
#: fp32 one.  DESIGN.md "Pre-split activations" has what was measured; False leaves the kernels in place and the engines off them.
PRESPLIT_ASPP = True


#: Row pruning (DESIGN.md "Row pruning").  Where a stage's output is read by the next stage's stride-2 1x1 convs alone (block 0's
#: conv1 and downsample conv: torchvision v1 puts the stride there), three quarters of its rows are never read.  ResNetEngine.forward
#: then runs the stage's LAST block on the even grid only: conv2 at twice its stride, conv3 on the compact tensor with the block input
#: as a stride-2 residual (ops.conv2d residual_stride=2), and the next block 0 at stride 1 on the compact tensor.  Same dot products:
#: the step's results do not change by a bit.  PEMP_PRUNE_ROWS=0 restores the full block (the A/B switch).
PRUNE_ROWS = os.environ.get("PEMP_PRUNE_ROWS", "1") != "0"


def restrided(cp, stride):
    """``cp`` at another stride: a ConvParams that shares its tensors."""
    return ConvParams(cp.w, cp.scale, cp.shift, cp.cin, cp.cout, cp.kh, cp.kw, stride, cp.pad, cp.dil, cp.kpad, cp.stem, cp.relu,
                      cp.w3, cp.w3pool)


def presplit_readers(prod, readers, x, rows, enabled=True):
    """Whether ``prod`` (fed ``x``) may write a second, pre-split copy of its output for the multi-tap layers among ``readers``:
    every one of them qualifies under ``presplit_pair``'s rule."""
    multi = [c for c in readers if c.kh * c.kw > 1]
    return bool(multi) and all(presplit_pair(prod, c, x, rows, enabled and PRESPLIT_ASPP) for c in multi)


class Arena:
    """Named activation buffers reused across calls (static addresses make hipGraph replay valid)."""

    def __init__(self, device, dtype=torch.float32):
        self.device = device
        self.dtype = dtype            # activations between the stem and the encoder's last layer (bfloat16: the side-figure variant)
        self.bufs = {}
        self.ws = {}

    def get(self, name, shape, dtype=None, zero=False):
        """``zero``: cleared ONCE, when the buffer is created (for buffers with regions nobody writes afterwards).
        ``dtype`` None: the arena's activation dtype."""
        dtype = self.dtype if dtype is None else dtype
        key = (name, tuple(shape), dtype)
        t = self.bufs.get(key)
        if t is None:
            t = (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=self.device)
            self.bufs[key] = t
        return t


class _BlockPlan:
    def __init__(self, blk, extra_in=0, dtype=torch.float32):
        # extra_in: the CM variant's two spatially-constant channels are applied as a per-image
        # bias (see ResNetCMEngine), so the packed weights cover only the real channels.
        sl = None
        if extra_in:
            sl = (0, blk.conv1.weight.shape[1] - extra_in)
        self.c1 = conv_params(blk.conv1, blk.bn1, relu=True, in_slice=sl, dtype=dtype)
        self.c2 = conv_params(blk.conv2, blk.bn2, relu=True, dtype=dtype)
        self.c3 = conv_params(blk.conv3, blk.bn3, relu=True, dtype=dtype)     # relu after the residual add
        self.ds = conv_params(blk.downsample[0], blk.downsample[1], relu=False, in_slice=sl, dtype=dtype) \
            if blk.downsample is not None else None
        if extra_in:
            # weights of the extra channels, pre-multiplied by the BN alpha: [Cout, extra]
            self.c1_extra = (blk.conv1.weight.detach()[:, sl[1]:, 0, 0].float() * self.c1.scale[:, None]).contiguous()
            self.ds_extra = (blk.downsample[0].weight.detach()[:, sl[1]:, 0, 0].float() * self.ds.scale[:, None]).contiguous()


class _BottleneckTrunk:
    """The bottleneck walker of both ResNet trunks: stride on conv1 (torchvision v1, ResNetEngine) or on conv2 (pfe_resent v1.5,
    pfenet_engine.DeepBaseResNetEngine)."""
    #: a block's conv1 and downsample conv go out as one grouped launch on small steps.  The deep-base trunk launches them one
    #: by one: switching the grouping on there changes PFENet's speed and is therefore a change of its own.
    GROUP_DS = True
    #: conv1 hands y1 to conv2 pre-split (presplit_pair).  Off on the deep-base trunk for the same reason.
    PRESPLIT = True

    def _block(self, x, bp, tag, c1_shift=None, ds_shift=None, out=None, prune=False):
        """``out``: where the block's result goes (an NHWC view, e.g. a channel slice of a wider buffer); None: the arena's
        ping-pong buffer of ``tag``.  ``prune`` (a block without a downsample conv whose only readers are stride-2 1x1 convs): only
        the output rows on the even grid are computed -- conv2 at twice its stride, conv3 with ``x`` as a stride-2 residual -- and
        the compact tensor is returned."""
        if prune:
            bp = self._pruned_plan(bp)
        a = self.arena
        n, h, w, _ = x.shape
        h1, w1 = (ops.conv_out_size(v, k, bp.c1.stride, bp.c1.pad, bp.c1.dil) for v, k in ((h, bp.c1.kh), (w, bp.c1.kw)))
        ho, wo = (ops.conv_out_size(v, k, bp.c2.stride, bp.c2.pad, bp.c2.dil) for v, k in ((h1, bp.c2.kh), (w1, bp.c2.kw)))
        if out is None:
            out = a.get(("blk", tag), (n, ho, wo, bp.c3.cout))
        res = a.get("res", (n, ho, wo, bp.ds.cout)) if bp.ds is not None else x
        # small step: conv1 and the downsample conv read the same x -- one grouped launch
        grouped = self.GROUP_DS and bp.ds is not None and c1_shift is None and ds_shift is None \
            and 0 < n * ho * wo <= GROUP_MAX_ROWS and x.dtype == torch.float32
        pre = presplit_pair(bp.c1, bp.c2, x, n * ho * wo, self.PRESPLIT and not grouped)       # y1 has one reader: conv2
        y1 = a.get("y1s", ops.split3_shape(n, h1, w1, bp.c1.cout), torch.bfloat16) if pre else a.get("y1", (n, h1, w1, bp.c1.cout))
        if grouped:
            ops.conv2d_group([x, x], [bp.c1, bp.ds], [y1, res])
        else:
            ops.conv2d(x, bp.c1, out=y1, shift_override=c1_shift, per_image_shift=c1_shift is not None, out_split3=pre)
        y2 = ops.conv2d(y1, bp.c2, out=a.get("y2", (n, ho, wo, bp.c2.cout)), x_split3=pre)
        if bp.ds is not None and not grouped:
            ops.conv2d(x, bp.ds, out=res, shift_override=ds_shift, per_image_shift=ds_shift is not None)
        return ops.conv2d(y2, bp.c3, out=out, residual=res, residual_stride=2 if prune else 1)

    def _plan_copy(self, bp, what, **convs):
        """``bp`` with the layers ``convs`` replaced: made once per block and kept (the layers share their tensors with ``bp``'s)."""
        cache = self.__dict__.setdefault("_plan_copies", {})
        key = (id(bp), what)
        if key not in cache:
            q = copy.copy(bp)
            for name, cp in convs.items():
                setattr(q, name, cp)
            cache[key] = (bp, q)            # (bp is kept alive: its id stays its own)
        return cache[key][1]

    def _pruned_plan(self, bp):
        """The last block of a pruned stage: conv2 at twice its stride."""
        if bp.ds is not None:
            raise ValueError("row pruning: the block has a downsample conv of its own")
        return self._plan_copy(bp, "pruned", c2=restrided(bp.c2, 2 * bp.c2.stride))

    def _compact_plan(self, bp):
        """Block 0 behind a pruned stage: its stride-2 conv1 and downsample conv read the compact tensor at stride 1."""
        return self._plan_copy(bp, "compact", c1=restrided(bp.c1, 1), ds=restrided(bp.ds, 1))

    def _stage(self, x, si, final_out=None, compact_in=False, prune=False):
        """Stage ``si``; ``final_out``: an NHWC view its last block writes to (e.g. a channel slice of a wider buffer).
        ``compact_in``: ``x`` comes from a pruned stage (only the rows block 0's stride-2 convs read); ``prune``: the stage's last
        block computes only the rows the next stage reads (``_prunes``)."""
        blocks = self.stages[si]
        for bi, bp in enumerate(blocks):
            last = bi == len(blocks) - 1
            if bi == 0 and compact_in:
                bp = self._compact_plan(bp)
            x = self._block(x, bp, (si, bi & 1), out=final_out if last else None, prune=prune and last)
        return x

    def _prunes(self, si, stage_outs=None):
        """Whether stage ``si``'s output may be computed on the even grid only: a split3 engine on an fp32 arena, nobody but the next
        stage reads the output, that stage's block 0 reads it through two 1x1 / pad 0 / stride 2 convs, the last block of ``si`` adds
        its own input (no downsample conv) behind a 1x1 conv3, and a tile id takes the strided residual for that conv."""
        if not PRUNE_ROWS or self.arena.dtype != torch.float32 or si + 1 >= len(self.stages) or (stage_outs and si in stage_outs):
            return False
        last, nxt = self.stages[si][-1], self.stages[si + 1][0]
        if len(self.stages[si]) < 2 or last.ds is not None or nxt.ds is None:
            return False
        if any(c.w3 is None for c in (last.c1, last.c2, last.c3, nxt.c1, nxt.ds)):
            return False
        if any((c.kh, c.kw, c.pad, c.stride) != (1, 1, 0, 2) for c in (nxt.c1, nxt.ds)):
            return False
        return (last.c3.kh, last.c3.kw, last.c3.pad, last.c3.stride) == (1, 1, 0, 1) and bool(ops.res_s2_tiles(last.c3))


class ResNetEngine(_BottleneckTrunk):
    """ResNet trunk (reference: networks/backbones.py:124-136)."""

    def __init__(self, prm, arena):
        self.arena = arena
        self.stem = conv_params(prm.conv1, prm.bn1, relu=True, stem4=True)
        self.stages = []
        for name in ("layer1", "layer2", "layer3"):
            self.stages.append([_BlockPlan(b, dtype=arena.dtype) for b in getattr(prm, name)])

    def stem_forward(self, x4):
        a = self.arena
        n, h, w, _ = x4.shape
        ho, wo = ops.conv_out_size(h, 7, 2, 3, 1), ops.conv_out_size(w, 7, 2, 3, 1)
        if a.dtype == torch.float32 and ops.stem_pool_supported(self.stem):
            # split3 engines: conv + pool in one launch, only the pooled tensor is written (no "stem" buffer)
            hp, wp = ops._pool_out(ho, 3, 2, 1, True), ops._pool_out(wo, 3, 2, 1, True)
            return ops.stem_pool(x4, self.stem, out=a.get("pool", (n, hp, wp, 64), torch.float32))
        y = ops.conv2d(x4, self.stem, out=a.get("stem", (n, ho, wo, 64), torch.float32))
        hp, wp = ops._pool_out(ho, 3, 2, 1, True), ops._pool_out(wo, 3, 2, 1, True)
        x = ops.maxpool2d(y, 3, 2, 1, ceil_mode=True, out=a.get("pool", (n, hp, wp, 64), torch.float32))
        if a.dtype != torch.float32:       # bf16 variant: the fp32 stem + pool hand over a bf16 copy
            x = ops.convert(x, a.get("pool16", (n, hp, wp, 64)))
        return x

    def forward(self, x4, stage_outs=None):
        """``stage_outs`` {stage index: NHWC view}: the last block of that stage writes there (CANet: layer2 and layer3 into
        the channel slices of one buffer, so that their concatenation is never formed)."""
        x = self.stem_forward(x4)
        pruned = False                  # x holds only the rows the next stage's stride-2 convs read (PRUNE_ROWS)
        for si in range(len(self.stages)):
            prune = self._prunes(si, stage_outs)
            x = self._stage(x, si, stage_outs.get(si) if stage_outs else None, compact_in=pruned, prune=prune)
            pruned = prune
        return x


class ResNetCMEngine(ResNetEngine):
    """ResNetCM (reference: networks/backbones.py:208-247).

    The communication module appends two channels that are CONSTANT over space (and over the
    S+Q images of an episode) before each stage.  A 1x1 conv over a constant channel is a
    per-image bias, so instead of concatenating, the first block of each stage receives
    ``shift[img][co] = beta[co] + alpha[co] * sum_e W[co][C+e] * feat[img][e]``.
    """

    def __init__(self, prm, arena):
        self.arena = arena
        self.spq = prm.spq
        self.stem = conv_params(prm.conv1, prm.bn1, relu=True, stem4=True)
        self.stages = []
        for name in ("layer1", "layer2", "layer3"):
            blocks = list(getattr(prm, name))
            self.stages.append([_BlockPlan(blocks[0], extra_in=2)] + [_BlockPlan(b) for b in blocks[1:]])
        self.lin = [(l.weight.detach().float().contiguous(), l.bias.detach().float().contiguous())
                    for l in (prm.linear1, prm.linear2, prm.linear3)]
        self.group = None   # LongTensor [N]: episode id of every image (set by the caller)

    def _comm(self, x, mask, lin, stride):
        """-> (feat [episodes,2], pooled mask): statistics, episode mean and the 2C -> 2 Linear on HIP kernels."""
        mask, stat = ops.cm_reduce(x, mask, stride)
        _, feat = ops.cm_linear(stat, self.group, lin[0], lin[1], self.n_groups)
        return feat, mask

    def forward(self, x4, prior):
        """x4: NHWC4 input (RGB + prior); prior: [N,H,W] fp32 mask plane."""
        mask = ops.cm_reduce(None, prior, 2)[0]                       # backbones.py:227
        x = self.stem_forward(x4)
        strides = (2, 1, 2)                                           # backbones.py:230,235,240
        for si, blocks in enumerate(self.stages):
            feat, mask = self._comm(x, mask, self.lin[si], strides[si])
            b0 = blocks[0]
            c1_shift = ops.cm_bias(feat, self.group, b0.c1_extra, base=b0.c1.shift)
            ds_shift = ops.cm_bias(feat, self.group, b0.ds_extra, base=b0.ds.shift)
            x = self._block(x, b0, (si, 0), c1_shift, ds_shift)
            for bi, bp in enumerate(blocks[1:], start=1):
                x = self._block(x, bp, (si, bi & 1))
        return x


class VGG16CMEngine:
    """VGG16CM (reference: networks/backbones.py:424-500).

    Unlike ResNetCM, whose communication channels enter 1x1 convs (a per-image bias), here they enter zero-padded 3x3
    convs: at the image border some taps of the constant planes read padding, so their contribution is not constant
    over space.  They are therefore really concatenated: every stage's pooled output is written into the first C
    channels of a [N,h,w,C+32] buffer (the max-pool kernel takes an output stride), the two broadcast values into
    channels C, C+1, and the next stage's first conv runs over C+32 input channels with zero weights on the 30 padding
    channels (the conv engine wants Cin % 32 == 0): 50 / 25 / 12 / 6 % more K on four of the thirteen convs."""
    PADC = 32

    def __init__(self, prm, arena):
        from .networks.backbones import VGG_CM_LAYOUT
        self.arena, self.spq = arena, prm.spq
        self.stages = []
        first = True
        for si, (name, nconv, cout, d, pool) in enumerate(VGG_CM_LAYOUT):
            seq = getattr(prm, name)
            convs = []
            for k in range(nconv):
                conv = seq[2 * k]
                relu = not (pool is None and k == nconv - 1 and not prm.last_relu)
                if k == 0 and not first:
                    convs.append(pack_padded_in(conv, conv.weight.shape[1] - 2 + self.PADC, relu))
                else:
                    convs.append(conv_params(conv, None, relu=relu, stem4=first and k == 0))
            self.stages.append((convs, cout, pool))
            first = False
        self.lin = [(l.weight.detach().float().contiguous(), l.bias.detach().float().contiguous())
                    for l in (prm.linear1, prm.linear2, prm.linear3, prm.linear4)]
        self.group, self.n_groups = None, 0

    def forward(self, x4, prior):
        """x4: NHWC4 input (RGB + prior); prior: [N,H,W] fp32 mask plane -> NHWC features [N,h,w,512]."""
        a = self.arena
        x, mask = x4, prior
        for si, (convs, cout, pool) in enumerate(self.stages):
            for k, cp in enumerate(convs):
                n, h, w, _ = x.shape
                x = ops.conv2d(x, cp, out=a.get(("vcm", si, k & 1), (n, h, w, cp.cout)))
            if pool is None:
                return x
            n, h, w, c = x.shape
            ho, wo = ops._pool_out(h, 3, pool, 1, False), ops._pool_out(w, 3, pool, 1, False)
            wide = a.get(("vcm_cat", si), (n, ho, wo, c + self.PADC), zero=True)      # padding channels stay zero
            xs = ops.maxpool2d(x, 3, pool, 1, out=wide[..., :c])
            mask, stat = ops.cm_reduce(xs, mask, pool)                                # comm: mask pooled with the stage's stride
            _, feat = ops.cm_linear(stat, self.group, self.lin[si][0], self.lin[si][1], self.n_groups)
            wide[..., c:c + 2] = feat.index_select(0, self.group.long()).view(n, 1, 1, 2)   # broadcast over space (and the episode)
            x = wide
        return x


class ASPPV2Engine:
    """purifier.6 of stage 1 (reference: networks/backbones.py:359-369)."""

    def __init__(self, prm, arena):
        self.arena = arena
        self.bn = [bn_affine(getattr(prm, f"aspp_{i}")[0]) for i in range(5)]
        self.br = [conv_params(getattr(prm, f"aspp_{i}")[2], None, relu=True) for i in range(5)]
        midc = self.br[0].cout
        l6 = prm.layer6
        # layer6 split: columns of the broadcast global branch -> per-image bias; the rest -> 1x1 conv
        self.l6_global = conv_params(l6, None, relu=False, in_slice=(0, midc))
        self.l6_main = conv_params(l6, None, relu=False, in_slice=(midc, 5 * midc))
        self.l6_main.shift = None
        self.midc = midc
        # The BatchNorm in front of every branch folds into its conv: W*s, bias + sum_taps W t, and -- because the
        # reference zero-pads the BN OUTPUT -- out-of-image taps of the dilated convs read -t/s (ops.fold_input_affine).
        # That removes the pass that wrote four normalised copies of x (20 % of the non-conv time of an eval step).
        # PEMP_ASPP_COPIES=1 (or a zero BN scale) keeps the copy path.
        folded = [ops.fold_input_affine(self.br[i], *self.bn[i]) for i in range(5)]
        self.folded = None if (os.environ.get("PEMP_ASPP_COPIES") or any(f is None for f in folded)) else folded
        self._tails = set()
        if arena.dtype != torch.float32:
            # bf16 variant: the four spatial branches and layer6's main part take bf16 operands (folded in fp32 first, then
            # rounded once); the global branch works on [n, 1, 1, c] and stays fp32
            if self.folded is None:
                raise ValueError("the bf16 variant needs the folded ASPPV2 branches (non-zero BatchNorm scales)")
            for q, _ in self.folded[1:]:
                q.w = q.w.to(arena.dtype)
            self.l6_main.w = self.l6_main.w.to(arena.dtype)

    def branches(self):
        """The four spatial branch layers as ``forward`` runs them, or None on the copy path / the bf16 variant."""
        if self.folded is None or self.arena.dtype != torch.float32:
            return None
        return [self.folded[i + 1][0] for i in range(4)]

    def forward(self, x, tail=None, xs=None, tail_s=None):
        """``tail`` [>= 4, c]: spare rows right behind ``x`` in the same allocation; the padding vectors are parked there
        (once per buffer) so that the buffer-addressed conv kernels reach them through the activations' descriptor.
        ``xs`` / ``tail_s`` [>= 4, c / 32, 3, 32]: the pre-split copy of ``x`` and the spare rows behind it; the multi-tap branches
        then read ``xs``, with the split of their padding vectors parked in ``tail_s`` the same way."""
        a = self.arena
        n, h, w, c = x.shape
        midc = self.midc
        f32 = torch.float32
        x32 = x if x.dtype == f32 else ops.convert(x, a.get("aspp_x32", (n, h, w, c), f32))     # bf16 variant: the pooling reads fp32
        g = ops.global_avgpool(x32, out=a.get("gap", (n, c), f32))
        cat = a.get("aspp_cat", (n, h, w, 4 * midc))
        if self.folded is not None:
            g2 = ops.conv2d(g.view(n, 1, 1, c), self.folded[0][0], out=a.get("gap_c", (n, 1, 1, midc), f32))
            bias6 = ops.conv2d(g2, self.l6_global, out=a.get("bias6", (n, 1, 1, self.l6_global.cout), f32))
            if tail is not None and tail.data_ptr() not in self._tails:
                for i in range(4):
                    tail[i].copy_(self.folded[i + 1][1])
                self._tails.add(tail.data_ptr())
            qs = [self.folded[i + 1][0] for i in range(4)]
            pvs = [tail[i] if tail is not None else self.folded[i + 1][1] for i in range(4)]
            outs = [cat[..., i * midc:(i + 1) * midc] for i in range(4)]
            if xs is not None:
                if tail_s.data_ptr() not in self._tails:
                    for i in range(4):          # the ABI's padding value of a pre-split input: the [Cin / 32][3][32] split of the fp32 vector
                        tail_s[i].copy_(ops.pack_split3(self.folded[i + 1][1].view(1, c))[0])
                    self._tails.add(tail_s.data_ptr())
                for i in range(4):
                    if qs[i].kh * qs[i].kw > 1:
                        ops.conv2d(xs, qs[i], out=outs[i], pad_value=tail_s[i], x_split3=True)
                    else:
                        ops.conv2d(x, qs[i], out=outs[i])
            elif tail is not None and 0 < n * h * w <= GROUP_MAX_ROWS and x.dtype == f32:
                # small step: the four branches read the same x -- one grouped launch, the dilated 3x3 convs first (their
                # tiles are the long ones; the 1x1 branch's short tiles fill in behind them)
                order = sorted(range(4), key=lambda i: -qs[i].kh * qs[i].kw)
                ops.conv2d_group([x] * 4, [qs[i] for i in order], [outs[i] for i in order], pad_values=[pvs[i] for i in order])
            else:
                for i in range(4):
                    ops.conv2d(x, qs[i], out=outs[i], pad_value=pvs[i] if qs[i].kh * qs[i].kw > 1 else None)
            return ops.conv2d(cat, self.l6_main, out=a.get("feat", (n, h, w, self.l6_main.cout), f32),
                              shift_override=bias6.view(n, -1), per_image_shift=True)
        gb = a.get("gap_bn", (n, c))
        ops.channel_affine_multi(g, [self.bn[0][0]], [self.bn[0][1]], [gb])
        g2 = ops.conv2d(gb.view(n, 1, 1, c), self.br[0], out=a.get("gap_c", (n, 1, 1, midc)))
        bias6 = ops.conv2d(g2, self.l6_global, out=a.get("bias6", (n, 1, 1, self.l6_global.cout)))
        xb = [a.get(("aspp_in", i), (n, h, w, c)) for i in range(4)]
        ops.channel_affine_multi(x, [s for s, _ in self.bn[1:]], [t for _, t in self.bn[1:]], xb)
        for i in range(4):
            ops.conv2d(xb[i], self.br[i + 1], out=cat[..., i * midc:(i + 1) * midc])
        return ops.conv2d(cat, self.l6_main, out=a.get("feat", (n, h, w, self.l6_main.cout)),
                          shift_override=bias6.view(n, -1), per_image_shift=True)


class ASPPEngine:
    """purifier.6 of stage 2: conv -> ReLU per branch, no BN (reference: backbones.py:310-321).  ``out_relu``: a ReLU behind
    ``layer6`` (CANet's ASPP, networks/canet.py:96-100)."""

    def __init__(self, prm, arena, out_relu=False):
        self.arena = arena
        self.br = [conv_params(getattr(prm, f"aspp_{i}")[0], None, relu=True) for i in range(5)]
        midc = self.br[0].cout
        self.l6_global = conv_params(prm.layer6, None, relu=False, in_slice=(0, midc))
        self.l6_main = conv_params(prm.layer6, None, relu=out_relu, in_slice=(midc, 5 * midc))
        self.l6_main.shift = None
        self.midc = midc

    def branches(self):
        return self.br[1:] if self.arena.dtype == torch.float32 else None

    def forward(self, x, xs=None):
        """``xs``: the pre-split copy of ``x``; the multi-tap branches then read it."""
        a = self.arena
        n, h, w, c = x.shape
        midc = self.midc
        g = ops.global_avgpool(x, out=a.get("gap", (n, c)))
        g2 = ops.conv2d(g.view(n, 1, 1, c), self.br[0], out=a.get("gap_c", (n, 1, 1, midc)))
        bias6 = ops.conv2d(g2, self.l6_global, out=a.get("bias6", (n, 1, 1, self.l6_global.cout)))
        cat = a.get("aspp_cat", (n, h, w, 4 * midc))
        outs = [cat[..., i * midc:(i + 1) * midc] for i in range(4)]
        if xs is not None:
            for i in range(4):
                multi = self.br[i + 1].kh * self.br[i + 1].kw > 1
                ops.conv2d(xs if multi else x, self.br[i + 1], out=outs[i], x_split3=multi)
        elif 0 < n * h * w <= GROUP_MAX_ROWS:          # small step: one grouped launch (see ASPPV2Engine.forward)
            order = sorted(range(4), key=lambda i: -self.br[i + 1].kh * self.br[i + 1].kw)
            ops.conv2d_group([x] * 4, [self.br[i + 1] for i in order], [outs[i] for i in order])
        else:
            for i in range(4):
                ops.conv2d(x, self.br[i + 1], out=outs[i])
        return ops.conv2d(cat, self.l6_main, out=a.get("feat", (n, h, w, self.l6_main.cout)),
                          shift_override=bias6.view(n, -1), per_image_shift=True)


class PurifierEngine:
    def __init__(self, seq, arena):
        self.arena = arena
        self.p0 = conv_params(seq[0], None, relu=True, dtype=arena.dtype)
        self.p3 = conv_params(seq[3], None, relu=True, dtype=arena.dtype)
        aspp = seq[6]
        self.aspp = ASPPV2Engine(aspp, arena) if isinstance(aspp.aspp_0[0], nn.BatchNorm2d) else ASPPEngine(aspp, arena)

    def forward(self, x):
        a = self.arena
        n, h, w, _ = x.shape
        pre = presplit_pair(self.p0, self.p3, x, n * h * w)         # p0's output has one reader: p3
        y = ops.conv2d(x, self.p0, out_split3=pre, out=a.get("pur0s", ops.split3_shape(n, h, w, self.p0.cout), torch.bfloat16) if pre
                       else a.get("pur0", (n, h, w, self.p0.cout)))
        # the ASPP input carries 8 spare pixel rows behind it: the folded-BatchNorm branches keep their per-channel
        # padding vectors there, inside the buffer-descriptor window of the tensor (conv_dma2.hip, PADV)
        # The kernels reach a padding vector at a non-negative offset from the first tap, so it must sit at least dil * (w + 1)
        # pixel rows behind the start of the map (ops._group_member_ok).  Behind the map itself that holds unless the map is
        # small: ONE 13 x 13 image under dilation 18 -- a one-image pass is what a prototype bank's enroll / segment make.  `gap`
        # unused rows then push the vectors out far enough, so that such a pass runs the split3 kernels too and equals, bit for
        # bit, the same image inside a larger batch (without them it fell back to the fp32 chain).  0 for every larger map.
        c = self.p3.cout
        reach = max([q.dil for q in (self.aspp.branches() or []) if q.kh * q.kw > 1] or [0]) if isinstance(self.aspp, ASPPV2Engine) else 0
        gap = max(0, reach * (w + 1) - n * h * w)
        flat = a.get("pur3+tail", (n * h * w + gap + 8, c), zero=gap > 0)             # nobody writes the gap rows
        # p3's output has five readers.  Where the dilated ASPP branches qualify (presplit_readers) p3 writes it twice, fp32 and
        # pre-split -- that copy with its 8 spare rows too, for the split padding vectors -- and they read the split one
        br = self.aspp.branches() if isinstance(self.aspp, (ASPPV2Engine, ASPPEngine)) else None
        dual = pre and br is not None and presplit_readers(self.p3, br, x, n * h * w)
        flat_s = a.get("pur3s+tail", (n * h * w + gap + 8, c // 32, 3, 32), torch.bfloat16, zero=gap > 0) if dual else None
        ys = flat_s[:n * h * w].view(ops.split3_shape(n, h, w, c)) if dual else None
        y = ops.conv2d(y, self.p3, out=flat[:n * h * w].view(n, h, w, c), x_split3=pre, also_split3=ys)
        if isinstance(self.aspp, ASPPV2Engine):
            return self.aspp.forward(y, tail=flat[n * h * w + gap:], xs=ys, tail_s=flat_s[n * h * w + gap:] if dual else None)
        return self.aspp.forward(y, xs=ys) if dual else self.aspp.forward(y)


class VGG16Engine:
    """VGG16 trunk (reference: networks/backbones.py:404-405)."""

    def __init__(self, prm, arena):
        from .networks.backbones import VGG_LAYOUT
        self.arena = arena
        self.steps = []
        for item in VGG_LAYOUT:
            if isinstance(item, tuple):
                idx, _, _, _, relu = item
                conv = prm.features[idx]
                relu = relu or prm.last_relu
                self.steps.append(conv_params(conv, None, relu=relu, stem4=(idx == 0)))
            else:
                self.steps.append(item)

    def forward(self, x4):
        a = self.arena
        x = x4
        for i, st in enumerate(self.steps):
            n, h, w, _ = x.shape
            if isinstance(st, ConvParams):
                x = ops.conv2d(x, st, out=a.get(("vgg", i & 1, st.cout), (n, h, w, st.cout)))
            else:
                ho, wo = ops._pool_out(h, 3, st, 1, False), ops._pool_out(w, 3, st, 1, False)
                x = ops.maxpool2d(x, 3, st, 1, out=a.get(("vggp", i), (n, ho, wo, x.shape[3])))
        return x
