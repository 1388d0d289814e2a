"""PEMP stage 1 on MI355X: drop-in for the reference's ``networks/pemp_stage1.py``.

Same module surface (``net_ingredient``, ``ModelClass``, ``PEMPStage1``, ``pretrained_weights``,
``backbone_error``), same constructor / ``forward`` signature and ``state_dict`` keys
(reference: networks/pemp_stage1.py:11-18,21-37,54-109,111-163,264); the arithmetic runs on
libpemp_hip.so through ``pemp_amd.engine`` / ``pemp_amd.ops`` and raises if that library is
missing or the tensors are not on the GPU.
"""
import gc
from collections import OrderedDict
from pathlib import Path

import torch
import torch.nn as nn

from .. import engine, ops
from ..config import Ingredient
from . import backbones

net_ingredient = Ingredient("net", save_git_info=False)
pretrained_weights = {
    "vgg16": Path(__file__).parents[2] / "data/vgg16-397923af.pth",
    "resnet50": Path(__file__).parents[2] / "data/resnet50-19c8e357.pth",
    "resnet101": Path(__file__).parents[2] / "data/resnet101-5d3b4d8f.pth",
}
backbone_error = "Not supported backbone '{}'. [vgg16, resnet50, resnet101]"
_RES_LAYERS = {"resnet50": (3, 4, 6), "resnet101": (3, 4, 23)}


@net_ingredient.config
def net_config():
    dist_scalar = 20            # int, factor multiplied to the cosine similarity
    init_channels = 3           # int, input channels of the model
    out_channels = 512          # int, output channels of the feature extractor
    backbone = "resnet50"       # str, [vgg16, resnet50, resnet101]
    protos = 3                  # int, prototypes per class (0: plain masked average pooling)
    drop_rate = 0.1             # float, DropBlock rate of the purifier (train only)
    block_size = 4              # int, DropBlock block size (train only)


@net_ingredient.config_hook
def net_hook(config, command_name, logger):
    if config["net"]["backbone"] not in pretrained_weights:
        raise ValueError(backbone_error.format(config["net"]["backbone"]))
    return {}


def import_torchvision_trunk(trunk, path, resnet=True):
    """Pretrained import rules of the reference: ResNet copies torchvision keys up to the first
    ``layer4.*`` (networks/backbones.py:138-157); VGG copies the first 26 tensors (:412-421)."""
    pre = torch.load(str(path), map_location="cpu")
    cur = trunk.state_dict()
    if resnet:
        for key in pre:
            if key.split(".")[0] in ("layer4", "fc"):
                break
            cur[key] = pre[key]
    else:
        ck, pk = list(cur.keys()), list(pre.keys())
        for i in range(26):
            cur[ck[i]] = pre[pk[i]]
    trunk.load_state_dict(cur)


MAX_PROTOS = 8      # the prototype-head kernels are instantiated for 2 * protos <= 8 and <= 16 rows per pixel (csrc/head.hip)


def check_protos(protos, key):
    """The reference accepts any ``protos`` (networks/pemp_stage1.py:26,104-105; default 3); this build's head kernels are
    instantiated for at most MAX_PROTOS per class.  Fail at model construction, not inside a kernel launch."""
    if not 0 <= int(protos) <= MAX_PROTOS:
        raise ValueError(f"{key} = {protos}: this build supports 0 (plain masked average pooling) .. {MAX_PROTOS} prototypes "
                         f"per class (the head kernels keep 2 * protos <= 16 rows per pixel in registers; MAXJ in "
                         f"pemp_amd/csrc/head.hip)")


class _HeadMixin:
    """Episode head shared by stage 1 / stage 2 / baseline: prototypes -> cosine map -> upsample."""

    def _engine_for(self, device):
        """The inference engine (packed weights + activation arena + captured graphs) of the current LANE.  Lane 0 is
        the default; ``with model.lane(k):`` selects replica k -- same weights, its own arena and graphs -- so that
        several single-episode steps can be in flight on different HIP streams (entry.pemp_stage1.Evaluator(lanes=K))."""
        lane = self.__dict__.get("_lane", 0)
        prec = self.__dict__.get("_precision", "f32")
        key = lane if prec == "f32" else (lane, prec)
        engines = self.__dict__.setdefault("_engines", {})
        eng = engines.get(key)
        if eng is None or eng["device"] != device:
            arena = engine.Arena(device, torch.bfloat16 if prec == "bf16" else torch.float32)
            eng = {"device": device, "arena": arena}
            split3 = engine.SPLIT3
            engine.SPLIT3 = split3 and prec == "f32"       # "f32_chain" / "bf16": every conv on the fp32-chain kernels
            try:
                self._build_engine(eng, arena)
            finally:
                engine.SPLIT3 = split3
            engines[key] = eng
        if key == 0:
            self.__dict__["_engine"] = eng
        return eng

    def precision(self, prec):
        """Context manager: ``with model.precision("bf16"):`` runs the enclosed inference calls on the bf16-OPERAND variant of the
        encoder (bf16 activations and weights between the fp32 stem and the fp32 head, fp32 accumulation) -- the side figure of
        bench.py that shows what exact fp32 costs; stage-1 ResNet encoders only.  The default, and everything the parity
        tests hold, is "f32" (its convs on the split3 family where engine.SPLIT3 is on); "f32_chain" runs the same fp32 encoder on the
        fp32-chain conv kernels (A/B runs and tests)."""
        if prec not in ("f32", "bf16", "f32_chain"):
            raise ValueError(f"precision must be 'f32', 'f32_chain' or 'bf16', got {prec!r}")
        if prec == "bf16" and not (getattr(self, "_bf16_variant", False) and getattr(self, "backbone_name", "") != "vgg16"):
            raise ValueError("the bf16 variant exists for the stage-1 ResNet encoders only")
        model = self

        class _Prec:
            def __enter__(self_inner):
                self_inner.prev = model.__dict__.get("_precision", "f32")
                model.__dict__["_precision"] = prec

            def __exit__(self_inner, *exc):
                model.__dict__["_precision"] = self_inner.prev
                return False
        return _Prec()

    def lane(self, k):
        """Context manager: run the enclosed inference calls on engine replica ``k``."""
        model = self

        class _Lane:
            def __enter__(self_inner):
                self_inner.prev = (model.__dict__.get("_lane", 0), ops.SK_SCOPE)
                model.__dict__["_lane"] = k
                ops.SK_SCOPE = k                   # lanes run beside each other: each has its own split-K workspace

            def __exit__(self_inner, *exc):
                model.__dict__["_lane"], ops.SK_SCOPE = self_inner.prev
                return False
        return _Lane()

    @staticmethod
    def _require_eval_gpu(model, *tensors):
        if model.training:
            raise RuntimeError("pemp_amd: lowres()/graph replay are inference paths; call model.eval() "
                               "(model(...) itself works in train() mode and is differentiable)")
        for t in tensors:
            if not t.is_cuda:
                raise RuntimeError("pemp_amd: inputs must live on the GPU; there is no CPU fallback")

    def _head(self, eng, feats, sup_mask, B, S, Q, protos, dist_scalar, ret_ind, ctr):
        """feats: NHWC [B*S + B*Q, h, w, c] (supports first).  -> pred [BQ,2,h,w] (+ resp uint8)."""
        if Q != 1:
            raise ValueError("query must be 1 (the reference's broadcasting requires it, pemp_stage1.py:197,257)")
        ws = eng["arena"].ws
        sup, qry = feats[:B * S], feats[B * S:]
        H, W = sup_mask.shape[-2:]
        msk = sup_mask.reshape(B * S, 2, H, W).contiguous()
        if protos > 0:
            pro = ops.mpm_protos(sup, msk, ctr, B, S, protos, ws_cache=ws)
        else:
            pro = ops.masked_avg_pool(sup, msk, B, S, full_res=False, ws_cache=ws)
        self.__dict__["_last_protos"] = pro
        return ops.cosine_proto_max(qry, pro, dist_scalar, want_resp=ret_ind)

    def lowres_graphed(self, *inputs, ret_ind=False, device=None):
        """``lowres`` replayed from a captured hipGraph (one per input signature).

        The ~80 launches of one episode are short (tens of µs), so eager issue is bound by the
        host (ctypes + launch ≈ 5-10 µs each); the graph removes that.  Inputs are copied into
        static buffers; the returned tensors are the graph's static outputs and are overwritten
        by the next call with the same signature.  ``device``: HOST tensors are accepted and go
        straight into the static buffers on that device (one H2D copy each -- the reference's
        ``test_step`` body hands over host tensors, entry/pemp_stage1.py:48-49 -- instead of a
        fresh device tensor plus a device-to-device copy); the compute still has no CPU path.
        """
        if device is None or any(t.is_cuda for t in inputs):
            self._require_eval_gpu(self, *inputs)
            device = inputs[0].device
        elif self.training:
            self._require_eval_gpu(self)
        key = tuple((tuple(t.shape), t.dtype) for t in inputs) + (ret_ind, ops.EVAL_SPLITK)    # the conv variants are baked in
        # (the bf16 variant has its own engine, hence its own graphs)
        run = lambda static_in: self.lowres(*static_in, ret_ind=ret_ind)
        return self._replay(self._engine_for(torch.device(device)), key, inputs, run, run)

    @staticmethod
    def _replay(eng, key, inputs, warm, capture):
        """The capture protocol of every graphed entry point: on the first call with ``key`` the inputs go into static buffers
        on the engine's device, ``warm(static_in)`` runs twice on a side stream (populates arena + workspaces) and
        ``capture(static_in)`` is recorded into a hipGraph; every call then copies the inputs over and replays.  -> what
        ``capture`` returned (the graph's static outputs)."""
        device = eng["device"]
        graphs = eng.setdefault("graphs", {})
        entry = graphs.get(key)
        if entry is None:
            static_in = [torch.empty(t.shape, dtype=t.dtype, device=device) for t in inputs]
            for s, t in zip(static_in, inputs):
                s.copy_(t)
            side = torch.cuda.Stream(device=device)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side), torch.no_grad():
                for _ in range(2):
                    warm(static_in)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            # a dead model and its engine form a reference cycle that owns hipGraphs; the collection that destroys them must
            # not happen to run inside a capture (the runtime aborts), and torch.cuda.graph no longer collects on entry
            gc.collect()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph), torch.no_grad():
                out = capture(static_in)
            entry = graphs[key] = (graph, static_in, out)
        graph, static_in, out = entry
        for s, t in zip(static_in, inputs):
            s.copy_(t, non_blocking=True)
        graph.replay()
        return out

    @staticmethod
    def _finish(pred, resp, out_shape):
        out = ops.upsample_bilinear_ac(pred, out_shape)
        if resp is None:
            return out
        return out, ops.upsample_nearest_u8_i64(resp, out_shape)

    # -- prototype banks (pemp_amd.bank): enroll supports once, segment many queries -------------------------------
    # A model family states: _bank_family (str, or None: its head conditions on the query, no bank), _bank_resp (it has a
    # response map), _bank_setup() -> (p, dist_scalar), _bank_features(images) and _bank_pool(eng, feats, masks, K, S, out):
    # the feature pass and the pooling call of its own ``lowres``.
    _bank_family = None
    _bank_resp = False

    def _bank_desc(self):
        if self._bank_family is None:
            raise ValueError(f"{type(self).__name__}: prototype banks exist for the prototype-matching heads only (PEMP stage 1, "
                             "Baseline, PANet); this model's head depends on the query")
        p, dist_scalar = self._bank_setup()
        return dict(family=self._bank_family, backbone=self.backbone_name, precision=self.__dict__.get("_precision", "f32"),
                    p=int(p), c=int(self.feat_channels), dist_scalar=float(dist_scalar))

    @staticmethod
    def _bank_class():
        from ..bank import PrototypeBank
        return PrototypeBank

    def _check_bank(self, bank, what):
        cls = self._bank_class()
        if not isinstance(bank, cls):
            raise TypeError(f"{what}: expected a {cls.__name__}, got {type(bank).__name__}")
        for k, v in self._bank_desc().items():
            if getattr(bank, k) != v:
                raise ValueError(f"{what}: the bank was made with {k} = {getattr(bank, k)!r}, this model has {k} = {v!r}")

    def enroll(self, sup_img, sup_mask, labels=None, out=None):
        """Supports of K classes, ``sup_img`` [K,S,3,H,W] and ``sup_mask`` [K,S,2,H,W] -> ``PrototypeBank`` of their prototypes:
        one supports-only pass through the trunk and the pooling call an episode makes.  ``out``: enroll into that bank (same
        K) in place -- its ``protos`` keep their address, so captured graphs that read them see the new classes."""
        from ..bank import PrototypeBank
        desc = self._bank_desc()
        if out is not None:
            self._check_bank(out, "enroll(out=)")
        self._require_eval_gpu(self, sup_img, sup_mask)
        K, S, ch, H, W = sup_img.shape
        if tuple(sup_mask.shape) != (K, S, 2, H, W):
            raise ValueError(f"enroll: sup_mask must be [{K},{S},2,{H},{W}], got {tuple(sup_mask.shape)}")
        if out is not None and (len(out) != K or not out.protos.is_cuda):
            raise ValueError(f"enroll(out=): the bank holds {len(out)} classes on {out.protos.device}, {K} are enrolled")
        eng = self._engine_for(sup_img.device)
        with torch.no_grad():
            feats = self._bank_features(sup_img.reshape(K * S, ch, H, W))
            msk = sup_mask.reshape(K * S, 2, H, W).contiguous()
            pro = self._bank_pool(eng, feats, msk, K, S, None if out is None else out.protos)
        if out is None:
            return PrototypeBank(pro, labels=labels, **{k: desc[k] for k in ("family", "backbone", "precision", "dist_scalar")})
        if labels is not None:
            out.labels = PrototypeBank._labels(labels, K)
        return out

    def _segment_dev(self, bank, qry_img, index_dev, ret_ind):
        feats = self._bank_features(qry_img)
        out = ops._cosine_bank(feats, bank.protos, bank.dist_scalar, index_dev, want_resp=ret_ind)
        return out if ret_ind else (out, None)

    def _segment_args(self, bank, qry_img, index, ret_ind, what):
        self._check_bank(bank, what)
        if ret_ind and not self._bank_resp:
            raise ValueError(f"{what}: ret_ind is a stage-1 option (the response map of its meta-prototypes)")
        if qry_img.dim() != 4:
            raise ValueError(f"{what}: qry_img must be [N,3,H,W], got {tuple(qry_img.shape)}")
        self._bank_query_check(bank, qry_img, what)
        return None if index is None else ops.bank_index(index, qry_img.shape[0], len(bank))      # checked on the host

    def _bank_query_check(self, bank, qry_img, what):
        """A family's own rules for the queries a bank may meet (none here)."""

    def segment_lowres(self, bank, qry_img, index=None, ret_ind=False):
        """Queries ``qry_img`` [N,3,H,W] against an enrolled bank, at feature resolution: one query-only pass through the
        trunk, one cosine launch.  ``index`` None: every query against every class -> pred [N,K,2,h,w]; ``index`` (N class
        numbers, a Python sequence or a CPU tensor): query b against class index[b] -> pred [N,2,h,w].
        -> (pred, resp uint8 or None)."""
        idx = self._segment_args(bank, qry_img, index, ret_ind, "segment_lowres")
        self._require_eval_gpu(self, qry_img, *bank.tensors())
        with torch.no_grad():
            return self._segment_dev(bank, qry_img, None if idx is None else idx.to(qry_img.device, non_blocking=True), ret_ind)

    def segment(self, bank, qry_img, index=None, out_shape=None, ret_ind=False):
        """``segment_lowres`` + the final upsampling of ``forward``: logits [N,2,Ho,Wo] with ``index``, [N,K,2,Ho,Wo] without
        (+ the int64 response map [N,Ho,Wo] / [N,K,Ho,Wo] when ``ret_ind``)."""
        pred, resp = self.segment_lowres(bank, qry_img, index, ret_ind)
        out_shape = tuple(out_shape) if out_shape is not None else tuple(qry_img.shape[-2:])
        lead = tuple(pred.shape[:-3])
        out = self._finish(pred.reshape((-1,) + tuple(pred.shape[-3:])), None if resp is None else resp.reshape((-1,) + tuple(resp.shape[-2:])),
                           out_shape)
        if resp is None:
            return out.view(lead + (2,) + out_shape)
        return out[0].view(lead + (2,) + out_shape), out[1].view(lead + out_shape)

    def segment_graphed(self, bank, qry_img, index=None, ret_ind=False):
        """``segment_lowres`` replayed from a captured hipGraph (the protocol of ``lowres_graphed``).  The graph reads
        ``bank.protos`` where it lies -- ``bank.update`` / ``enroll(out=bank)`` need no recapture -- and the index through a
        static int32 buffer.  The returned tensors are the graph's static outputs."""
        idx = self._segment_args(bank, qry_img, index, ret_ind, "segment_graphed")
        self._require_eval_gpu(self, qry_img, *bank.tensors())
        inputs = [qry_img] if idx is None else [qry_img, idx]
        key = ("bank",) + tuple(t.data_ptr() for t in bank.tensors()) + tuple((tuple(t.shape), t.dtype) for t in inputs) + \
              (len(bank), idx is not None, ret_ind, ops.EVAL_SPLITK)
        eng = self._engine_for(qry_img.device)
        # the graph holds the bank's addresses, the copy into the static index buffer reads host memory: keep both alive
        eng.setdefault("bank_refs", {})[key] = (bank.tensors(), idx)
        run = lambda s: self._segment_dev(bank, s[0], s[1] if idx is not None else None, ret_ind)
        return self._replay(eng, key, inputs, run, run)

    def segment_labels(self, bank, qry_img, out_shape=None, want_margin=False, graphed=False):
        """Every query against every enrolled class, decided per pixel: ``segment_lowres`` without an index (``graphed``:
        ``segment_graphed``) and one fused launch (``ops.nway_tail``) that upsamples the K binary maps and keeps, per pixel, 0
        where every class says background and else 1 + the slot of the class that claims it by the largest margin
        (foreground logit - background logit; the lowest slot wins equal margins).  -> labels uint8 [N,Ho,Wo] of slot
        numbers (``bank.labels`` maps them), with ``want_margin`` (labels, margin fp32 [N,Ho,Wo]).  ``out_shape`` defaults to
        the query size.  No full-resolution logits are stored.  ``out_shape`` may also be a sequence of N (Ho, Wo) pairs, one
        per query (frames resized from different originals): then the result is a list of N uint8 maps [Ho_i,Wo_i], with
        ``want_margin`` a list of N (labels, margin) pairs, every map a view into one packed buffer, from one ragged launch
        (``ops.nway_tail_ragged``); each map equals the single-query call with that ``out_shape``."""
        self._segment_args(bank, qry_img, None, False, "segment_labels")
        if len(bank) > 255:
            raise ValueError(f"segment_labels: the bank holds {len(bank)} classes; the labels are uint8 with 0 for no class, "
                             "so at most 255")
        ragged = out_shape is not None and all(hasattr(s, "__len__") for s in out_shape)      # pairs (or none at all), not two ints
        if ragged:
            out_shape = [tuple(int(v) for v in s) for s in out_shape]
            if len(out_shape) != qry_img.shape[0] or any(len(s) != 2 or min(s) < 1 for s in out_shape):
                raise ValueError(f"segment_labels: out_shape must be one (Ho, Wo) or one pair per query ({qry_img.shape[0]}), "
                                 f"got {out_shape}")
        pred, _ = (self.segment_graphed if graphed else self.segment_lowres)(bank, qry_img)
        if ragged:
            labels, margin, _ = ops.nway_tail_ragged(pred, out_shape, want_margin=want_margin,
                                                     ws_cache=self._engine_for(qry_img.device)["arena"].ws)
            return list(zip(labels, margin)) if want_margin else labels
        out_shape = tuple(out_shape) if out_shape is not None else tuple(qry_img.shape[-2:])
        labels, margin, _ = ops.nway_tail(pred, out_shape, want_margin=want_margin, ws_cache=self._engine_for(qry_img.device)["arena"].ws)
        return (labels, margin) if want_margin else labels

    def segment_confusion(self, bank, qry_img, target, want=None, graphed=False, want_labels=False):
        """``segment_labels`` scored as a semantic segmentation: ``segment_lowres`` without an index (``graphed``:
        ``segment_graphed``) and ONE confusion launch (``ops.nway_confusion``) that decides every pixel as ``segment_labels``
        does and counts it against ``target``.  -> (conf int64 [N,K+1,K+1], labels | None): ``conf[n, t, p]`` is the number
        of pixels of query n with target class t and label p, 0 for no class and 1 + slot otherwise
        (``core.metrics.SemanticMetric`` turns the table into per-class IoU).  ``target``: one int64 tensor [N,Ho,Wo], or a
        list of N int64 tensors with their own sizes (one ragged launch); it holds slot labels 0..K with 255 ignored
        (``ops.slot_targets`` maps dataset class ids), or with ``want`` (N slots) the binary mask 0 / 1 / 255 of each query's
        own class.  ``want_labels``: also the label maps, ``segment_labels``'s bit for bit.  At most 63 classes."""
        self._segment_args(bank, qry_img, None, False, "segment_confusion")
        if len(bank) > ops.CONFUSION_MAX_K:
            raise ValueError(f"segment_confusion: the bank holds {len(bank)} classes; the confusion tail counts at most "
                             f"{ops.CONFUSION_MAX_K}")
        ragged = not isinstance(target, torch.Tensor)
        n = qry_img.shape[0]
        if ragged:
            target = list(target)
            if len(target) != n:
                raise ValueError(f"segment_confusion: {len(target)} targets for {n} queries")
        elif target.dim() != 3 or target.shape[0] != n or target.dtype != torch.int64:
            raise ValueError(f"segment_confusion: target must be int64 [{n},Ho,Wo] or a list of {n} int64 maps, got "
                             f"{tuple(target.shape)} {target.dtype}")
        if want is not None and not (isinstance(want, torch.Tensor) and want.device.type != "cpu"):
            want = ops.bank_index(want, n, len(bank))                                           # checked on the host
        pred, _ = (self.segment_graphed if graphed else self.segment_lowres)(bank, qry_img)
        if ragged:
            return ops.nway_confusion_ragged(pred, target, want=want, want_labels=want_labels)
        return ops.nway_confusion(pred, target.to(pred.device, non_blocking=True).contiguous(), want=want, want_labels=want_labels)


class PEMPStage1(_HeadMixin, backbones.BaseModel):
    """Stage 1 of the Prior-Enhanced network with Meta-Prototypes (reference class of the same name)."""
    _bf16_variant = True

    @net_ingredient.capture
    def __init__(self, logger, backbone, init_channels, out_channels, protos, drop_rate, block_size):
        super().__init__()
        if backbone not in pretrained_weights:
            raise ValueError(backbone_error.format(backbone))
        pretrained = pretrained_weights[backbone]
        self.backbone_name = backbone
        self.drop_rate, self.block_size = drop_rate, block_size          # DropBlock of the purifier / ASPPV2 (train only)
        if backbone == "vgg16":
            trunk = backbones.VGG16Params(init_channels, last_relu=False)
            self.encoder = nn.Sequential(OrderedDict([("backbone", trunk)]))
            self.__class__.__name__ = "PEMP_Stage1/VGG16"
        else:
            trunk = backbones.ResNetParams(init_channels, _RES_LAYERS[backbone], freeze_bn=True)
            self.encoder = nn.Sequential(OrderedDict([
                ("backbone", trunk), ("purifier", backbones.purifier_params(out_channels, v2=True))]))
            self.__class__.__name__ = "PEMP_Stage1/Resnet50" if backbone == "resnet50" else "PEMP_stage1/Resnet101"
        if pretrained is not None and Path(pretrained).exists():
            import_torchvision_trunk(trunk, pretrained, resnet=backbone != "vgg16")
        elif logger is not None:
            logger.info(f"           ==> pretrained file {pretrained} not found: backbone left at random init")
        check_protos(protos, "net.protos")
        self.feat_channels = 512 if backbone == "vgg16" else out_channels         # c of the encoder's output
        self.ctr = nn.Parameter(torch.rand(out_channels, protos * 2), requires_grad=True) if protos > 0 else None
        if logger is not None:
            logger.info(f"           ==> Model {self.__class__.__name__} created")

    # -- engine --------------------------------------------------------------------------------
    def _build_engine(self, eng, arena):
        bb = self.encoder.backbone
        if self.backbone_name == "vgg16":
            eng["trunk"] = engine.VGG16Engine(bb, arena)
            eng["purifier"] = None
        else:
            eng["trunk"] = engine.ResNetEngine(bb, arena)
            eng["purifier"] = engine.PurifierEngine(self.encoder.purifier, arena)
        eng["ctr"] = self.ctr.detach().float().contiguous() if self.ctr is not None else None

    def encode(self, *image_groups):
        """One or more [n_i,3,H,W] fp32 device tensors -> NHWC features [sum n_i,h,w,c] (in order)."""
        eng = self._engine_for(image_groups[0].device)
        x4 = engine.pack_episode(eng["arena"], image_groups)
        f = eng["trunk"].forward(x4)
        return eng["purifier"].forward(f) if eng["purifier"] is not None else f

    # -- prototype banks: the calls of lowres() / _head(), supports and queries apart ---------------
    _bank_family = "pemp_stage1"
    _bank_resp = True

    def _bank_setup(self):
        return (self.ctr.shape[1] // 2 if self.ctr is not None else 1), net_ingredient.cfg["dist_scalar"]

    def _bank_features(self, images):
        return self.encode(images)

    def _bank_pool(self, eng, feats, msk, K, S, out):
        ws = eng["arena"].ws
        if self.ctr is not None:
            return ops.mpm_protos(feats, msk, eng["ctr"], K, S, self.ctr.shape[1] // 2, ws_cache=ws, out=out)
        return ops.masked_avg_pool(feats, msk, K, S, full_res=False, ws_cache=ws, out=out)

    # -- API -----------------------------------------------------------------------------------
    @net_ingredient.capture
    def forward(self, sup_img, sup_mask, qry_img, out_shape=None, ret_ind=False, protos=3, dist_scalar=20):
        """Same contract as the reference (pemp_stage1.py:111-163): returns logits [BQ,2,Ho,Wo]
        (+ int64 response map [BQ,Ho,Wo] when ``ret_ind``).  In ``train()`` mode the logits carry a grad_fn:
        ``loss.backward()`` runs the explicit HIP backward and fills ``p.grad`` (entry/pemp_stage1.py:59-61)."""
        if self.training:
            if ret_ind:
                raise ValueError("ret_ind is an inference option (entry/pemp_stage1.py:213-217); call model.eval()")
            return self._train_bridge("stage1", sup_img.device)(sup_img, sup_mask, qry_img, out_shape)
        self._require_eval_gpu(self, sup_img, sup_mask, qry_img)
        pred, resp = self.lowres(sup_img, sup_mask, qry_img, ret_ind, protos, dist_scalar)
        H, W = sup_img.shape[-2:]
        return self._finish(pred, resp, out_shape if out_shape is not None else (H, W))

    def lowres(self, sup_img, sup_mask, qry_img, ret_ind=False, protos=None, dist_scalar=None):
        """Feature-resolution prediction [BQ,2,h,w] (+ uint8 response) -- everything before the
        final F.interpolate; shape-static, so it is what gets captured into a hipGraph."""
        cfg = net_ingredient.cfg
        protos = cfg["protos"] if protos is None else protos
        dist_scalar = cfg["dist_scalar"] if dist_scalar is None else dist_scalar
        if (self.ctr is None) != (protos == 0):
            protos = 0 if self.ctr is None else self.ctr.shape[1] // 2
        B, S, ch, H, W = sup_img.shape
        Q = qry_img.shape[1]
        eng = self._engine_for(sup_img.device)
        feats = self.encode(sup_img.reshape(B * S, ch, H, W), qry_img.reshape(B * Q, ch, H, W))
        self.__dict__["_last_feats"] = feats
        out = self._head(eng, feats, sup_mask, B, S, Q, protos, dist_scalar, ret_ind, eng["ctr"])
        return out if ret_ind else (out, None)


ModelClass = PEMPStage1
