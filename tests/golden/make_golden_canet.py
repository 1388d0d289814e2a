#!/usr/bin/env python3
"""Generate the CANet fixtures under tests/golden/ from the REFERENCE itself (networks/canet.py, networks/backbones.py).

Runs only in the build container (needs /root/reference).  The unmodified reference ``CaNet`` is built with
``pretrained_weights["resnet50"] = None`` (the ImageNet checkpoint is not part of either box), its parameters are set by
``synth.wgen_state_dict_for`` and ``synth`` episodes are run on the CPU in eval mode.  The ``sacred`` / ``dropblock`` stand-ins
come from make_golden.py.  Every case stores THREE passes of the iterative refinement (entry/canet.py:72-80): pass 0 with a
zero history, pass p with ``softmax(pass p - 1)`` of the reference's own low-resolution logits.  Per pass: the low-resolution
logits, and per output size the packed arg-max and the cross-entropy loss.  From pass 0, with forward hooks, in pipeline
order: the support vector ``z`` (channels 256..511 of ``layer55``'s input), samples of ``layer5``'s output (rows reordered to
[all supports | all queries], the engines' layout), of ``layer55``'s output and of the ASPP input (``aspp_1``'s input).
``canet_small`` also holds pass 0 of a ``history=False`` model (``nh_`` keys).

usage:  python tests/golden/make_golden_canet.py
"""
import json
import logging
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[2]
REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

from pemp_amd import synth  # noqa: E402
from tests.golden.make_golden import _install_standins  # noqa: E402

#: Wgen seed of the parameters.  The default (1234) answers "background" at every pixel; 1259 gives both classes in every
#: episode used here (foreground share 0.3 .. 0.5) with logits within -66 .. 24.
WGEN_SEED = 1259
PASSES = 3
#: pass 1 must differ from pass 0 by more than this (100 x the logit tolerance of the tests): the history input matters
MIN_HISTORY_EFFECT = 0.2
#: tests/util.py: MARGIN = 2 * LOGIT_TOL, and assert_argmax_exact's cap on the share of pixels whose lead is inside it
MARGIN, MAX_MASKED = 4e-3, 0.03
#: (file, seeds, shot, H, out_shapes): every seed of a case is one episode of ONE batch
CASES = (
    ("canet_small", (3, 4), 1, 97, ((97, 97), (80, 120))),
    ("canet_small5", (5,), 5, 97, ((64, 90),)),
    ("canet_full", (5678,), 1, 401, (synth.QUERY_SIZES[5678 % 5],)),
)


def build_model(history=True):
    from networks import canet
    canet.pretrained_weights["resnet50"] = None
    canet.net_ingredient.cfg = dict(init_channels=3, drop_rate=0.5, history=history, freeze_backbone=True)
    model = canet.CaNet(logging.getLogger("golden"))
    model.load_state_dict(synth.wgen_state_dict_for(model, seed=WGEN_SEED))
    return model.eval()


def _sample(t, H):
    return t[:, ::16].numpy() if H <= 97 else t[:, ::32, ::5, ::5].numpy()


def _outputs(res, pre, low, seeds, shot, H, out_shapes):
    """Arg-max bits and CE loss of low-resolution logits ``low`` at every output size (canet.py:156-159)."""
    for n, oh in enumerate(out_shapes):
        gt = torch.from_numpy(np.concatenate([synth.make_episode(s, shot=shot, height=H, width=H, out_hw=oh)["qry_mask"]
                                              for s in seeds]))
        logits = F.interpolate(low, tuple(oh), mode="bilinear", align_corners=True)
        am = logits.argmax(1)
        masked = float(((logits[:, 1] - logits[:, 0]).abs() <= MARGIN).float().mean())
        assert masked <= MAX_MASKED / 3, f"{pre}: out {oh}: {masked:.4f} of the pixels lead by <= {MARGIN}"
        res[f"{pre}o{n}_masked"] = np.array(masked)
        for b in range(len(seeds)):
            assert set(np.unique(am[b].numpy())) == {0, 1}, f"{pre}: episode {seeds[b]}, out {oh}: arg-max holds one class only"
        loss = float(F.cross_entropy(logits, gt, ignore_index=255))
        assert np.isfinite(loss)
        res[f"{pre}o{n}_argmax_bits"] = np.packbits(am.numpy().astype(np.uint8).reshape(-1))
        res[f"{pre}o{n}_loss"] = np.array(loss, np.float64)


def run_case(model, seeds, shot, H, out_shapes, passes=PASSES, pre=""):
    eps = [synth.make_episode(s, shot=shot, height=H, width=H) for s in seeds]
    sup = torch.from_numpy(np.stack([e["sup_img"] for e in eps]))
    msk = torch.from_numpy(np.stack([e["sup_mask"] for e in eps]))
    qry = torch.from_numpy(np.stack([e["qry_img"] for e in eps]))
    B = len(seeds)
    grab = {}
    hooks = [model.layer5.register_forward_hook(lambda _m, _i, o: grab.__setitem__("l5", o.detach())),
             model.layer55.register_forward_hook(lambda _m, i, o: grab.update(l55_in=i[0].detach(), l55=o.detach())),
             model.aspp_1.register_forward_hook(lambda _m, i, _o: grab.__setitem__("aspp_in", i[0].detach()))]
    res = {}
    h = (H - 1) // 8 + 1                                                   # pascal_voc.py:424
    hist = torch.zeros(B, 1, 2, h, h)
    prev = None
    for p in range(passes):
        with torch.no_grad():
            low = model(sup, msk, qry, False, history_mask=hist)
        if p == 0:
            l5 = grab["l5"].view(B, shot + 1, *grab["l5"].shape[1:])
            l5 = torch.cat((l5[:, :shot].flatten(0, 1), l5[:, shot:].flatten(0, 1)))      # [all supports | all queries]
            res[pre + "layer5_s"] = _sample(l5, H)
            res[pre + "z"] = grab["l55_in"][:, 256:, 0, 0].numpy()
            res[pre + "layer55_s"] = _sample(grab["l55"], H)
            res[pre + "aspp_in_s"] = _sample(grab["aspp_in"], H)
        else:
            change = float((low - prev).abs().max())
            res[f"{pre}p{p}_change"] = np.array(change)
            if p == 1 and model.use_history:
                assert change > MIN_HISTORY_EFFECT, f"the history input moves the logits by only {change}"
        res[f"{pre}p{p}_logits"] = low.numpy()
        _outputs(res, f"{pre}p{p}_", low, seeds, shot, H, out_shapes)
        prev = low
        hist = F.softmax(low, dim=1)[:, None]
    for hk in hooks:
        hk.remove()
    return res


def main():
    torch.set_num_threads(8)
    torch.manual_seed(0)
    _install_standins()
    sys.path.insert(0, str(REF))
    model = build_model()
    spec = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in model.state_dict().items()]
    (OUT / "state_keys_canet.json").write_text(json.dumps(spec))
    for name, seeds, shot, H, out_shapes in CASES:
        res = {"seeds": np.array(seeds), "shot": np.array(shot), "H": np.array(H), "passes": np.array(PASSES)}
        for n, oh in enumerate(out_shapes):
            res[f"o{n}_out_hw"] = np.array(oh)
        res.update(run_case(model, seeds, shot, H, out_shapes))
        if name == "canet_small":
            res.update(run_case(build_model(history=False), seeds, shot, H, out_shapes, passes=1, pre="nh_"))
        np.savez_compressed(OUT / f"{name}.npz", **res)
        print("wrote", name, "range", float(res["p0_logits"].min()), float(res["p0_logits"].max()),
              "change", [float(res[f"p{p}_change"]) for p in range(1, PASSES)],
              "loss", [float(res[f"p{p}_o0_loss"]) for p in range(PASSES)], flush=True)


if __name__ == "__main__":
    main()
