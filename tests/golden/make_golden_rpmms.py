#!/usr/bin/env python3
"""Generate the RPMMs fixtures under tests/golden/ from the REFERENCE itself (networks/rpmms.py, networks/backbones.py).

Runs only in the build container (needs /root/reference).  The unmodified reference ``RPMMs`` is built with
``pretrained_weights["resnet50"] = None`` (the ImageNet checkpoint is not part of either box), its parameters are set by
``synth.wgen_state_dict_for`` and ``synth`` episodes are run on the CPU in eval mode.  The ``sacred`` / ``dropblock`` stand-ins
come from make_golden.py.  The reference hard-codes ``.cuda()`` (rpmms.py:41,230,234): ``Tensor.cuda`` / ``Module.cuda`` are
made the identity in this process.  ``PMMs.__init__`` is wrapped: the float32 run records the three initial ``mu`` it draws
after ``torch.manual_seed(7)`` (K = 1, 3, 6 in this order, rpmms.py:41-43), and a float64 run of the same model (``.double()``)
is handed the same three tensors, so ``f64_err_p*`` is the reference's own float32 rounding and nothing else.

Every case stores the initial ``mu``, ``mu_f`` / ``mu_b`` per K, samples of ``layer5``'s output (rows reordered to [supports |
queries], the engines' layout), the prob-map channels of the three ``layer56`` inputs, samples of the last pass's ASPP input,
the three low-resolution logits and, per output size and pass, the packed arg-max, the cross-entropy against the synth label
(no ignore index: the reference's loss has none; synth labels hold no 255) and the share of pixels inside the margin.

usage:  python tests/golden/make_golden_rpmms.py
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

WGEN_SEED = 1259
MU_SEED = 7
KS = (1, 3, 6)
#: tests/util.py: LOGIT_TOL, MARGIN = 2 * LOGIT_TOL; the fixtures keep the masked share far inside assert_argmax_exact's 3 % cap
LOGIT_TOL, MARGIN, MAX_MASKED = 2e-3, 4e-3, 0.01
#: every pass must move the logits by more than this (100 x the logit tolerance): the history input matters
MIN_PASS_EFFECT = 0.2
#: (file, seeds, H, out_shapes): every seed of a case is one episode of ONE batch
CASES = (
    ("rpmms_small", (3, 4), 97, ((97, 97), (80, 120))),
    ("rpmms_full", (5678,), 401, (synth.QUERY_SIZES[5678 % 5],)),
)
#: what the wrapped PMMs does: {"force": {k: mu [1,256,k]} or None, "drawn": {k: mu}, "protos": {k: (mu_f, mu_b)}}
STATE = {"force": None, "drawn": {}, "protos": {}}


def install_patches(rpmms):
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    init, gen = rpmms.PMMs.__init__, rpmms.PMMs.generate_prototype

    def wrapped_init(self, c, k=3, stage_num=10):
        init(self, c, k, stage_num)
        if STATE["force"] is not None:
            self.mu = STATE["force"][k].clone()
        else:
            STATE["drawn"][k] = self.mu.detach().clone()

    def wrapped_gen(self, feature, mask):
        out = gen(self, feature, mask)
        STATE["protos"][self.num_pro] = (out[1].detach().clone(), out[2].detach().clone())
        return out

    rpmms.PMMs.__init__ = wrapped_init
    rpmms.PMMs.generate_prototype = wrapped_gen


def build_model():
    from networks import rpmms
    rpmms.pretrained_weights["resnet50"] = None
    rpmms.net_ingredient.cfg = dict(dist_scalar=20, init_channels=3, out_channels=512, backbone="resnet50", protos=3, drop_rate=0.5)
    model = rpmms.RPMMs(logging.getLogger("golden"))
    model.load_state_dict(synth.wgen_state_dict_for(model, seed=WGEN_SEED))
    return model.eval()


def _sample(t, H):
    return t[:, ::16].numpy() if H <= 97 else t[:, ::32, ::5, ::5].numpy()


def _sample_pm(t, H):
    """Both prob-map channels, ``_sample``'s spatial strides."""
    return t.numpy() if H <= 97 else t[:, :, ::5, ::5].numpy()


def _outputs(res, pre, low, seeds, H, out_shapes):
    for n, oh in enumerate(out_shapes):
        gt = torch.from_numpy(np.concatenate([synth.make_episode(s, shot=1, height=H, width=H, out_hw=oh)["qry_mask"] for s in seeds]))
        gt = torch.where(gt == 255, torch.zeros_like(gt), gt)
        logits = F.interpolate(low, tuple(oh), mode="bilinear", align_corners=True)
        am = logits.argmax(1)
        masked = float(((logits[:, 1] - logits[:, 0]).abs() <= MARGIN).float().mean())
        assert masked <= MAX_MASKED, f"{pre}: out {oh}: {masked:.4f} of the pixels lead by <= {MARGIN}"
        res[f"{pre}o{n}_masked"] = np.array(masked)
        for b in range(len(seeds)):
            assert set(np.unique(am[b].numpy())) == {0, 1}, f"{pre}: episode {seeds[b]}, out {oh}: arg-max holds one class only"
        loss = float(F.cross_entropy(logits, gt))
        assert np.isfinite(loss)
        res[f"{pre}o{n}_argmax_bits"] = np.packbits(am.numpy().astype(np.uint8).reshape(-1))
        res[f"{pre}o{n}_loss"] = np.array(loss, np.float64)


def run_case(model, seeds, H, out_shapes):
    eps = [synth.make_episode(s, shot=1, height=H, width=H) for s in seeds]
    sup = torch.from_numpy(np.stack([e["sup_img"] for e in eps]))
    msk = torch.from_numpy(np.stack([e["sup_mask"] for e in eps]))
    qry = torch.from_numpy(np.stack([e["qry_img"] for e in eps]))
    grab = {"l5": [], "pm": [], "aspp_in": []}
    hooks = [model.layer5.register_forward_hook(lambda _m, _i, o: grab["l5"].append(o.detach())),
             model.layer56.register_forward_hook(lambda _m, i, _o: grab["pm"].append(i[0][:, 256:258].detach())),
             model.layer6.register_forward_hook(lambda _m, i, _o: grab["aspp_in"].append(i[0].detach()))]
    STATE.update(force=None, drawn={}, protos={})
    torch.manual_seed(MU_SEED)
    with torch.no_grad():
        _, *outs = model(sup, msk, qry)
    for hk in hooks:
        hk.remove()
    res = {}
    for k in KS:
        res[f"mu0_k{k}"] = STATE["drawn"][k][0].numpy()                    # [256,k]
        res[f"mu_f_k{k}"] = STATE["protos"][k][0].numpy()                  # [B,k,256]
        res[f"mu_b_k{k}"] = STATE["protos"][k][1].numpy()
    assert len(grab["l5"]) == 2 and len(grab["pm"]) == 3 and len(grab["aspp_in"]) == 3
    res["layer5_s"] = _sample(torch.cat(grab["l5"]), H)                    # the reference runs the supports first
    for p in range(3):
        res[f"p{p}_prob_s"] = _sample_pm(grab["pm"][p], H)
    res["aspp_in_s"] = _sample(grab["aspp_in"][2], H)
    # the same model in float64 with the same initial mu
    STATE.update(force={k: v.double() for k, v in STATE["drawn"].items()}, protos={})
    model.double()
    with torch.no_grad():
        _, *outs64 = model(sup.double(), msk.double(), qry.double())
    model.float()
    STATE["force"] = None
    for p, (low, low64) in enumerate(zip(outs, outs64)):
        err = float((low.double() - low64).abs().max())
        assert err <= LOGIT_TOL / 4, f"pass {p}: the reference's float32 logits are {err:.3e} off its float64 run"
        res[f"f64_err_p{p}"] = np.array(err)
        res[f"p{p}_logits"] = low.numpy()
        if p:
            change = float((low - outs[p - 1]).abs().max())
            assert change > MIN_PASS_EFFECT, f"pass {p} moves the logits by only {change}"
            res[f"p{p}_change"] = np.array(change)
        _outputs(res, f"p{p}_", low, seeds, H, out_shapes)
    return res


def main():
    torch.set_num_threads(8)
    torch.manual_seed(0)
    _install_standins()
    sys.path.insert(0, str(REF))
    from networks import rpmms
    install_patches(rpmms)
    model = build_model()
    spec = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in model.state_dict().items()]
    (OUT / "state_keys_rpmms.json").write_text(json.dumps(spec))
    for name, seeds, H, out_shapes in CASES:
        res = {"seeds": np.array(seeds), "shot": np.array(1), "H": np.array(H), "passes": np.array(3)}
        for n, oh in enumerate(out_shapes):
            res[f"o{n}_out_hw"] = np.array(oh)
        res.update(run_case(model, seeds, H, out_shapes))
        np.savez_compressed(OUT / f"{name}.npz", **res)
        print("wrote", name, "range", float(res["p2_logits"].min()), float(res["p2_logits"].max()),
              "f64_err", [float(res[f"f64_err_p{p}"]) for p in range(3)], "change", [float(res[f"p{p}_change"]) for p in (1, 2)],
              "masked", [float(res[f"p{p}_o0_masked"]) for p in range(3)], "loss", [float(res[f"p{p}_o0_loss"]) for p in range(3)],
              flush=True)


if __name__ == "__main__":
    main()
