#!/usr/bin/env python3
"""Generate the PFENet train-step fixtures under tests/golden/ from the REFERENCE itself (networks/pfenet.py in train() mode).

Needs the reference checkout (``REF``); runs on the CPU in under a minute.  Built like
make_golden_canet_train.py: the unmodified reference ``PFENet`` of make_golden_pfenet.build_model (wgen seed 1259), here in
``train()`` mode, so the trunk -- run under ``no_grad`` once for the queries and once per shot -- normalises every call with
that call's batch statistics and moves its running statistics S + 1 times.  The ``nn.Dropout2d`` modules get forward hooks that
replace their output by ``input * keep / (1 - p)``, keep where a STORED uniform u < 1 - p (the rule of
train_ops.dropout2d_mask(uniforms=...)); ``down_supp.2`` is called once per shot and counts its calls.  The step is the
reference Trainer's (entry/pfenet.py:63-71): ``loss = CE(out, y)``, ``(loss + aux_loss * loss_coef).backward()``, loss_coef 1.
Each step is run twice, in float32 and in float64 (the same model ``.double()``).

Files (key layout of tests/util.check_gradients):
  <case>.npz      seeds, shot, H, dropout (False: every p = 0), ``draws__<module>`` [rows, 256] (``down_supp.2``: row b * S + s, the
                  engine's support order), ``loss``, ``aux``, ``grad_names``, ``grad_norms`` (-1: trunk, no gradient),
                  ``grad__<name>`` (every 37th element above 40000 elements), ``low32``, ``inner32__<k>``, ``l3_s`` / ``l4_s``
                  (samples of the query's train-mode layer-3 / layer-4 features), ``prior_bin0``, ``bn__<module>.running_mean`` /
                  ``.running_var`` / ``.num_batches_tracked`` after the step, ``draw_seed`` and the two figures of
                  ``_down_supp_margin``
  <case>_f64.npz  ``loss64``, ``aux64``, ``low64``, ``inner64__<k>``, ``grad_norms64``, ``g64__<name>``, ``l3_s64``, ``l4_s64``,
                  ``prior_bin0_64``, ``bn64__...``
  pfenet_trajectory.npz   five SGD steps (every p = 0, lr 1e-4, momentum 0.9, wd 1e-4) on seeds (3, 4): ``losses32``,
                  ``losses64``, ``aux32``, ``aux64``

usage:  python tests/golden/make_golden_pfenet_train.py
"""
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[2]
REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

from pemp_amd import synth  # noqa: E402
from tests.golden import make_golden_pfenet as G  # noqa: E402
from tests.golden.make_golden import _install_standins  # noqa: E402

DRAW_SEED = 78
#: (file, seeds, shot, H, Dropout2d on)
CASES = (
    ("pfenet_trainstep", (3, 4), 1, 97, True),
    ("pfenet_trainstep5", (5,), 5, 97, True),
    ("pfenet_trainstep_p0", (3, 4), 1, 97, False),
)
DROP_P = {"down_query.2": 0.5, "down_supp.2": 0.5, "cls.2": 0.1, **{f"inner_cls.{i}.2": 0.1 for i in range(4)}}
#: gradients stored as samples (the norms of all are stored)
SAMPLED = ("down_query.0.weight", "down_supp.0.weight", "init_merge.0.0.weight", "init_merge.2.0.weight", "alpha_conv.1.0.weight",
           "beta_conv.0.0.weight", "inner_cls.0.0.weight", "inner_cls.1.3.weight", "inner_cls.1.3.bias", "res1.0.weight",
           "res2.2.weight", "cls.3.weight", "cls.3.bias")
BN_STORED = ("layer0.1", "layer3.0.bn1", "layer4.2.bn3")
TRAJ = dict(seeds=(3, 4), steps=5, lr=1e-4, momentum=0.9, weight_decay=1e-4)


def _batch(seeds, shot, H, dtype):
    eps = [synth.make_episode(s, shot=shot, height=H, width=H) for s in seeds]
    sup = torch.from_numpy(np.stack([e["sup_img"] for e in eps])).to(dtype)
    msk = torch.from_numpy(np.stack([e["sup_mask"] for e in eps])).to(dtype)
    qry = torch.from_numpy(np.stack([e["qry_img"] for e in eps])).to(dtype)
    gt = torch.from_numpy(np.concatenate([synth.make_episode(s, shot=shot, height=H, width=H, out_hw=(H, H))["qry_mask"]
                                          for s in seeds]))
    return sup, msk, qry, gt


def _model(shot, dtype, drop, draws):
    """The reference model in train() mode, its Dropout2d modules pinned to ``draws`` (``drop`` False: every p = 0); ``model.grab``
    collects what the fixtures store."""
    model = G.build_model(shot).train().to(dtype)
    grab = model.grab = {"pre_supp": [], "l3": [], "l4": [], "inner": [None] * 4}
    calls = {}
    for name, m in model.named_modules():
        if isinstance(m, nn.Dropout2d):
            assert abs(m.p - DROP_P[name]) < 1e-12, (name, m.p)
            if not drop:
                m.p = 0.0

            def hook(mod, inp, _out, name=name):
                x = inp[0]
                k = calls.get(name, 0)
                calls[name] = k + 1
                if mod.p == 0.0:
                    return x
                u = draws[name]
                u = u[k::shot] if name == "down_supp.2" else u       # call k is shot k: rows b * S + k
                assert tuple(u.shape) == tuple(x.shape[:2]), (name, u.shape, x.shape)
                return x * ((u < 1 - mod.p).to(x.dtype) / (1 - mod.p))[:, :, None, None]
            m.register_forward_hook(hook)
    model.down_supp[0].register_forward_hook(lambda _m, _i, o: grab["pre_supp"].append(o.detach().clone()))   # before the in-place ReLU
    model.layer3.register_forward_hook(lambda _m, _i, o: grab["l3"].append(o.detach().clone()))
    model.layer4.register_forward_hook(lambda _m, _i, o: grab["l4"].append(o.detach().clone()))
    model.init_merge[0].register_forward_hook(lambda _m, i, _o: grab.__setitem__("prior0", i[0][:, 512].detach().clone()))
    model.cls.register_forward_hook(lambda _m, _i, o: grab.__setitem__("low", o.detach().clone()))
    for k, mod in enumerate(model.inner_cls):
        mod.register_forward_hook(lambda _m, _i, o, k=k: grab["inner"].__setitem__(k, o.detach().clone()))
    model.drop_calls = calls
    return model


def _draws(B, shot, seed):
    gen = torch.Generator().manual_seed(seed)
    d = {k: torch.rand((B * shot if k == "down_supp.2" else B, 256), generator=gen) for k in DROP_P}
    for k, u in d.items():
        assert float((u - (1 - DROP_P[k])).abs().min()) > 1e-6, f"{k}: a draw sits on the keep threshold"
    return d


def _step(seeds, shot, H, drop, dtype, draws):
    model = _model(shot, dtype, drop, draws)
    sup, msk, qry, gt = _batch(seeds, shot, H, dtype)
    out, aux = model(sup, msk, qry, gt[:, None], (H, H))
    loss = F.cross_entropy(out, gt, ignore_index=255)
    (loss + aux * 1.0).backward()
    assert model.drop_calls == {k: (shot if k == "down_supp.2" else 1) for k in DROP_P}, model.drop_calls
    return model, float(loss.detach()), float(aux.detach())


def _down_supp_margin(pre32, pre64, msk, keep, shot):
    """A support pixel carries mask / area of its channel's ``down_supp`` gradient (Weighted_GAP's adjoint), so ONE ReLU of
    ``down_supp`` that switches there is not absorbed the way a query-side switch is (make_golden_canet_train._layer5_margin).  A
    pre-activation closer to zero than the reference's OWN float32-vs-float64 difference of that tensor is a coin flip for any
    float32 implementation, so a fixture holds none among the support positions that carry gradient (interpolated mask > 0, channel
    kept by ``down_supp.2``).  pre32 / pre64: one [B,256,h,w] per shot; keep: bool [B * S, 256], row b * S + s.
    -> (smallest such |pre-activation| in float64, the reference's max |f32 - f64| of the pre-activations)."""
    near, margin = float("inf"), 0.0
    for s in range(shot):
        m = F.interpolate((msk[:, s, 0:1] == 1).double(), pre64[s].shape[-2:], mode="bilinear", align_corners=True) > 0
        carry = m & keep[s::shot][:, :, None, None]
        near = min(near, float(pre64[s].abs()[carry].min()))
        margin = max(margin, float((pre32[s].double() - pre64[s]).abs().max()))
    return near, margin


def gen_step(name, seeds, shot, H, drop):
    B = len(seeds)
    draw_seed = DRAW_SEED
    draws = _draws(B, shot, draw_seed)
    m32, loss32, aux32 = _step(seeds, shot, H, drop, torch.float32, draws)
    m64, loss64, aux64 = _step(seeds, shot, H, drop, torch.float64, draws)
    msk = _batch(seeds, shot, H, torch.float32)[1]
    while True:               # down_supp's pre-activation does not depend on the draws: only which positions carry gradient does
        keep = draws["down_supp.2"] < 0.5 if drop else torch.ones_like(draws["down_supp.2"], dtype=torch.bool)
        near, margin = _down_supp_margin(m32.grab["pre_supp"], m64.grab["pre_supp"], msk, keep, shot)
        if near > margin:
            break
        assert drop, f"{name}: a support pre-activation of down_supp lies {near:.1e} from zero (margin {margin:.1e}) without Dropout2d"
        draw_seed += 1
        draws = _draws(B, shot, draw_seed)
    if draw_seed != DRAW_SEED:
        m32, loss32, aux32 = _step(seeds, shot, H, drop, torch.float32, draws)
        m64, loss64, aux64 = _step(seeds, shot, H, drop, torch.float64, draws)
    g32, g64 = m32.grab, m64.grab
    res = {"draw_seed": np.array(draw_seed), "down_supp_support_min_abs": np.array(near), "down_supp_f32_error": np.array(margin),
           "seeds": np.array(seeds), "shot": np.array(shot), "H": np.array(H), "dropout": np.array(drop),
           "loss": np.array(loss32, np.float64), "aux": np.array(aux32, np.float64), "low32": g32["low"].numpy(),
           "l3_s": g32["l3"][0][:, ::64].numpy(), "l4_s": g32["l4"][0][:, ::64].numpy(), "prior_bin0": g32["prior0"].numpy()}
    res.update({"draws__" + k: v.numpy() for k, v in draws.items()})
    res.update({f"inner32__{k}": v.numpy() for k, v in enumerate(g32["inner"])})
    r64 = {"loss64": np.array(loss64, np.float64), "aux64": np.array(aux64, np.float64), "low64": g64["low"].numpy(),
           "l3_s64": g64["l3"][0][:, ::64].numpy(), "l4_s64": g64["l4"][0][:, ::64].numpy(), "prior_bin0_64": g64["prior0"].numpy()}
    r64.update({f"inner64__{k}": v.numpy() for k, v in enumerate(g64["inner"])})
    mods32, mods64 = dict(m32.named_modules()), dict(m64.named_modules())
    for bn in BN_STORED:
        for key in ("running_mean", "running_var", "num_batches_tracked"):
            res[f"bn__{bn}.{key}"] = getattr(mods32[bn], key).numpy()
            r64[f"bn64__{bn}.{key}"] = getattr(mods64[bn], key).numpy()
        assert int(mods32[bn].num_batches_tracked) == shot + 1, (bn, int(mods32[bn].num_batches_tracked))
    names, n32, n64 = [], [], []
    p32, p64 = dict(m32.named_parameters()), dict(m64.named_parameters())
    for k, q in p32.items():
        names.append(k)
        n32.append(float(q.grad.norm()) if q.grad is not None else -1.0)
        n64.append(float(p64[k].grad.norm()) if p64[k].grad is not None else -1.0)
        assert (q.grad is None) == k.startswith("layer"), k
        if q.grad is not None:
            assert n32[-1] > 0 and n64[-1] > 0, f"{name}: the gradient of {k} is zero"
    res["grad_names"], res["grad_norms"] = np.array(names), np.array(n32, np.float64)
    r64["grad_norms64"] = np.array(n64, np.float64)
    for k in SAMPLED:
        g, gd = p32[k].grad, p64[k].grad
        res["grad__" + k] = g.numpy() if g.numel() <= 40000 else g.reshape(-1)[::37].numpy()
        r64["g64__" + k] = gd.numpy() if gd.numel() <= 40000 else gd.reshape(-1)[::37].numpy()
    am = g64["low"].argmax(1)
    for b in range(B):
        assert set(np.unique(am[b].numpy())) == {0, 1}, f"{name}: episode {seeds[b]}: one class only in the low-resolution arg-max"
    np.savez_compressed(OUT / f"{name}.npz", **res)
    np.savez_compressed(OUT / f"{name}_f64.npz", **r64)
    worst = max((float((p32[k].grad.double() - p64[k].grad).norm() / p64[k].grad.norm()), k) for k in p64 if p64[k].grad is not None)
    print(f"  draw seed {draw_seed}: smallest gradient-carrying support pre-activation of down_supp {near:.2e}, reference f32 error "
          f"{margin:.2e}")
    print(f"wrote {name}: loss {loss32:.6f} (f64 {loss64:.6f}), aux {aux32:.6f} (f64 {aux64:.6f}), worst relative L2 gradient error "
          f"f32 vs f64 {worst[0]:.1e} ({worst[1]}), |low32 - low64| {float((g32['low'] - g64['low']).abs().max()):.1e}", flush=True)


def _trajectory(dtype):
    seeds, H = TRAJ["seeds"], 97
    model = _model(1, dtype, False, None)
    sup, msk, qry, gt = _batch(seeds, 1, H, dtype)
    opt = torch.optim.SGD(list(model.parameters()), lr=TRAJ["lr"], momentum=TRAJ["momentum"], weight_decay=TRAJ["weight_decay"])
    losses, auxs = [], []
    for _ in range(TRAJ["steps"]):
        opt.zero_grad()
        for k in ("pre_supp", "l3", "l4"):
            model.grab[k].clear()
        out, aux = model(sup, msk, qry, gt[:, None], (H, H))
        loss = F.cross_entropy(out, gt, ignore_index=255)
        (loss + aux).backward()
        opt.step()
        losses.append(float(loss.detach()))
        auxs.append(float(aux.detach()))
    return np.array(losses, np.float64), np.array(auxs, np.float64)


def gen_trajectory():
    (l32, a32), (l64, a64) = _trajectory(torch.float32), _trajectory(torch.float64)
    tot = l64 + a64
    assert tot[-1] < 0.5 * tot[0], f"the trajectory does not descend: {tot}"
    np.savez_compressed(OUT / "pfenet_trajectory.npz", seeds=np.array(TRAJ["seeds"]), H=np.array(97), lr=np.array(TRAJ["lr"]),
                        momentum=np.array(TRAJ["momentum"]), weight_decay=np.array(TRAJ["weight_decay"]), losses32=l32, losses64=l64,
                        aux32=a32, aux64=a64)
    print("wrote pfenet_trajectory: f64 total", [round(float(v), 4) for v in tot], "gap",
          [f"{max(abs(a - b), abs(c - d)):.1e}" for a, b, c, d in zip(l32, l64, a32, a64)], flush=True)


def main():
    torch.set_num_threads(8)
    torch.manual_seed(0)
    _install_standins()
    sys.path.insert(0, str(REF))
    for case in CASES:
        gen_step(*case)
    gen_trajectory()


if __name__ == "__main__":
    main()
