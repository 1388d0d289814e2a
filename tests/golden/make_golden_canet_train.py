#!/usr/bin/env python3
"""Generate the CANet train-step fixtures under tests/golden/ from the REFERENCE itself (networks/canet.py in train() mode).

Runs only in the build container (needs /root/reference), on the CPU, in under a minute.  Built like make_golden_canet.py: the
unmodified reference ``CaNet`` with wgen weights (seed 1259), here in ``train()`` mode after ``maybe_fix_params`` (frozen trunk,
the reference's ``freeze_backbone = True``).  The eight ``nn.Dropout2d`` modules get forward hooks that replace their output by
``input * keep / (1 - p)``, the keep-mask derived from STORED uniforms by the rule of oracle/ref_cpu.py: Dropout2d and
train_ops.dropout2d_mask(uniforms=...) (keep where u < 1 - p), so that the HIP step can be given the same masks.  Each step is
run twice, in float32 and in float64 (the same model ``.double()``).

Files (key layout of tests/util.check_gradients):
  <case>.npz      seeds, shot, H, p, history flag, ``history`` [B,2,h,w], ``draws__<module>`` [images, 256] in the REFERENCE's
                  image order (per episode: its supports, then its query), ``loss``, ``grad_names``, ``grad_norms`` (-1: frozen),
                  ``grad__<name>`` (every 37th element above 40000 elements), ``draw_seed`` and the two figures of
                  ``_layer5_margin`` (why a case may take a later draw seed than DRAW_SEED)
  <case>_f64.npz  ``loss64``, ``low64`` (low-resolution logits), ``grad_norms64``, ``g64__<name>``
  canet_trajectory.npz   five SGD steps (p = 0, lr 1e-4, momentum 0.9, wd 5e-4) on seeds (3, 4), the history chained as
                  softmax(previous low-resolution logits) from zeros: ``losses32``, ``losses64``

usage:  python tests/golden/make_golden_canet_train.py
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
from tests.golden import make_golden_canet as G  # noqa: E402
from tests.golden.make_golden import _install_standins  # noqa: E402

#: Dropout2d draws: the first seed from DRAW_SEED on that passes ``_layer5_margin`` (stored as ``draw_seed``)
DRAW_SEED, HISTORY_SEED = 78, 5
#: (file, seeds, shot, H, p, history)
CASES = (
    ("canet_trainstep", (3, 4), 1, 97, 0.5, True),
    ("canet_trainstep5", (5,), 5, 97, 0.5, True),
    ("canet_trainstep_nh", (3, 4), 1, 97, 0.0, False),
)
#: gradients stored as samples (the norms of all are stored); layer5.0.weight (3.5 M elements) is held by its norm and by the
#: whole-tensor live check of tests/test_canet_train_gpu.py
SAMPLED = ("layer5.0.bias", "layer55.0.weight", "layer55.0.bias", "residual_1.1.weight", "residual_2.3.bias", "aspp_0.0.weight",
           "aspp_2.0.bias", "layer6.0.weight", "layer7.weight", "layer7.bias")
TRAJ = dict(seeds=(3, 4), steps=5, lr=1e-4, momentum=0.9, weight_decay=5e-4)


def _batch(seeds, shot, H, dtype):
    eps = [synth.make_episode(s, shot=shot, height=H, width=H) for s in seeds]
    sup = torch.from_numpy(np.stack([e["sup_img"] for e in eps])).to(dtype)
    msk = torch.from_numpy(np.stack([e["sup_mask"] for e in eps])).to(dtype)
    qry = torch.from_numpy(np.stack([e["qry_img"] for e in eps])).to(dtype)
    gt = torch.from_numpy(np.concatenate([synth.make_episode(s, shot=shot, height=H, width=H, out_hw=(H, H))["qry_mask"]
                                          for s in seeds]))
    return sup, msk, qry, gt


def _model(history, dtype, p, draws):
    model = G.build_model(history=history).train()
    model.maybe_fix_params(freeze_backbone=True)
    model = model.to(dtype)
    model.layer5[0].register_forward_hook(lambda _m, _i, out: setattr(model, "pre5", out.detach().clone()))   # before the in-place ReLU
    for name, m in model.named_modules():
        if isinstance(m, nn.Dropout2d):
            m.p = p

            def hook(_mod, inp, _out, name=name):
                x = inp[0]
                if p == 0.0:
                    return x
                u = draws[name]
                assert tuple(u.shape) == tuple(x.shape[:2]), (name, u.shape, x.shape)
                return x * ((u < 1 - p).to(x.dtype) / (1 - p))[:, :, None, None]
            m.register_forward_hook(hook)
    return model


def _draws(B, shot, p, seed):
    gen = torch.Generator().manual_seed(seed)
    names = ["layer5.2", "layer55.2"] + [f"aspp_{i}.2" for i in range(5)] + ["layer6.2"]
    d = {k: torch.rand((B * (shot + 1) if k == "layer5.2" else B, 256), generator=gen) for k in names}
    for k, u in d.items():
        assert float((u - (1 - p)).abs().min()) > 1e-6, f"{k}: a draw sits on the keep threshold"
    return d


def _step(seeds, shot, H, p, history, dtype, draws, hist):
    model = _model(history, dtype, p, draws)
    sup, msk, qry, gt = _batch(seeds, shot, H, dtype)
    low = model(sup, msk, qry, False, history_mask=hist[:, None].to(dtype))
    loss = F.cross_entropy(F.interpolate(low, (H, H), mode="bilinear", align_corners=True), gt, ignore_index=255)
    loss.backward()
    return model, float(loss.detach()), low.detach()


def _layer5_margin(pre32, pre64, msk, keep, shot):
    """A support pixel under the mask carries 1 / (masked pixels of its image) of its channel's layer5 gradient (the support
    vector's adjoint hands every masked pixel the same value): with 14 .. 40 masked pixels on a 13 x 13 map ONE ReLU of layer5
    that switches there moves that channel's bias gradient by several per cent, far beyond the 3e-3 of util.check_gradients
    (which absorbs switches on the query side, where 169 pixels share a channel).  A pre-activation closer to zero than the
    reference's OWN float32-vs-float64 difference of that tensor is a coin flip for any float32 implementation, so a fixture
    must hold none among the support positions that carry gradient (masked pixel, channel kept by layer5's Dropout2d).
    -> (smallest |pre-activation| among them in float64, the reference's max |f32 - f64| of layer5's pre-activation)."""
    B, h = msk.shape[0], pre64.shape[-1]
    m = F.interpolate(msk[:, :, 0].reshape(B * shot, 1, *msk.shape[-2:]).double(), (h, h), mode="nearest") > 0
    sup_rows = torch.tensor([b * (shot + 1) + s for b in range(B) for s in range(shot)])        # the reference's image order
    carry = m & keep[sup_rows][:, :, None, None]
    return float(pre64[sup_rows].abs()[carry].min()), float((pre32.double() - pre64).abs().max())


def gen_step(name, seeds, shot, H, p, history):
    B, h = len(seeds), (H - 1) // 8 + 1
    draw_seed = DRAW_SEED
    draws = _draws(B, shot, p, draw_seed)
    if history:
        hist = F.softmax(torch.randn((B, 2, h, h), generator=torch.Generator().manual_seed(HISTORY_SEED)) * 2, dim=1)
    else:
        hist = torch.zeros(B, 2, h, h)
    m32, loss32, low32 = _step(seeds, shot, H, p, history, torch.float32, draws, hist)
    m64, loss64, low64 = _step(seeds, shot, H, p, history, torch.float64, draws, hist)
    msk = _batch(seeds, shot, H, torch.float32)[1]
    while True:               # layer5's pre-activation does not depend on the draws: only which positions carry gradient does
        keep = draws["layer5.2"] < 1 - p if p > 0 else torch.ones_like(draws["layer5.2"], dtype=torch.bool)
        near, margin = _layer5_margin(m32.pre5, m64.pre5, msk, keep, shot)
        if near > margin:
            break
        assert p > 0, f"{name}: a support pre-activation of layer5 lies {near:.1e} from zero (margin {margin:.1e}) without Dropout2d"
        draw_seed += 1
        draws = _draws(B, shot, p, draw_seed)
    if draw_seed != DRAW_SEED:
        m32, loss32, low32 = _step(seeds, shot, H, p, history, torch.float32, draws, hist)
        m64, loss64, low64 = _step(seeds, shot, H, p, history, torch.float64, draws, hist)
    res = {"draw_seed": np.array(draw_seed), "layer5_support_min_abs": np.array(near), "layer5_f32_error": np.array(margin),"seeds": np.array(seeds), "shot": np.array(shot), "H": np.array(H), "p": np.array(p), "use_history": np.array(history),
           "history": hist.numpy(), "loss": np.array(loss32, np.float64), "low32": low32.numpy()}
    res.update({"draws__" + k: v.numpy() for k, v in draws.items()})
    r64 = {"loss64": np.array(loss64, np.float64), "low64": low64.numpy()}
    names, n32, n64 = [], [], []
    p64 = dict(m64.named_parameters())
    for k, q in m32.named_parameters():
        names.append(k)
        n32.append(float(q.grad.norm()) if q.grad is not None else -1.0)
        n64.append(float(p64[k].grad.norm()) if p64[k].grad is not None else -1.0)
        assert (q.grad is None) == (not q.requires_grad) == k.startswith("encoder."), k
        if q.grad is not None:
            assert n32[-1] > 0 and n64[-1] > 0, f"{name}: the gradient of {k} is zero"
    res["grad_names"], res["grad_norms"] = np.array(names), np.array(n32, np.float64)
    r64["grad_norms64"] = np.array(n64, np.float64)
    p32 = dict(m32.named_parameters())
    for k in SAMPLED:
        g, g64 = p32[k].grad, p64[k].grad
        res["grad__" + k] = g.numpy() if g.numel() <= 40000 else g.reshape(-1)[::37].numpy()
        r64["g64__" + k] = g64.numpy() if g64.numel() <= 40000 else g64.reshape(-1)[::37].numpy()
    if history:
        hn = float(p64["residual_1.1.weight"].grad[:, 256:258].norm())
        assert hn > 0, "the history channels of residual_1.1.weight get no gradient"
        r64["history_grad_norm64"] = np.array(hn)
    am = low64.argmax(1)
    for b in range(B):
        assert set(np.unique(am[b].numpy())) == {0, 1}, f"{name}: episode {seeds[b]}: one class only in the low-resolution arg-max"
    np.savez_compressed(OUT / f"{name}.npz", **res)
    np.savez_compressed(OUT / f"{name}_f64.npz", **r64)
    worst = max(float((p32[k].grad.double() - p64[k].grad).norm() / p64[k].grad.norm()) for k in p64 if p64[k].grad is not None)
    print(f"  draw seed {draw_seed}: smallest gradient-carrying support pre-activation of layer5 {near:.2e}, reference f32 error {margin:.2e}")
    print(f"wrote {name}: loss {loss32:.6f} (f64 {loss64:.6f}), worst relative L2 gradient error f32 vs f64 {worst:.1e}, "
          f"logits {float(low64.min()):.1f} .. {float(low64.max()):.1f}, |low32 - low64| {float((low32 - low64).abs().max()):.1e}",
          flush=True)


def _trajectory(dtype):
    seeds, H = TRAJ["seeds"], 97
    model = _model(True, dtype, 0.0, None)
    sup, msk, qry, gt = _batch(seeds, 1, H, dtype)
    h = (H - 1) // 8 + 1
    hist = torch.zeros(len(seeds), 1, 2, h, h, dtype=dtype)
    opt = torch.optim.SGD([q for q in model.parameters() if q.requires_grad], lr=TRAJ["lr"], momentum=TRAJ["momentum"],
                          weight_decay=TRAJ["weight_decay"])
    losses = []
    for _ in range(TRAJ["steps"]):
        opt.zero_grad()
        low = model(sup, msk, qry, False, history_mask=hist)
        loss = F.cross_entropy(F.interpolate(low, (H, H), mode="bilinear", align_corners=True), gt, ignore_index=255)
        loss.backward()
        opt.step()
        hist = F.softmax(low.detach(), dim=1)[:, None]
        losses.append(float(loss))
    return np.array(losses, np.float64)


def gen_trajectory():
    l32, l64 = _trajectory(torch.float32), _trajectory(torch.float64)
    assert l64[-1] < 0.5 * l64[0], f"the trajectory does not descend: {l64}"
    np.savez_compressed(OUT / "canet_trajectory.npz", seeds=np.array(TRAJ["seeds"]), H=np.array(97), lr=np.array(TRAJ["lr"]),
                        momentum=np.array(TRAJ["momentum"]), weight_decay=np.array(TRAJ["weight_decay"]), losses32=l32, losses64=l64)
    print("wrote canet_trajectory: f64", [round(float(v), 4) for v in l64], "gap", [f"{abs(a - b):.1e}" for a, b in zip(l32, l64)],
          flush=True)


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
