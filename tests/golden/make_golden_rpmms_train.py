#!/usr/bin/env python3
"""Generate the RPMMs train-step fixtures under tests/golden/ from the REFERENCE itself (networks/rpmms.py in train() mode).

Runs only in the build container (needs /root/reference), on the CPU, in about three minutes.  Built like make_golden_canet_train.py
on top of make_golden_rpmms.py's patches: the unmodified reference ``RPMMs`` with wgen weights (seed 1259) in ``train()`` mode,
every ``model_res`` parameter frozen HERE (the reference's ``maybe_fix_params`` freezes nothing for RPMMs; the HIP path trains
the head behind a frozen trunk).  The three initial ``mu`` of the EM are drawn once after ``torch.manual_seed(7)`` and handed to
every run of both precisions.  The ``nn.Dropout2d`` modules get forward hooks that keep a call counter per module and replace
the output by ``input * keep / (1 - p)``, keep where the STORED uniform of that call is < 1 - p (the rule of oracle/ref_cpu.py and
train_ops.dropout2d_mask(uniforms=...)): ``layer55.2`` is called ten times per forward (once per prototype, rpmms.py:237-244),
``layer56.2``, the five ``layer6.aspp_k.2`` and ``layer7.2`` three times (once per pass).  Every draw is at least 1e-6 from the
threshold.  Each step runs in float32 and in float64 (the same model ``.double()``).

Seed condition.  The EM amplifies rounding: a fixture is only useful if the reference's own float32 prototypes stay as close to
its float64 ones as its eval-mode float32 logits stay to float64 in ``rpmms_small`` (the largest stored ``f64_err_p*`` there).
A seed pair that misses this is skipped for the next of SEED_PAIRS; the pair used is stored (``seeds``, ``seed_pair``) with both
figures (``proto_err``, ``proto_limit``).  For the trajectory the condition is on its FIRST step, the one both precisions start
from the same weights.  Checked on this CPU when the committed files were written: the first pair, (3, 4), holds for all three
cases with 2.76e-5 against a limit of 1.84e-4.

Draw condition.  With Wgen weights the three cross-entropies are 6 .. 10, the gradient sits on few pixels, and a single ReLU of
the head that switches can move a gradient by more than the 3e-3 that tests/util.check_gradients allows for switches in all.
Whether a float32 evaluation meets such a switch is decided by the trunk's float32 rounding, which differs between any two
implementations.  So a p > 0 fixture must be stable under the reference's OWN float32 error: the float64 step is repeated
PROBES times with the queries' trunk features (layer2, layer3) moved by |reference float32 - reference float64| with random
signs -- what another float32 trunk's error looks like -- and every sampled gradient must stay within STABLE = eps / 2 = 1.5e-3
(relative L2) of the unperturbed float64 gradient: half of the allowance is left to the implementation's own head rounding
and to a trunk error somewhat larger than the reference's.  The Dropout2d draws decide which units carry gradient, so the
draw seed is the first from DRAW_SEED on that passes (stored: ``draw_seed``, ``stability``, ``stable_limit``).  Only the
reference is run for this.  Found on this CPU when the committed files were written: seeds 78 .. 82 respond with 3.9e-3, 3.8e-3, 1.8e-3, 3.6e-3, 3.4e-3 and are skipped, seed 83 with 1.09e-3 is used.  The p = 0 case has no
draws to choose; its figure is stored for information.

Files (key layout of tests/util.check_gradients):
  <case>.npz      seeds, seed_pair, H, p, ``mu0_k<K>`` [256,K], ``draws__<module>`` [calls,B,256], ``loss`` (sum, CE of out2, CE of
                  out1), ``low32_p<pass>``, ``mu_f32_k<K>`` / ``mu_b32_k<K>``, ``grad_names``, ``grad_norms`` (-1: frozen),
                  ``grad__<name>`` (every 37th element above 40000 elements), ``proto_err``, ``proto_limit``, ``draw_seed``,
                  ``stability``, ``stable_limit``
  <case>_f64.npz  ``loss64``, ``low64_p<pass>``, ``mu_f64_k<K>`` / ``mu_b64_k<K>``, ``grad_norms64``, ``g64__<name>``,
                  ``history_grad_norm64`` (of residule1.1.weight[:, 256:258])
  rpmms_trajectory.npz   five SGD steps (p = 0, lr 1e-4, momentum 0.9, wd 5e-4), the initial mu pinned for all five:
                  ``losses32``, ``losses64`` [5,3]

usage:  python tests/golden/make_golden_rpmms_train.py
"""
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn as nn

ROOT = Path(__file__).resolve().parents[2]
REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

from pemp_amd import synth  # noqa: E402
from tests.golden import make_golden_rpmms as G  # noqa: E402
from tests.golden.make_golden import _install_standins  # noqa: E402

#: Dropout2d draws: the first seed from DRAW_SEED on that passes the draw condition (module docstring)
DRAW_SEED, MAX_DRAW_SEEDS = 78, 16
#: the draw condition: probes per candidate, their generator seeds, the largest relative L2 response of a sampled gradient
PROBES, PROBE_SEED, STABLE = 8, 1000, 1.5e-3
#: the seed pairs tried in order (module docstring: seed condition)
SEED_PAIRS = ((3, 4), (5, 6), (7, 8), (9, 10))
#: (file, H, p)
CASES = (("rpmms_trainstep", 97, 0.5), ("rpmms_trainstep_p0", 97, 0.0))
#: calls per forward of every Dropout2d module
DROP_CALLS = {"layer55.2": 10, "layer56.2": 3, "layer7.2": 3, **{f"layer6.aspp_{i}.2": 3 for i in range(5)}}
#: gradients stored as samples (the norms of all are stored)
SAMPLED = ("layer5.1.weight", "layer5.1.bias", "layer55.0.weight", "layer55.0.bias", "layer56.0.weight", "residule1.1.weight",
           "residule2.3.bias", "layer6.aspp_2.0.weight", "layer7.0.weight", "layer9.weight", "layer9.bias")
#: layer5's conv bias sits in front of a batch-statistics BatchNorm: its gradient is zero up to rounding
ZERO_GRAD = ("layer5.0.bias",)
TRAJ = dict(steps=5, lr=1e-4, momentum=0.9, weight_decay=5e-4)


def _batch(seeds, H, dtype):
    eps = [synth.make_episode(s, shot=1, height=H, width=H) for s in seeds]
    sup = torch.from_numpy(np.stack([e["sup_img"] for e in eps])).to(dtype)
    msk = torch.from_numpy(np.stack([e["sup_mask"] for e in eps])).to(dtype)
    qry = torch.from_numpy(np.stack([e["qry_img"] for e in eps])).to(dtype)
    gt = torch.from_numpy(np.concatenate([synth.make_episode(s, shot=1, height=H, width=H, out_hw=(H, H))["qry_mask"] for s in seeds]))
    assert int(gt.max()) <= 1, "the reference's loss has no ignore index"
    return sup, msk, qry, gt


def _model(dtype, p, draws):
    model = G.build_model().train()
    for q in model.model_res.parameters():
        q.requires_grad = False
    model = model.to(dtype)
    calls = {}
    for name, m in model.named_modules():
        if isinstance(m, nn.Dropout2d):
            assert name in DROP_CALLS, name
            m.p = p

            def hook(_mod, inp, _out, name=name):
                x = inp[0]
                n = calls[name] = calls.get(name, -1) + 1
                if p == 0.0:
                    return x
                u = draws[name][n % DROP_CALLS[name]]
                assert tuple(u.shape) == tuple(x.shape[:2]), (name, u.shape, x.shape)
                return x * ((u < 1 - p).to(x.dtype) / (1 - p))[:, :, None, None]
            m.register_forward_hook(hook)
    model.drop_calls = calls
    return model


def _draws(B, p, seed):
    gen = torch.Generator().manual_seed(seed)
    d = {k: torch.rand((n, B, 256), generator=gen) for k, n in DROP_CALLS.items()}
    for k, u in d.items():
        assert float((u - (1 - p)).abs().min()) > 1e-6, f"{k}: a draw sits on the keep threshold"
    return d


def _mu0():
    """The three initial mu the reference draws after torch.manual_seed(7), K = 1, 3, 6 in this order (rpmms.py:41-43,232-234)."""
    from networks import rpmms
    torch.manual_seed(G.MU_SEED)
    G.STATE.update(force=None, drawn={}, protos={})
    for k in G.KS:
        rpmms.PMMs(256, k)
    return {k: v.clone() for k, v in G.STATE["drawn"].items()}


def _forward_backward(model, batch, dtype, mu0):
    sup, msk, qry, gt = batch
    G.STATE.update(force={k: v.to(dtype) for k, v in mu0.items()}, protos={})
    logits = model(sup, msk, qry)
    losses = model.get_loss(logits, gt[:, None])
    losses[0].backward()
    protos = {k: (a.clone(), b.clone()) for k, (a, b) in G.STATE["protos"].items()}
    G.STATE["force"] = None
    return [float(v.detach()) for v in losses], [o.detach() for o in logits[1:]], protos


def _trunk_hook(model, store=None, add=None):
    """Forward hook on ``model_res``, whose second call of a forward is the queries' (rpmms.py:222-225): ``store`` (a list) takes
    that call's (layer2, layer3), ``add`` = (d2, d3) is added to them."""
    calls = [0]

    def hook(_mod, _inp, out):
        calls[0] += 1
        if calls[0] % 2:
            return None
        if store is not None:
            store[:] = [out[1].detach().clone(), out[2].detach().clone()]
        return None if add is None else (out[0], out[1] + add[0], out[2] + add[1])
    model.model_res.register_forward_hook(hook)


def _step(seeds, H, p, dtype, draws, mu0, store=None, add=None):
    model = _model(dtype, p, draws)
    _trunk_hook(model, store, add)
    out = _forward_backward(model, _batch(seeds, H, dtype), dtype, mu0)
    assert {k: v + 1 for k, v in model.drop_calls.items()} == DROP_CALLS, model.drop_calls
    return (model,) + out


def _proto_limit():
    g = np.load(OUT / "rpmms_small.npz")
    return max(float(g[f"f64_err_p{p}"]) for p in range(3))


def _proto_err(pr32, pr64):
    return max(float((pr32[k][s].double() - pr64[k][s]).abs().max()) for k in G.KS for s in (0, 1))


def _stability(seeds, H, p, draws, mu0, m64, delta, stop=None):
    """The draw condition's figure: the largest relative L2 change of a sampled float64 gradient over PROBES float64 steps whose
    query trunk features are moved by ``delta`` = |float32 - float64| with random signs (``stop``: give up beyond it)."""
    base = {k: q.grad.clone() for k, q in m64.named_parameters() if k in SAMPLED}
    worst = 0.0
    for n in range(PROBES):
        gen = torch.Generator().manual_seed(PROBE_SEED + n)
        add = [d * (torch.randint(0, 2, d.shape, generator=gen).double() * 2 - 1) for d in delta]
        grads = dict(_step(seeds, H, p, torch.float64, draws, mu0, add=add)[0].named_parameters())
        worst = max(worst, max(float((grads[k].grad - g).norm() / g.norm()) for k, g in base.items()))
        if stop is not None and worst > stop:
            break
    return worst


def gen_step(name, H, p, mu0, limit):
    for pair, seeds in enumerate(SEED_PAIRS):
        B = len(seeds)
        draws = _draws(B, p, DRAW_SEED)
        f32, f64 = [], []
        m32, loss32, low32, pr32 = _step(seeds, H, p, torch.float32, draws, mu0, store=f32)
        m64, loss64, low64, pr64 = _step(seeds, H, p, torch.float64, draws, mu0, store=f64)
        err = _proto_err(pr32, pr64)
        print(f"  {name}: seeds {seeds}: |prototypes f32 - f64| {err:.2e} (limit {limit:.2e})", flush=True)
        if err <= limit:
            break
    else:
        raise AssertionError(f"{name}: no seed pair of {SEED_PAIRS} keeps the float32 prototypes within {limit:.2e} of float64")
    delta = [(a.double() - b).abs() for a, b in zip(f32, f64)]          # the trunk does not see the draws
    draw_seed = DRAW_SEED
    while True:
        stab = _stability(seeds, H, p, draws, mu0, m64, delta, stop=STABLE if p > 0 else None)
        print(f"  {name}: draw seed {draw_seed}: largest response of a sampled gradient to a float32-sized trunk difference {stab:.2e} "
              f"(limit {STABLE:.1e})", flush=True)
        if stab <= STABLE or p == 0:
            break
        draw_seed += 1
        assert draw_seed < DRAW_SEED + MAX_DRAW_SEEDS, f"{name}: no draw seed passes the draw condition"
        draws = _draws(B, p, draw_seed)
        m64, loss64, low64, pr64 = _step(seeds, H, p, torch.float64, draws, mu0)
    if draw_seed != DRAW_SEED:
        m32, loss32, low32, pr32 = _step(seeds, H, p, torch.float32, draws, mu0)
    res = {"seeds": np.array(seeds), "seed_pair": np.array(pair), "H": np.array(H), "p": np.array(p), "draw_seed": np.array(draw_seed),
           "stability": np.array(stab), "stable_limit": np.array(STABLE),
           "proto_err": np.array(err), "proto_limit": np.array(limit), "loss": np.array(loss32, np.float64)}
    r64 = {"loss64": np.array(loss64, np.float64)}
    for k in G.KS:
        res[f"mu0_k{k}"] = mu0[k][0].numpy()
        res[f"mu_f32_k{k}"], res[f"mu_b32_k{k}"] = pr32[k][0].numpy(), pr32[k][1].numpy()
        r64[f"mu_f64_k{k}"], r64[f"mu_b64_k{k}"] = pr64[k][0].numpy(), pr64[k][1].numpy()
    for q in range(3):
        res[f"low32_p{q}"], r64[f"low64_p{q}"] = low32[q].numpy(), low64[q].numpy()
    res.update({"draws__" + k: v.numpy() for k, v in draws.items()})
    names, n32, n64 = [], [], []
    p32, p64 = dict(m32.named_parameters()), dict(m64.named_parameters())
    for k, q in p32.items():
        names.append(k)
        n32.append(float(q.grad.norm()) if q.grad is not None else -1.0)
        n64.append(float(p64[k].grad.norm()) if p64[k].grad is not None else -1.0)
        assert (q.grad is None) == (not q.requires_grad) == k.startswith("model_res."), k
        if q.grad is not None and k not in ZERO_GRAD:
            assert n32[-1] > 0 and n64[-1] > 0, f"{name}: the gradient of {k} is zero"
    res["grad_names"], res["grad_norms"] = np.array(names), np.array(n32, np.float64)
    r64["grad_norms64"] = np.array(n64, np.float64)
    for k in SAMPLED:
        g, g64 = p32[k].grad, p64[k].grad
        res["grad__" + k] = g.numpy() if g.numel() <= 40000 else g.reshape(-1)[::37].numpy()
        r64["g64__" + k] = g64.numpy() if g64.numel() <= 40000 else g64.reshape(-1)[::37].numpy()
    hn = float(p64["residule1.1.weight"].grad[:, 256:258].norm())
    assert hn > 0, "the history channels of residule1.1.weight get no gradient"
    r64["history_grad_norm64"] = np.array(hn)
    np.savez_compressed(OUT / f"{name}.npz", **res)
    np.savez_compressed(OUT / f"{name}_f64.npz", **r64)
    worst = max(float((p32[k].grad.double() - p64[k].grad).norm() / p64[k].grad.norm()) for k in p64
                if p64[k].grad is not None and k not in ZERO_GRAD)
    print(f"wrote {name}: losses {[round(v, 6) for v in loss32]} (f64 {[round(v, 6) for v in loss64]}), worst relative L2 gradient "
          f"error f32 vs f64 {worst:.1e}, |low32 - low64| {[f'{float((a - b).abs().max()):.1e}' for a, b in zip(low32, low64)]}, "
          f"|grad layer5.0.bias| {float(p64['layer5.0.bias'].grad.norm()):.1e}", flush=True)
    return seeds


def _trajectory(seeds, dtype, mu0):
    model = _model(dtype, 0.0, None)
    batch = _batch(seeds, 97, dtype)
    opt = torch.optim.SGD([q for q in model.parameters() if q.requires_grad], lr=TRAJ["lr"], momentum=TRAJ["momentum"],
                          weight_decay=TRAJ["weight_decay"])
    losses = []
    for n in range(TRAJ["steps"]):
        opt.zero_grad()
        ls, _, pr = _forward_backward(model, batch, dtype, mu0)
        opt.step()
        losses.append(ls)
        protos = pr if n == 0 else protos          # the seed condition is about the step both precisions start from the same weights
    return np.array(losses, np.float64), protos


def gen_trajectory(mu0, limit):
    for pair, seeds in enumerate(SEED_PAIRS):
        (l32, pr32), (l64, pr64) = _trajectory(seeds, torch.float32, mu0), _trajectory(seeds, torch.float64, mu0)
        err = _proto_err(pr32, pr64)
        print(f"  rpmms_trajectory: seeds {seeds}: |prototypes f32 - f64| in the first step {err:.2e} (limit {limit:.2e})", flush=True)
        if err <= limit:
            break
    else:
        raise AssertionError("rpmms_trajectory: no seed pair keeps the float32 prototypes within the limit")
    assert l64[-1, 0] < l64[0, 0], f"the trajectory does not descend: {l64[:, 0]}"
    np.savez_compressed(OUT / "rpmms_trajectory.npz", seeds=np.array(seeds), seed_pair=np.array(pair), H=np.array(97), lr=np.array(TRAJ["lr"]),
                        momentum=np.array(TRAJ["momentum"]), weight_decay=np.array(TRAJ["weight_decay"]), losses32=l32, losses64=l64,
                        proto_err=np.array(err), proto_limit=np.array(limit), **{f"mu0_k{k}": mu0[k][0].numpy() for k in G.KS})
    print("wrote rpmms_trajectory: f64", [round(float(v), 4) for v in l64[:, 0]], "gap", [f"{abs(a - b):.1e}" for a, b in zip(l32[:, 0], l64[:, 0])],
          flush=True)


def main():
    torch.set_num_threads(8)
    torch.manual_seed(0)
    _install_standins()
    sys.path.insert(0, str(REF))
    from networks import rpmms
    G.install_patches(rpmms)
    mu0, limit = _mu0(), _proto_limit()
    for case in CASES:
        gen_step(*case, mu0, limit)
    gen_trajectory(mu0, limit)


if __name__ == "__main__":
    main()
