"""Functional torch restatement of CANet's head in train() mode (reference networks/canet.py:163-209 + the bilinear upsample and
cross-entropy of entry/canet.py:107-116), from the ``cat((f2, f3))`` features to the loss, differentiated by autograd -- test
infrastructure.  Pinned by the reference-made fixtures of tests/golden/make_golden_canet_train.py (tests/test_canet_train_cpu.py
holds it to their losses and gradient norms in float64), not trusted on its own; the GPU tests then use it on the engine's own
trunk features, which separates the head's arithmetic from the trunk's rounding.

Image order: [all supports | all queries] (the engines' layout), NHWC features, Dropout2d draws [images, channels] per
reference module name -- keep where u < 1 - p, the rule of oracle/ref_cpu.py: Dropout2d and train_ops.dropout2d_mask."""
import torch
import torch.nn.functional as F

DROPS = ("layer5.2", "layer55.2", "aspp_0.2", "aspp_1.2", "aspp_2.2", "aspp_3.2", "aspp_4.2", "layer6.2")
#: the 30 head tensors, in ``model.parameters()`` order
HEAD = tuple(f"{m}.{k}" for m in ("layer5.0", "layer55.0", "aspp_0.0", "aspp_1.0", "aspp_2.0", "aspp_3.0", "aspp_4.0", "layer6.0",
                                  "residual_1.1", "residual_1.3", "residual_2.1", "residual_2.3", "residual_3.1", "residual_3.3",
                                  "layer7") for k in ("weight", "bias"))


def keep_mask(u, p, dtype):
    """Dropout2d's multiplier from its uniform draws: (u < 1 - p) / (1 - p)."""
    return (u < 1 - p).to(dtype) / (1 - p)


def trunk_cat23(sd, sup_img, qry_img, dtype=torch.float64, train_bn=True):
    """The frozen trunk by the oracle's ResNet restatement -> cat((f2, f3)) NHWC [B*S + B, h, w, 1536], supports first.
    ``train_bn`` (the reference's training step): ``freeze_bn`` there only stops the BatchNorms' affine parameters from
    training (networks/backbones.py:56-62,93-95) -- in ``train()`` mode they still normalise with the statistics of the batch,
    all B(S+1) images together.  ``sd`` is not changed (the running statistics move in a copy)."""
    from oracle import ref_cpu
    sd = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items() if k.startswith("encoder.")}
    x = torch.cat((sup_img.flatten(0, 1), qry_img.flatten(0, 1))).to(dtype)
    saved, ref_cpu.TRAIN = ref_cpu.TRAIN, bool(train_bn)
    try:
        with torch.no_grad():
            x = ref_cpu.resnet_stem(x, sd, "encoder")
            f1 = ref_cpu._res_layer(x, sd, "encoder", "layer1", 3)
            f2 = ref_cpu._res_layer(f1, sd, "encoder", "layer2", 4)
            f3 = ref_cpu._res_layer(f2, sd, "encoder", "layer3", 6)
    finally:
        ref_cpu.TRAIN = saved
    return torch.cat((f2, f3), dim=1).permute(0, 2, 3, 1).contiguous()


def head_logits(cat23, sup_mask, prm, B, S, history=None, draws=None, p=0.0, use_history=True):
    """cat23 NHWC [B*S + B, h, w, 1536]; sup_mask [B,S,2,H,W]; ``prm``: {reference key: tensor} of the head; ``history``
    [B,2,h,w] or None (zeros); ``draws``: {name of DROPS: uniforms} (needed when p > 0) -> low-resolution logits [B,2,h,w]."""
    dt = cat23.dtype

    def drop(x, name):
        return x if p == 0.0 else x * keep_mask(draws[name], p, dt)[:, :, None, None]

    def conv(x, name, dil=1, k=3):
        return F.conv2d(x, prm[name + ".weight"], prm[name + ".bias"], 1, dil if k == 3 else 0, dil)

    ns = B * S
    x = cat23.permute(0, 3, 1, 2)
    f5 = drop(F.relu(conv(x, "layer5.0", 2)), "layer5.2")
    h, w = f5.shape[-2:]
    H, W = sup_mask.shape[-2:]
    m = F.interpolate(sup_mask[:, :, 0].reshape(ns, 1, H, W).to(dt), (h, w), mode="nearest")
    z = (f5[:ns] * m).sum(dim=(2, 3)) / (m.sum(dim=(2, 3)) + 1e-5)
    z = z.view(B, S, -1).mean(dim=1)
    out = torch.cat((f5[ns:], z[:, :, None, None].expand(-1, -1, h, w)), dim=1)
    out = drop(F.relu(conv(out, "layer55.0", 2)), "layer55.2")
    for k in (1, 2, 3):
        inp = out
        if k == 1 and use_history:
            hist = torch.zeros((B, 2, h, w), dtype=dt) if history is None else history.to(dt)
            inp = torch.cat((out, hist), dim=1)
        out = out + conv(F.relu(conv(F.relu(inp), f"residual_{k}.1")), f"residual_{k}.3")
    g = drop(F.relu(conv(F.avg_pool2d(out, (h, w)), "aspp_0.0", k=1)), "aspp_0.2").expand(-1, -1, h, w)
    br = [g, drop(F.relu(conv(out, "aspp_1.0", k=1)), "aspp_1.2")]
    br += [drop(F.relu(conv(out, f"aspp_{i}.0", d)), f"aspp_{i}.2") for i, d in ((2, 6), (3, 12), (4, 18))]
    out = drop(F.relu(conv(torch.cat(br, dim=1), "layer6.0", k=1)), "layer6.2")
    return conv(out, "layer7", k=1)


def loss_of(low, target, weight=None):
    """Bilinear (align_corners) upsample to the target's size + CE(ignore 255); ``weight``: CELossDT's map (core/losses.py:33-43)."""
    logits = F.interpolate(low, tuple(target.shape[-2:]), mode="bilinear", align_corners=True)
    if weight is not None:
        ce = F.cross_entropy(logits, target, ignore_index=255, reduction="none")
        return (ce * weight.to(low.dtype)).sum() / weight.to(low.dtype).sum()
    return F.cross_entropy(logits, target, ignore_index=255)


def head_step(cat23, sup_mask, target, sd, B, S, dtype, history=None, draws=None, p=0.0, use_history=True):
    """One forward + backward of the head in ``dtype`` -> (loss float, low-resolution logits, {key: gradient} of the head)."""
    prm = {k: sd[k].detach().to(dtype).clone().requires_grad_(True) for k in HEAD}
    dr = None if draws is None else {k: v.detach().cpu() for k, v in draws.items()}
    low = head_logits(cat23.detach().to(dtype), sup_mask, prm, B, S, history, dr, p, use_history)
    loss = loss_of(low, target)
    grads = torch.autograd.grad(loss, [prm[k] for k in HEAD])
    return float(loss.detach()), low.detach(), dict(zip(HEAD, grads))


# -- the fixtures of tests/golden/make_golden_canet_train.py -------------------------------------------------------------------
def _ref_order_to_engine(B, S):
    """Row permutation that takes the reference's image order (per episode: its supports, then its query) to the engine's
    [all supports | all queries]."""
    return torch.tensor([b * (S + 1) + s for b in range(B) for s in range(S)] + [b * (S + 1) + S for b in range(B)])


def fixture_state_dict(history=True):
    """The fixtures' weights: wgen seed 1259 over the key layout of the model (``history=False``: residual_1.1 sees 256 channels)."""
    from pemp_amd import synth
    from pemp_amd.networks import canet
    if history:
        from tests import util
        return util.wgen_state_dict("canet", seed=1259)
    return synth.wgen_state_dict_for(canet.CaNet(None, init_channels=3, drop_rate=0.5, history=False, freeze_backbone=True), seed=1259)


def fixture_inputs(name):
    """The fixture's episode batch, history and draws (rows of layer5.2 in the engines' image order) on the CPU."""
    from pemp_amd import synth
    from tests import util
    g = util.gold(name)
    seeds, shot, H = [int(s) for s in g["seeds"]], int(g["shot"]), int(g["H"])
    b = synth.make_batch(seeds, shot=shot, height=H, width=H, out_hw=(H, H))
    sup, msk, qry = (torch.from_numpy(b[k]) for k in ("sup_img", "sup_mask", "qry_img"))
    gt = torch.from_numpy(b["qry_mask"]).reshape(-1, H, H)
    draws = {k: torch.from_numpy(g["draws__" + k]) for k in DROPS}
    draws["layer5.2"] = draws["layer5.2"][_ref_order_to_engine(len(seeds), shot)].contiguous()
    return g, sup, msk, qry, gt, torch.from_numpy(g["history"]), draws
