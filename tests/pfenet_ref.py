"""Functional torch restatement of PFENet's training step (reference networks/pfenet.py:157-285 in train() mode + the loss of
entry/pfenet.py:63-71) -- test infrastructure.  Two parts:

* ``trunk_features``: the deep-base trunk with batch-statistics BatchNorm, called as the reference calls it (once for the
  queries, once per shot) or, to show why that matters, in one pass over all images or with the running statistics;
* ``head_step``: the head from ``cat(layer3, layer2)``, the support masks at feature resolution and the prior to the two
  losses, differentiated by autograd, in a given dtype.

Pinned by the reference-made fixtures of tests/golden/make_golden_pfenet_train.py (tests/test_pfenet_train_cpu.py holds it to
their float64 losses), not trusted on its own; the GPU tests then use ``head_step`` on the engine's own trunk features, which
separates the head's arithmetic from the trunk's rounding.

Image order of the supports: row b * S + s (the engines' layout), NHWC features, Dropout2d draws [rows, channels] per reference
module name -- keep where u < 1 - p, the rule of train_ops.dropout2d_mask."""
import torch
import torch.nn.functional as F

BINS = (60, 30, 15, 8)
DROPS = {"down_query.2": 0.5, "down_supp.2": 0.5, "cls.2": 0.1, **{f"inner_cls.{i}.2": 0.1 for i in range(4)}}
TRUNK = ("layer0.", "layer1.", "layer2.", "layer3.", "layer4.")
_AC = dict(mode="bilinear", align_corners=True)


def head_keys(sd):
    """The head's parameters in ``state_dict`` order (everything outside layer0 .. layer4)."""
    return [k for k in sd if not k.startswith(TRUNK)]


def keep_mask(u, p, dtype):
    return (u < 1 - p).to(dtype) / (1 - p)


# -- trunk ------------------------------------------------------------------------------------------------------------------
def _bn(x, sd, name, train):
    return F.batch_norm(x, sd[name + ".running_mean"], sd[name + ".running_var"], sd[name + ".weight"], sd[name + ".bias"], train,
                        0.1, 1e-5)


def _layer(x, sd, name, blocks, stride, dil, train):
    for i in range(blocks):
        p, s = f"{name}.{i}", stride if i == 0 else 1
        out = F.relu(_bn(F.conv2d(x, sd[p + ".conv1.weight"]), sd, p + ".bn1", train))
        out = F.relu(_bn(F.conv2d(out, sd[p + ".conv2.weight"], None, s, dil, dil), sd, p + ".bn2", train))
        out = _bn(F.conv2d(out, sd[p + ".conv3.weight"]), sd, p + ".bn3", train)
        res = x
        if p + ".downsample.0.weight" in sd:
            res = _bn(F.conv2d(x, sd[p + ".downsample.0.weight"], None, s), sd, p + ".downsample.1", train)
        x = F.relu(out + res)
    return x


def _trunk_call(x, sd, train, mask=None):
    """layer0 .. layer4 on one batch -> (layer2, layer3, layer4); ``mask`` [n,1,H,W] binary: layer 4 reads layer3 * its bilinear
    resize (pfenet.py:191-193); moves the running statistics in ``sd`` when ``train``."""
    x = F.relu(_bn(F.conv2d(x, sd["layer0.0.weight"], None, 2, 1), sd, "layer0.1", train))
    x = F.relu(_bn(F.conv2d(x, sd["layer0.3.weight"], None, 1, 1), sd, "layer0.4", train))
    x = F.relu(_bn(F.conv2d(x, sd["layer0.6.weight"], None, 1, 1), sd, "layer0.7", train))
    x = F.max_pool2d(x, 3, 2, 1)
    f1 = _layer(x, sd, "layer1", 3, 1, 1, train)
    f2 = _layer(f1, sd, "layer2", 4, 2, 1, train)
    f3 = _layer(f2, sd, "layer3", 6, 1, 2, train)
    x4 = f3 if mask is None else f3 * F.interpolate(mask, f3.shape[-2:], **_AC)
    return f2, f3, _layer(x4, sd, "layer4", 3, 1, 4, train)


def _prior(q4, s4_list, masks):
    """pfenet.py:201-231 (the two identity resizes left out)."""
    out = []
    for s4, m in zip(s4_list, masks):
        s = s4 * F.interpolate(m, s4.shape[-2:], **_AC)
        b, c, sp, _ = q4.shape
        qv, sv = q4.reshape(b, c, -1), s.reshape(b, c, -1).permute(0, 2, 1)
        sim = torch.bmm(sv, qv) / (torch.bmm(sv.norm(dim=2, keepdim=True), qv.norm(dim=1, keepdim=True)) + 1e-7)
        sim = sim.max(1)[0]
        sim = (sim - sim.min(1)[0].unsqueeze(1)) / (sim.max(1)[0].unsqueeze(1) - sim.min(1)[0].unsqueeze(1) + 1e-7)
        out.append(sim.view(b, 1, sp, sp))
    return torch.cat(out, 1).mean(1)


def trunk_features(sd, sup_img, sup_mask, qry_img, dtype=torch.float64, mode="per_call"):
    """-> (cat_q NHWC [B,h,w,1536], cat_s NHWC [B*S,h,w,1536] rows b * S + s, mfeat float32 [B*S,h,w], prior [B,h,w], the trunk's state
    after the step).  ``mode``: "per_call" -- the reference's S + 1 train-mode calls (query, shot 0, shot 1, ...); "one_pass" --
    one train-mode call over all B (S + 1) images; "eval" -- the running statistics.  ``sd`` itself is not changed."""
    sd = {k: (v.detach().to(dtype).clone() if v.is_floating_point() else v.clone()) for k, v in sd.items() if k.startswith(TRUNK)}
    B, S = sup_img.shape[:2]
    qry, sup = qry_img.flatten(0, 1).to(dtype), sup_img.to(dtype)
    masks = [(sup_mask[:, s, 0:1] == 1).float() for s in range(S)]          # float32 whatever the dtype, as pfenet.py:184 makes them
    with torch.no_grad():
        if mode == "one_pass":
            x = torch.cat([qry] + [sup[:, s] for s in range(S)])
            m = torch.cat([torch.ones_like(masks[0])] + masks)
            f2, f3, f4 = _trunk_call(x, sd, True, m)
            outs = [(f2[i * B:(i + 1) * B], f3[i * B:(i + 1) * B], f4[i * B:(i + 1) * B]) for i in range(S + 1)]
        else:
            train = mode == "per_call"
            outs = [_trunk_call(qry, sd, train)] + [_trunk_call(sup[:, s], sd, train, masks[s]) for s in range(S)]
        h, w = outs[0][1].shape[-2:]
        nhwc = lambda f2, f3: torch.cat((f3, f2), dim=1).permute(0, 2, 3, 1)
        cat_q = nhwc(*outs[0][:2]).contiguous()
        cat_s = torch.stack([nhwc(*o[:2]) for o in outs[1:]], dim=1).flatten(0, 1).contiguous()
        mfeat = torch.stack([F.interpolate(m, (h, w), **_AC)[:, 0] for m in masks], dim=1).flatten(0, 1).contiguous()
        prior = _prior(outs[0][2], [o[2] for o in outs[1:]], masks)
    return cat_q, cat_s, mfeat, prior, sd


# -- head -------------------------------------------------------------------------------------------------------------------
def head_forward(cat_q, cat_s, mfeat, prior, prm, S, draws=None, drop=True):
    """``prm``: {reference key: tensor} of the head; ``draws``: {name of DROPS: uniforms} (needed with ``drop``) -> (low-resolution
    logits [B,2,h,w], the four inner logits)."""
    dt = cat_q.dtype

    def dr(x, name):
        return x * keep_mask(draws[name].to("cpu"), DROPS[name], dt)[:, :, None, None] if drop else x

    def c1(x, name):
        return F.conv2d(x, prm[name + ".weight"], prm.get(name + ".bias"))

    def c3(x, name):
        return F.conv2d(x, prm[name + ".weight"], None, 1, 1)

    q = dr(F.relu(c1(cat_q.permute(0, 3, 1, 2), "down_query.0")), "down_query.2")
    s = dr(F.relu(c1(cat_s.permute(0, 3, 1, 2), "down_supp.0")), "down_supp.2")
    B, _, h, w = q.shape
    m = mfeat[:, None]                                                        # float32 (see trunk_features): so is the area
    area = F.avg_pool2d(m, (h, w)) * h * w + 0.0005                           # Weighted_GAP, pfenet.py:15-20
    v = (F.avg_pool2d(s * m, (h, w)) * h * w / area).view(B, S, -1, 1, 1)
    supp = v[:, 0]
    for i in range(1, S):
        supp = supp + v[:, i]
    if S > 1:
        supp = supp / S
    pr = prior[:, None].to(dt)
    pyr, inner = [], []
    for idx, b in enumerate(BINS):
        merge = torch.cat((F.adaptive_avg_pool2d(q, b), supp.expand(-1, -1, b, b), F.interpolate(pr, (b, b), **_AC)), dim=1)
        merge = F.relu(c1(merge, f"init_merge.{idx}.0"))
        if idx >= 1:
            pre = F.interpolate(pyr[idx - 1], (b, b), **_AC)
            merge = F.relu(c1(torch.cat((merge, pre), dim=1), f"alpha_conv.{idx - 1}.0")) + merge
        merge = F.relu(c3(F.relu(c3(merge, f"beta_conv.{idx}.0")), f"beta_conv.{idx}.2")) + merge
        inner.append(c1(dr(F.relu(c3(merge, f"inner_cls.{idx}.0")), f"inner_cls.{idx}.2"), f"inner_cls.{idx}.3"))
        pyr.append(F.interpolate(merge, (h, w), **_AC))
    x = F.relu(c1(torch.cat(pyr, dim=1), "res1.0"))
    x = F.relu(c3(F.relu(c3(x, "res2.0")), "res2.2")) + x
    return c1(dr(F.relu(c3(x, "cls.0")), "cls.2"), "cls.3"), inner


def ce(low, target):
    return F.cross_entropy(F.interpolate(low, tuple(target.shape[-2:]), **_AC), target, ignore_index=255)


def head_step(cat_q, cat_s, mfeat, prior, target, sd, S, dtype, draws=None, drop=True, loss_coef=1.0):
    """One forward + backward of the head in ``dtype`` -> (loss, aux_loss, low-resolution logits, inner logits, {key: gradient})."""
    prm = {k: sd[k].detach().cpu().to(dtype).clone().requires_grad_(True) for k in head_keys(sd)}
    to = lambda t: t.detach().cpu().to(dtype)
    low, inner = head_forward(to(cat_q), to(cat_s), mfeat.detach().cpu().float(), to(prior), prm, S, draws, drop)
    target = target.detach().cpu()
    loss = ce(low, target)
    aux = sum(ce(o, target) for o in inner) / len(inner)
    (loss + aux * loss_coef).backward()
    return float(loss.detach()), float(aux.detach()), low.detach(), [o.detach() for o in inner], {k: v.grad for k, v in prm.items()}
