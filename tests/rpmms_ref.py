"""Functional torch restatement of RPMMs' head in train() mode (reference networks/rpmms.py:213-311), from the two
``cat((f2, f3))`` feature groups (supports, queries) to the three losses, differentiated by autograd -- test infrastructure.
Pinned by the reference-made fixtures of tests/golden/make_golden_rpmms_train.py (tests/test_rpmms_train_cpu.py holds it to
their float64 gradients), not trusted on its own; the GPU tests then use it on the engine's own trunk features.

It restates the four points a port gets wrong (RPMMs head training): the EM and the probability maps run
under ``no_grad``; the history is the softmax of the pass before WITH its gradient (``cut_history=True`` detaches it: the GPU
tests use that to show they can see the difference); ``layer55.2`` draws once per prototype, the other Dropout2d modules once
per pass; ``layer5``'s BatchNorm normalises the supports and the queries as two batches.

NHWC features, Dropout2d draws [calls, B, 256] per reference module name -- keep where u < 1 - p."""
import torch
import torch.nn.functional as F

KS = (1, 3, 6)
DROP_CALLS = {"layer55.2": 10, "layer56.2": 3, "layer7.2": 3, **{f"layer6.aspp_{i}.2": 3 for i in range(5)}}
#: the head tensors, in ``model.parameters()`` order
HEAD = tuple(f"{m}.{k}" for m in ("layer5.0", "layer5.1", "layer55.0", "layer56.0", "layer6.aspp_0.0", "layer6.aspp_1.0",
                                  "layer6.aspp_2.0", "layer6.aspp_3.0", "layer6.aspp_4.0", "layer7.0", "layer9", "residule1.1",
                                  "residule1.3", "residule2.1", "residule2.3", "residule3.1", "residule3.3") for k in ("weight", "bias"))
#: layer5's conv bias sits in front of a batch-statistics BatchNorm: its gradient is zero up to rounding
ZERO_GRAD = ("layer5.0.bias",)


def trunk_cat23(sd, images, dtype=torch.float64):
    """ONE ``model_res`` call in train() mode on one group of images [n,3,H,W] by the oracle's ResNet restatement -> cat((f2,
    f3)) NHWC [n,h,w,1536].  ``sd`` is not changed (the running statistics move in a copy)."""
    from oracle import ref_cpu
    sd = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items() if k.startswith("model_res.")}
    saved, ref_cpu.TRAIN = ref_cpu.TRAIN, True
    try:
        with torch.no_grad():
            x = ref_cpu.resnet_stem(images.to(dtype), sd, "model_res")
            f1 = ref_cpu._res_layer(x, sd, "model_res", "layer1", 3)
            f2 = ref_cpu._res_layer(f1, sd, "model_res", "layer2", 4)
            f3 = ref_cpu._res_layer(f2, sd, "model_res", "layer3", 6)
    finally:
        ref_cpu.TRAIN = saved
    return torch.cat((f2, f3), dim=1).permute(0, 2, 3, 1).contiguous()


def em(x, mu0, iters=10, kappa=20.0):
    """PMMs.EM (rpmms.py:65-86): x [B,C,N], mu0 [C,K] -> mu [B,K,C]."""
    l2 = lambda t: t / (1e-6 + t.norm(dim=1, keepdim=True))
    mu = mu0.to(x.dtype)[None].repeat(x.shape[0], 1, 1)
    for _ in range(iters):
        z = F.softmax(kappa * torch.bmm(x.permute(0, 2, 1), mu), dim=2)
        mu = l2(torch.bmm(x, z / (1e-6 + z.sum(dim=1, keepdim=True))))
    return mu.permute(0, 2, 1)


def head_logits(cat_s, cat_q, sup_mask, prm, mu0, draws=None, p=0.0, cut_history=False):
    """cat_s / cat_q NHWC [B,h,w,1536]; sup_mask [B,1,2,H,W]; ``prm``: {reference key: tensor} of the head; ``mu0``: {K: [256,K]}
    -> ([out0, out1, out2] low-resolution logits, {K: (mu_f, mu_b)})."""
    dt = cat_q.dtype
    B = cat_q.shape[0]

    def drop(x, name, call):
        return x if p == 0.0 else x * ((draws[name][call] < 1 - p).to(dt) / (1 - p))[:, :, None, None]

    def conv(x, name, dil=1, k=3):
        return F.conv2d(x, prm[name + ".weight"], prm[name + ".bias"], 1, dil if k == 3 else 0, dil)

    def layer5(c):
        z = conv(c.permute(0, 3, 1, 2), "layer5.0", 2)
        return F.relu(F.batch_norm(z, None, None, prm["layer5.1.weight"], prm["layer5.1.bias"], True, 0.1, 1e-5))

    fs, fq = layer5(cat_s), layer5(cat_q)
    h, w = fq.shape[-2:]
    H, W = sup_mask.shape[-2:]
    protos, probs = {}, {}
    with torch.no_grad():
        m = F.interpolate(sup_mask.reshape(B, 2, H, W)[:, :1].to(dt), (h, w), mode="bilinear", align_corners=True)
        for K in KS:
            mu_f, mu_b = em((m * fs).flatten(2), mu0[K]), em(((1 - m) * fs).flatten(2), mu0[K])
            P = F.softmax(torch.bmm(fq.flatten(2).permute(0, 2, 1), torch.cat((mu_f, mu_b), dim=1).permute(0, 2, 1)), dim=2)
            P = P.permute(0, 2, 1).reshape(B, 2 * K, h, w)
            protos[K], probs[K] = (mu_f, mu_b), torch.cat((P[:, K:].sum(1, keepdim=True), P[:, :K].sum(1, keepdim=True)), dim=1)
    hist, outs, col = torch.zeros((B, 2, h, w), dtype=dt), [], 0
    for ps, K in enumerate(KS):
        acc = None
        for i in range(K):
            vec = protos[K][0][:, i][:, :, None, None].expand(-1, -1, h, w)
            y = drop(F.relu(conv(torch.cat((fq, vec), dim=1), "layer55.0", 2)), "layer55.2", col)
            acc, col = (y if acc is None else acc + y), col + 1
        out = drop(F.relu(conv(torch.cat((acc, probs[K]), dim=1), "layer56.0")), "layer56.2", ps)
        out = out + conv(F.relu(conv(F.relu(torch.cat((out, hist), dim=1)), "residule1.1")), "residule1.3")
        out = out + conv(F.relu(conv(F.relu(out), "residule2.1")), "residule2.3")
        out = out + conv(F.relu(conv(F.relu(out), "residule3.1")), "residule3.3")
        g = drop(F.relu(conv(F.adaptive_avg_pool2d(out, (1, 1)), "layer6.aspp_0.0", k=1)), "layer6.aspp_0.2", ps).expand(-1, -1, h, w)
        br = [g, drop(F.relu(conv(out, "layer6.aspp_1.0", k=1)), "layer6.aspp_1.2", ps)]
        br += [drop(F.relu(conv(out, f"layer6.aspp_{i}.0", d)), f"layer6.aspp_{i}.2", ps) for i, d in ((2, 6), (3, 12), (4, 18))]
        out = drop(F.relu(conv(torch.cat(br, dim=1), "layer7.0", k=1)), "layer7.2", ps)
        out = conv(out, "layer9", k=1)
        outs.append(out)
        hist = F.softmax(out.detach() if cut_history else out, dim=1)
    return outs, protos


def losses_of(outs, target):
    """get_loss (rpmms.py:289-311): bilinear (align_corners) upsample + mean CE without an ignore index per pass -> (sum, CE of
    out2, CE of out1)."""
    ce = [F.cross_entropy(F.interpolate(o, tuple(target.shape[-2:]), mode="bilinear", align_corners=True), target) for o in outs]
    return ce[0] + ce[1] + ce[2], ce[2], ce[1]


def head_step(cat_s, cat_q, sup_mask, target, sd, mu0, dtype, draws=None, p=0.0, cut_history=False):
    """One forward + backward of the head in ``dtype`` -> (the three losses as floats, the three low-resolution logits,
    {key: gradient} of the head, {K: (mu_f, mu_b)})."""
    prm = {k: sd[k].detach().to(dtype).clone().requires_grad_(True) for k in HEAD}
    dr = None if draws is None else {k: v.detach().cpu() for k, v in draws.items()}
    outs, protos = head_logits(cat_s.detach().to(dtype), cat_q.detach().to(dtype), sup_mask, prm, mu0, dr, p, cut_history)
    ls = losses_of(outs, target)
    grads = torch.autograd.grad(ls[0], [prm[k] for k in HEAD])
    return [float(v.detach()) for v in ls], [o.detach() for o in outs], dict(zip(HEAD, grads)), protos


# -- the fixtures of tests/golden/make_golden_rpmms_train.py -------------------------------------------------------------------
def fixture_state_dict():
    """The fixtures' weights: wgen seed 1259 over the key layout of the model."""
    from tests import util
    return util.wgen_state_dict("rpmms", seed=1259)


def fixture_inputs(name):
    """The fixture's episode batch, initial mu and draws on the CPU -> (g, sup, msk, qry, gt, mu0 {K: [256,K]}, draws)."""
    from pemp_amd import synth
    from tests import util
    g = util.gold(name)
    seeds, H = [int(s) for s in g["seeds"]], int(g["H"])
    b = synth.make_batch(seeds, shot=1, height=H, width=H, out_hw=(H, H))
    sup, msk, qry = (torch.from_numpy(b[k]) for k in ("sup_img", "sup_mask", "qry_img"))
    gt = torch.from_numpy(b["qry_mask"]).reshape(-1, H, H)
    mu0 = {K: torch.from_numpy(g[f"mu0_k{K}"]) for K in KS}
    draws = {k: torch.from_numpy(g["draws__" + k]) for k in DROP_CALLS} if "draws__layer55.2" in g.files else None
    return g, sup, msk, qry, gt, mu0, draws
