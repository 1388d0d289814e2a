"""The heavy layers of the 25-episode eval step (M = 130 050 rows: 50 maps of 51 x 51) alone on the chip, per split3 tile id: us,
TFLOP/s, bit-identity of every unsplit id with id 43, and a hash of every output (ids 51..56 included) so that two builds can be
compared.  The multi-tap layers also run the ids that read PRE-SPLIT activations (146 / 149, and 246 / 249 where they apply, the input
split on the device by the reference arithmetic) -- without a residual also with the second, pre-split output ("149+s" = id 149 with also_split3: the fp32 tensor
must be id 43's and the second one its split) -- and the 1x1 layers without a residual also run as producers of a pre-split output
("43s" = id 43 with out_split3, "49s" / "349s" = the persistent ids' producer kernels; the result must be the split of id 43's).  Every cell carries the fastest and the slowest of its --reps timings.  GPU.

    python3 scratch/s3_layers_bench.py [--only 256-256-k3[,...]] [--ids 49,149] [--reps N] [--res 0|1]

Inputs come from a seeded CPU generator: the hashes are functions of the kernels alone."""
import argparse
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pemp_amd import ops  # noqa: E402

UNSPLIT = (43, 42, 41, 44, 46, 47, 49)     # 47 / 49: persistent forms of 43 / 46
SPLIT = (52, 51, 54, 56)
PANEL = ops.SPLIT3_PANEL_TILES             # 71 / 72: activation-stationary forms (1x1, Kpad <= 256; conv_panel.hip)
PRESPLIT = ops.SPLIT3_PRESPLIT_TILES       # 146 / 149: the forms of 46 / 49 on pre-split activations
RING = getattr(ops, "SPLIT3_RING_TILES", ())     # 349: the form of 49 on a three-deep activation ring (1x1, pad 0, K >= 128, no residual; conv_ring.hip); () on a tree without it
ROW3 = ops.SPLIT3_ROW3_TILES               # 246 / 249: 146 / 149 with one activation stage per (chunk, kh) (3x3, pad == dil, no residual / padding value; conv_row3.hip)
# (cin, cout, k, dil, residual, padding value[, stride, maps of HW x HW]): the six geometries that carry ~81 % of the step's conv time, and the 3 x 3 layer
# once more with a padding value (the PADV instantiation)
LAYERS = ((256, 1024, 1, 1, True, False), (512, 1024, 1, 1, False, False), (1024, 256, 1, 1, False, False),
          (256, 256, 3, 2, False, False), (128, 512, 1, 1, True, False), (1024, 512, 1, 1, False, False),
          (256, 256, 3, 2, False, True),
          # the short-K expand convs of layer1 / layer2 at the headline's M (510 050 rows: 50 maps of 101 x 101), the stride-2 downsample
          (64, 256, 1, 1, True, False, 1, 101), (64, 256, 1, 1, False, False, 1, 101), (256, 512, 1, 1, False, False, 2, 101),
          # the other 3x3 widths (layer2: stride 1 at 51 x 51 and stride 2 from 101 x 101; layer1 at 101 x 101) and layer2's conv1
          (128, 128, 3, 1, False, False), (128, 128, 3, 1, False, False, 2, 101), (64, 64, 3, 1, False, False, 1, 101),
          (512, 128, 1, 1, False, False),
          # layer3 block 0 conv1 and a 256 -> 256 1x1 (the 1x1 ASPP branch)
          (512, 256, 1, 1, False, False), (256, 256, 1, 1, False, False),
          # layer1's last conv3 with row pruning: M = 130 050 compact rows, the residual on the 101 x 101 grid (residual_stride=2; a 9th
          # field: the residual's grid).  Against the dense-residual row 64-256-k1-hw101-res1 at M = 510 050
          (64, 256, 1, 1, True, False, 1, 51, 101),
          # ... and its conv2 at stride 2 (against 64-64-k3-hw101-res0)
          (64, 64, 3, 1, False, False, 2, 101),
          # a dilated ASPP branch (dilation 12) with its padding vector
          (256, 256, 3, 12, False, True))


def timed(fn, reps, n=5):
    for _ in range(2):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best, worst = 1e9, 0.0
    for _ in range(reps):
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        us = e0.elapsed_time(e1) / n * 1e3
        best, worst = min(best, us), max(worst, us)
    return best, worst


def presplit(x):
    """fp32 [..., C] -> bf16 [..., C / 32, 3, 32]: the planes h, m, l of pemp_pack_split3_bf16's arithmetic."""
    h = x.to(torch.bfloat16)
    r = x - h.float()
    m = r.to(torch.bfloat16)
    lo = (r - m.float()).to(torch.bfloat16)
    return torch.stack([p.reshape(*x.shape[:-1], x.shape[-1] // 32, 32) for p in (h, m, lo)], dim=-2).contiguous()


def digest(t):
    return hashlib.sha1(t.cpu().numpy().tobytes()).hexdigest()[:16]


def rs2_row(dev, N, HW, HR, cin, cout, name, keep, reps):
    """A 1x1 conv on N compact maps of HW x HW with the residual on the HR x HR grid (ops.conv2d residual_stride=2), every id that takes
    it; ! = differs from id 43 on the gathered dense residual."""
    g = torch.Generator().manual_seed(cin * 7 + cout * 3 + 1001)
    x = torch.randn(N * HW * HW, cin, generator=g).to(dev).view(N, HW, HW, cin)
    w = (torch.randn(cout, cin, 1, 1, generator=g) * (1.0 / cin ** 0.5)).to(dev)
    packed, kpad = ops.pack_conv_weight(w)
    packed = packed.contiguous()
    prm = ops.ConvParams(packed, None, torch.randn(cout, generator=g).to(dev), cin, cout, 1, 1, 1, 0, 1, kpad, False, True, ops.pack_split3(packed))
    res = torch.randn(N, HR, HR, cout, generator=g).to(dev)
    ref = ops.conv2d(x, prm, residual=res[:, ::2, ::2, :].contiguous(), tile=43).clone()
    out = torch.empty_like(ref)
    fl = 2.0 * N * HW * HW * cout * cin
    cells = []
    for tile in keep(ops.res_s2_tiles(prm)):
        run = lambda: ops.conv2d(x, prm, residual=res, residual_stride=2, out=out, tile=tile)
        out.zero_()
        run()
        same = torch.equal(out, ref)
        us, worst = timed(run, reps)
        cells.append(f"{tile}: {us:7.1f}..{worst:6.1f}us {fl / us / 1e6:5.1f}TF{'' if same else ' !'}")
    print(f"{name:>16} k1 d1 res1 | " + " | ".join(cells), flush=True)
    print(f"{'':>16} hash 43={digest(ref)}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="", help="cin-cout-kK[-padv]: one layer")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ids", default="", help="comma-separated tile ids: only these are timed (a counter run of one kernel)")
    ap.add_argument("--producers", action="store_true", help="with --ids: time the selected ids as producers of a pre-split output too")
    ap.add_argument("--res", type=int, choices=(0, 1), default=None, help="run the selected layers without / with a residual, whatever their row says")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N = 50
    keep = lambda ids: tuple(t for t in ids if not args.ids or str(t) in args.ids.split(","))
    for layer in LAYERS:
        cin, cout, k, dil, has_res, padv = layer[:6]
        stride, HW = layer[6:8] if len(layer) > 6 else (1, 51)
        RS2 = layer[8] if len(layer) > 8 else 0          # the strided residual's grid
        has_res = has_res if args.res is None or RS2 else bool(args.res)
        M = N * HW * HW
        HO = (HW - 1) // stride + 1
        name = f"{cin}-{cout}-k{k}" + (f"-d{dil}" if k == 3 and dil > 2 else "") + ("-padv" if padv else "") + (f"-s{stride}" if stride > 1 else "") + (f"-hw{HW}-res{int(has_res)}" if HW != 51 else "") + ("-rs2" if RS2 else "")
        if args.only and name not in args.only.split(","):
            continue
        if RS2:
            rs2_row(dev, N, HW, RS2, cin, cout, name, keep, args.reps)
            continue
        g = torch.Generator().manual_seed(cin * 7 + cout * 3 + k)
        buf = torch.empty(M + 4, cin, device=dev)
        buf[:M] = torch.randn(M, cin, generator=g).to(dev)
        buf[M:] = torch.randn(cin, generator=g).to(dev)
        x, pv = buf[:M].view(N, HW, HW, cin), buf[M]
        w = (torch.randn(cout, cin, k, k, generator=g) * (1.0 / (cin * k * k) ** 0.5)).to(dev)
        packed, kpad = ops.pack_conv_weight(w)
        packed = packed.contiguous()
        prm = ops.ConvParams(packed, None, torch.randn(cout, generator=g).to(dev), cin, cout, k, k, stride, dil if k == 3 else 0, dil, kpad,
                             False, True, ops.pack_split3(packed))
        res = torch.randn(N, HO, HO, cout, generator=g).to(dev) if has_res else None
        pad_value = pv if padv else None
        out = torch.empty(N, HO, HO, cout, device=dev)
        fl = 2.0 * N * HO * HO * cout * k * k * cin
        ref = ops.conv2d(x, prm, residual=res, pad_value=pad_value, tile=43).clone()
        cells, hashes = [], [f"43={digest(ref)}"]
        panel = PANEL if k == 1 and kpad <= 256 and not padv else ()
        ring = RING if k == 1 and kpad >= 128 and not has_res and not padv and cout % 128 == 0 else ()
        for tile in keep(UNSPLIT + ring + panel + SPLIT):
            if cout % ops._tile_bn(tile):
                continue
            run = lambda: ops.conv2d(x, prm, residual=res, pad_value=pad_value, out=out, tile=tile)
            run()
            same = torch.equal(out, ref)
            if tile in SPLIT:
                hashes.append(f"{tile}=" + ("43" if same else digest(out)))
            us, worst = timed(run, args.reps)
            mark = "" if same else (" ~" if tile in SPLIT else " !")
            cells.append(f"{tile}: {us:7.1f}..{worst:6.1f}us {fl / us / 1e6:5.1f}TF{mark}")
            if tile not in SPLIT and not same:
                hashes.append(f"{tile}=MISMATCH:{digest(out)}")
        if k > 1 and cout % 128 == 0:            # the same layer on pre-split activations
            sbuf = torch.zeros((M + 4) * cin * 3, dtype=torch.bfloat16, device=dev)
            sbuf[:(M + 1) * cin * 3] = presplit(buf[:M + 1]).reshape(-1)
            xs, pvs = sbuf[:M * cin * 3].view(N, HW, HW, cin // 32, 3, 32), sbuf[M * cin * 3:(M + 1) * cin * 3].view(cin // 32, 3, 32)
            row3 = ROW3 if k == 3 and stride == 1 and not has_res and not padv and ops.row3_stage_rows(HW, dil) <= ops.ROW3_STAGE_ROWS else ()
            for tile in keep(PRESPLIT + row3):
                run = lambda: ops.conv2d(xs, prm, residual=res, pad_value=pvs if padv else None, out=out, tile=tile, x_split3=True)
                out.zero_()
                run()
                same = torch.equal(out, ref)
                us, worst = timed(run, args.reps)
                cells.append(f"{tile}: {us:7.1f}..{worst:6.1f}us {fl / us / 1e6:5.1f}TF{'' if same else ' !'}")
            if not has_res:                      # ... writing its output twice: fp32 and pre-split (p3, whose readers take both forms)
                want = presplit(ref)
                outs = torch.empty_like(want)
                for tile in keep(PRESPLIT):
                    run = lambda: ops.conv2d(xs, prm, pad_value=pvs if padv else None, out=out, tile=tile, x_split3=True, also_split3=outs)
                    out.zero_()
                    run()
                    same = torch.equal(out, ref) and torch.equal(outs.view(torch.int16), want.view(torch.int16))
                    us, worst = timed(run, args.reps)
                    cells.append(f"{tile}+s: {us:7.1f}..{worst:6.1f}us{'' if same else ' !'}")
                del want, outs
            del sbuf, xs, pvs
        if k == 1 and not has_res:               # the same layer as the producer of a pre-split output
            want = presplit(ref)
            outs = torch.empty_like(want)
            for tile in keep((43, 42, 41, 44, 46, 47, 49) + ring if not args.ids or args.producers else ()):
                if cout % ops._tile_bn(tile):
                    continue
                run = lambda: ops.conv2d(x, prm, out=outs, tile=tile, out_split3=True)
                run()
                same = torch.equal(outs.view(torch.int16), want.view(torch.int16))
                us, worst = timed(run, args.reps)
                cells.append(f"{tile}s: {us:7.1f}..{worst:6.1f}us{'' if same else ' !'}")
            del want, outs
        print(f"{name:>16} k{k} d{dil} res{int(has_res)} | " + " | ".join(cells), flush=True)
        print(f"{'':>16} hash " + " ".join(hashes), flush=True)
    print("(146 / 149 / 246 / 249: on the pre-split input; NNs: id NN writing a pre-split output, ! = not the split of id 43's;")
    print(" NNN+s: id NNN writing fp32 and the pre-split copy, ! = either differs)")
    print("(! = an unsplit id differs from id 43; ~ = a split-K id differs from id 43, expected where it splits)")


if __name__ == "__main__":
    main()
