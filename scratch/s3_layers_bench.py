"""The heavy layers of the 25-episode eval step (M = 130 050 rows: 50 maps of 51 x 51) alone on the chip, per split3 tile id: us,
TFLOP/s, bit-identity of every unsplit id with id 43, and a hash of every output (ids 51..56 included) so that two builds can be
compared.  GPU.

    python3 scratch/s3_layers_bench.py [--only 256-256-k3] [--reps N]

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
# (cin, cout, k, dil, residual, padding value[, stride, maps of HW x HW]): the six geometries that carry ~81 % of the step's conv time, and the 3 x 3 layer
# once more with a padding value (the PADV instantiation)
LAYERS = ((256, 1024, 1, 1, True, False), (512, 1024, 1, 1, False, False), (1024, 256, 1, 1, False, False),
          (256, 256, 3, 2, False, False), (128, 512, 1, 1, True, False), (1024, 512, 1, 1, False, False),
          (256, 256, 3, 2, False, True),
          # the short-K expand convs of layer1 / layer2 at the headline's M (510 050 rows: 50 maps of 101 x 101), the stride-2 downsample
          (64, 256, 1, 1, True, False, 1, 101), (64, 256, 1, 1, False, False, 1, 101), (256, 512, 1, 1, False, False, 2, 101))


def timed(fn, reps, n=5):
    for _ in range(2):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e9
    for _ in range(reps):
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) / n * 1e3)
    return best


def digest(t):
    return hashlib.sha1(t.cpu().numpy().tobytes()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="", help="cin-cout-kK[-padv]: one layer")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N = 50
    for layer in LAYERS:
        cin, cout, k, dil, has_res, padv = layer[:6]
        stride, HW = layer[6:] if len(layer) > 6 else (1, 51)
        M = N * HW * HW
        HO = (HW - 1) // stride + 1 if k == 1 else HW
        name = f"{cin}-{cout}-k{k}" + ("-padv" if padv else "") + (f"-s{stride}" if stride > 1 else "") + (f"-hw{HW}-res{int(has_res)}" if HW != 51 else "")
        if args.only and args.only != name:
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
        for tile in UNSPLIT + panel + SPLIT:
            if cout % ops._tile_bn(tile):
                continue
            run = lambda: ops.conv2d(x, prm, residual=res, pad_value=pad_value, out=out, tile=tile)
            run()
            same = torch.equal(out, ref)
            if tile in SPLIT:
                hashes.append(f"{tile}=" + ("43" if same else digest(out)))
            us = timed(run, args.reps)
            mark = "" if same else (" ~" if tile in SPLIT else " !")
            cells.append(f"{tile}: {us:7.1f}us {fl / us / 1e6:5.1f}TF{mark}")
            if tile not in SPLIT and not same:
                hashes.append(f"{tile}=MISMATCH:{digest(out)}")
        print(f"{name:>16} k{k} d{dil} res{int(has_res)} | " + " | ".join(cells), flush=True)
        print(f"{'':>16} hash " + " ".join(hashes), flush=True)
    print("(! = an unsplit id differs from id 43; ~ = a split-K id differs from id 43, expected where it splits)")


if __name__ == "__main__":
    main()
