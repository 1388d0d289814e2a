"""Which kernel does every (conv entry point, tile id) pair launch?  Variants inside a family are bit-identical, so an id wired to
the wrong shape passes every output test and only costs speed: this launches each pair ONCE with an explicit ``tile=`` on a tiny
problem, so that a kernel trace of the run lists, in a fixed order, the kernel, grid, workgroup and LDS size behind every id.

  rocprofv3 --kernel-trace --output-format csv -d <dir> -- python3 scratch/conv_dispatch_trace.py       # the launches
  python3 scratch/conv_dispatch_trace.py --list <dir>/.../*_kernel_trace.csv > launches.txt              # the ordered list

Two commits dispatch alike when their lists are equal (profiles/r10_conv_dispatch_trace.txt).  The id lists are spelled out here,
not read from pemp_amd.ops: the script has to run unchanged on the commit it is compared against."""
import csv
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

FP32 = (1, 2, 3, 11, 12, 13, 14, 15, 16, 17, 21, 22, 23, 24, 25, 26, 27, 28, 29)
SPLITK = (31, 32, 34, 35, 36, 37)
SPLIT3 = (41, 42, 43, 44, 46, 47, 49)
SPLIT3_SPLITK = (51, 52, 54, 56)
DMA2 = (21, 22, 23, 24, 25, 26, 27)


def listing(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    conv = [r for r in rows if any(k in r["Kernel_Name"] for k in ("conv_dma", "conv_igemm", "conv_stem_pool"))]
    for i, r in enumerate(conv):
        name = r["Kernel_Name"].split("(")[0].replace("void pemp::", "").replace("pemp::", "")
        g = r.get("Grid_Size", r.get("Grid_Size_X", ""))
        wg = r.get("Workgroup_Size", r.get("Workgroup_Size_X", ""))
        print(f"{i:4d} grid {g:>8} wg {wg:>4} lds {r.get('LDS_Block_Size', ''):>7}  {name}")


def main():
    import torch
    from pemp_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    count = [0]

    def layer(cin, cout, k, dil=1, split3=False):
        packed, kpad = ops.pack_conv_weight(rnd(cout, cin, k, k) * (cin * k * k) ** -0.5)
        return ops.ConvParams(packed, None, None, cin, cout, k, k, 1, dil * (k // 2), dil, kpad, False, True,
                              ops.pack_split3(packed) if split3 else None)

    def run(what, fn, ids):
        for t in ids:
            fn(t)
            count[0] += 1
        torch.cuda.synchronize()
        print(f"{what}: ids {list(ids)}", flush=True)

    # one tiny problem: 2 x 13 x 13 = 338 output rows, Cin 64 -> Cout 256, 3 x 3 (6 tiles of 128 x 128: the split-K ids do split)
    x = rnd(2, 13, 13, 64)
    res = rnd(2, 13, 13, 256)
    pad = torch.cat([x.reshape(-1), rnd(64)])             # a padding vector BEHIND the activations (buffer-addressed kernels)
    xp, pv = pad[:x.numel()].view_as(x), pad[x.numel():]
    p, p3 = layer(64, 256, 3), layer(64, 256, 3, split3=True)
    for tag, kw, xin in (("plain", {}, x), ("residual", {"residual": res}, x), ("padding value", {"pad_value": pv}, xp)):
        run(f"conv2d, {tag}", lambda t: ops.conv2d(xin, p, tile=t, **kw), FP32 + SPLITK)
        run(f"conv2d split3, {tag}", lambda t: ops.conv2d(xin, p3, tile=t, **kw), SPLIT3 + SPLIT3_SPLITK)
    # the smallest geometry the hybrid launch (29) really splits, with 28 and 23 beside it
    xh, ph = rnd(3, 37, 45, 96), layer(96, 256, 1)
    assert ops.hybrid_rows(3, 37, 45, 256) > 0
    run("conv2d, hybrid geometry", lambda t: ops.conv2d(xh, ph, tile=t), (23, 28, 29))
    # grouped launch: two members
    outs = [torch.empty(2, 13, 13, 256, device=dev) for _ in range(2)]
    run("conv2d_group", lambda t: ops.conv2d_group([x, x], [p, p], outs, tile=t), DMA2 + (28,))
    run("conv2d_group split3", lambda t: ops.conv2d_group([x, x], [p3, p3], outs, tile=t), (41, 42, 43, 44, 46))
    run("conv2d_group, padding value", lambda t: ops.conv2d_group([xp, xp], [p, p], outs, pad_values=[pv, pv], tile=t), DMA2 + (28,))
    # statistics / BatchNorm-backward epilogues
    run("conv2d_stats", lambda t: ops.conv2d_stats(x, p, tile=t), DMA2 + SPLITK)
    bn = {"z": rnd(2, 13, 13, 256), "mean": rnd(256), "invstd": rnd(256).abs() + 0.5,
          "mask": torch.full((338, 8), -1, dtype=torch.int32, device=dev)}
    run("conv2d_bnbwd", lambda t: ops.conv2d_bnbwd(x, p, bn, residual=res, tile=t), DMA2 + SPLITK)
    # DropBlock epilogue
    db = (torch.ones(2, 13, 13, device=dev), torch.full((1,), 338, dtype=torch.int32, device=dev))
    run("conv2d, dropblock", lambda t: ops.conv2d(x, p, dropblock=db, tile=t), DMA2 + SPLITK)
    # bf16 operands
    xb = x.to(torch.bfloat16)
    pb = ops.ConvParams(p.w.to(torch.bfloat16), None, None, 64, 256, 3, 3, 1, 1, 1, p.kpad, False, True)
    run("conv2d, bf16", lambda t: ops.conv2d(xb, pb, tile=t), DMA2)
    run("conv2d, bf16 -> fp32", lambda t: ops.conv2d(xb, pb, out=outs[0], tile=t), DMA2)
    # the stem through the pointer-addressed fall-back (2x -> 1x, 28 -> 13, 29 -> 23 -> 13) and the fused stem + max-pool
    xs = rnd(1, 33, 33, 4)
    ws, kpad = ops.pack_conv_weight(rnd(64, 3, 7, 7) * 0.08, stem4=True)
    stem = ops.ConvParams(ws, None, None, 4, 64, 7, 7, 2, 3, 1, kpad, True, True, w3pool=ops.pack_split3(ws.contiguous()))
    run("conv2d, stem", lambda t: ops.conv2d(xs, stem, tile=t), (3, 13, 23, 28, 29, 12, 22))
    run("stem_pool", lambda t: ops.stem_pool(xs, stem), (0,))
    print(f"{count[0]} launching calls")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--list":
        listing(sys.argv[2])
    else:
        main()
