"""Do two commits run the inference engines alike?  Every model family, built with its Wgen seed at the ``*_small`` fixture size
(97 x 97, two episodes; the 5-shot fixtures' 64 x 90 query-mask size), runs ``lowres`` eagerly and then ``lowres_graphed`` /
``lowres_graphed_slots`` twice; per output tensor one JSON line with the sha256 of its bytes.  Timing-based variant picks are
off (``ops.AUTOTUNE = False``), so the lines of two runs are equal exactly when the two trees compute the same bits.

  python3 scratch/engine_ab.py > digests.txt                                                    # the digests
  rocprofv3 --kernel-trace --output-format csv -d <dir> -- python3 scratch/engine_ab.py --eager    # the eager launches
  python3 scratch/engine_ab.py --list <dir>/.../*_kernel_trace.csv > launches.txt                  # the ordered list

Two commits launch alike when their lists are equal (profiles/r12_engine_refactor_ab.txt).  Only the models' public API is
used, and every seed and shape is spelled out here: the script has to run unchanged on the commit it is compared against."""
import csv
import hashlib
import json
import os
import sys
import textwrap

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

H = 97
SEEDS = (11, 12)


GLUE = ("at::", "__amd_", "pack_split3_kernel")       # tensor glue of torch and the runtime, weight packing at engine build


def compact(launches):
    """launches: (name tag, short name, grid, workgroup, LDS bytes) in start order -> lines.  Consecutive launches of one kernel
    with one workgroup and LDS size share a line that lists their grids in order (``g x N``: N times in a row); a run of glue
    launches (GLUE) is one line with its length and a sha256 over its members' (tag, grid, workgroup, LDS)."""
    out, i = [], 0
    while i < len(launches):
        tag, short, _, wg, lds = launches[i]
        j = i
        if short.startswith(GLUE):
            while j < len(launches) and launches[j][1].startswith(GLUE):
                j += 1
            digest = hashlib.sha256(repr([(t, g, w, l) for t, _, g, w, l in launches[i:j]]).encode()).hexdigest()[:16]
            out.append(f"{i:5d} {j - i} glue launches {digest}")
        else:
            while j < len(launches) and (launches[j][0], launches[j][3], launches[j][4]) == (tag, wg, lds):
                j += 1
            grids, k = [], i
            while k < j:
                m = k
                while m < j and launches[m][2] == launches[k][2]:
                    m += 1
                grids.append(launches[k][2] + (f" x {m - k}" if m - k > 1 else ""))
                k = m
            head = f"{i:5d} {tag} {short:<40} wg {wg:>4} lds {lds:>6}  grids "
            out += textwrap.wrap(", ".join(grids), 150, initial_indent=head, subsequent_indent=" " * 12)
        i = j
    return out + [f"{len(launches)} launches"]


def listing(path):
    """Kernel, grid, workgroup and LDS size of EVERY launch in start order, in ``compact`` form."""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    launches = []
    for r in rows:
        name = r["Kernel_Name"].replace("void pemp::", "").replace("pemp::", "")
        tag = hashlib.sha256(name.encode()).hexdigest()[:8]            # the full name (template arguments included), shortened
        short = name.replace("(anonymous namespace)::", "").removeprefix("void ").split("(")[0][:40]
        launches.append((tag, short, r.get("Grid_Size", r.get("Grid_Size_X", "")),
                         r.get("Workgroup_Size", r.get("Workgroup_Size_X", "")), r.get("LDS_Block_Size", "")))
    print("\n".join(compact(launches)))


def main(eager_only):
    import torch
    from pemp_amd import ops, synth
    ops.AUTOTUNE = False
    dev = torch.device("cuda:0")

    def model(module, seed, *args, **kw):
        net = getattr(module, "ModelClass")(*args, **kw)
        net.load_state_dict(synth.wgen_state_dict_for(net, seed))
        return net.to(dev).eval()

    def batch(shot, out_hw=(H, H)):
        b = synth.make_batch(list(SEEDS), shot=shot, height=H, width=H, out_hw=out_hw)
        ins = [torch.from_numpy(b[k]).to(dev) for k in ("sup_img", "sup_mask", "qry_img")]
        prior = torch.from_numpy(b["qry_mask"] == 1).float().view(len(SEEDS), 1, *out_hw).to(dev)
        return ins, prior

    def emit(family, call, outs):
        torch.cuda.synchronize()
        outs = [o for o in (outs if isinstance(outs, (tuple, list)) else [outs]) if o is not None]
        for i, o in enumerate(outs):
            raw = o.detach().contiguous().cpu().numpy().tobytes()
            print(json.dumps({"family": family, "call": call, "out": i, "shape": list(o.shape), "dtype": str(o.dtype),
                              "sha256": hashlib.sha256(raw).hexdigest()}), flush=True)

    def run(family, net, args):
        with torch.no_grad():
            emit(family, "eager", net.lowres(*args))
            if not eager_only:
                for k in (1, 2):
                    emit(family, f"graphed{k}", net.lowres_graphed(*args))

    from pemp_amd.networks import baseline, canet, pemp_stage1, pemp_stage2, pfenet, rpmms
    ins1, prior1 = batch(1)
    run("stage1_rn50", model(pemp_stage1, 1234, None, backbone="resnet50"), ins1)
    run("stage1_vgg16", model(pemp_stage1, 1234, None, backbone="vgg16"), ins1)
    run("stage2_rn50cm", model(pemp_stage2, 4321, 1, 1, None), ins1 + [prior1])
    run("stage2_vgg16cm", model(pemp_stage2, 4321, 1, 1, None, backbone2="vgg16"), ins1 + [prior1])
    run("baseline_rn50", model(baseline, 1234, None, backbone="resnet50"), ins1)

    h, w = canet.CaNet.feature_hw(H, H)
    gen = torch.Generator().manual_seed(9)
    hist = torch.rand((len(SEEDS), 1, 2, h, w), generator=gen).to(dev)
    net = model(canet, 1259, None, init_channels=3, drop_rate=0.5, history=True, freeze_backbone=True)
    run("canet_history", net, ins1 + [hist])
    run("canet_zero_history", net, ins1)
    # the slot form: a 3-row table, read and written in place; the second graphed call names other rows than the captured one
    init = torch.rand((3, 2, h, w), generator=gen).to(dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    steps = [(i32([2, -1]), i32([0, 1])), (i32([2, -1]), i32([0, 1])), (i32([0, 1]), i32([1, 2]))]
    table = init.clone()
    with torch.no_grad():
        for k, (call, (rs, ws)) in enumerate(zip(("eager", "graphed1", "graphed2"), steps)):
            if k > 0 and eager_only:
                break
            if k < 2:
                table.copy_(init)
            fn = net.lowres_slots if k == 0 else net.lowres_graphed_slots
            emit("canet_slots", call, [fn(*ins1, table, rs, ws), table])
    run("canet_no_history", model(canet, 1259, None, init_channels=3, drop_rate=0.5, history=False, freeze_backbone=True), ins1)

    run("pfenet_1shot", model(pfenet, 1259, 1, None), ins1)
    run("pfenet_5shot", model(pfenet, 1259, 5, None), batch(5, (64, 90))[0])

    net = model(rpmms, 1259, None)
    net.resample_pmm_init(torch.Generator().manual_seed(7))
    net.set_pmm_init({k: net.pmm_mu0[j0:j0 + k].t() for j0, k in ((0, 1), (1, 3), (4, 6))})         # one init for every call
    run("rpmms", net, ins1)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--list":
        listing(sys.argv[2])
    else:
        main("--eager" in sys.argv[1:])
