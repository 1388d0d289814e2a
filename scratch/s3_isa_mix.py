"""Instruction mix of the split3 conv kernels' steady-state K loop (CPU only; conv_dma2.hip, S3 = the last template flag).

    python3 scratch/s3_isa_mix.py [conv_dma2.s | conv_dma2.hip] [--padv] [--sk]

Without an argument it compiles pemp_amd/csrc/conv_dma2.hip with the build's flags plus ``--cuda-device-only -S`` (and
``-Rpass-analysis=kernel-resource-usage`` for the register / scratch figures).  For each unsplit S3 tile id it finds the kernel
(plain, or with --padv / --sk the padding-value / split-K instantiation), takes the K loop's basic block (the block that branches
back to its own label and holds the most MFMAs), and prints per K step (32 channels) and per wave: MFMAs, VALU (of which
v_cvt_pk_bf16_f32), SALU, LDS reads, VALU per MFMA, and VGPR + AGPR / scratch / occupancy of the kernel."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# tile id -> (BM, BN, NW); the wave grid (WGM) is read from the kernel's name.  47 / 49: the persistent forms of 43 / 46
# (conv_dma2_s3p_kernel: no split-K instantiation)
TILES = {43: (64, 64, 4), 42: (128, 64, 4), 41: (128, 128, 4), 44: (128, 128, 8), 46: (256, 128, 8), 47: (64, 64, 4), 49: (256, 128, 8)}
PERSISTENT = (47, 49)
NAME = re.compile(r"^(_ZN4pemp16conv_dma2_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELi0ELb([01])ELb0ELb0ELb0ELb1EEEvNS_8ConvArgsE):")
NAME_P = re.compile(r"^(_ZN4pemp20conv_dma2_s3p_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])()EEEvNS_8ConvArgsE):")
NOT_SALU = ("s_waitcnt", "s_barrier", "s_nop", "s_cbranch", "s_branch", "s_setprio", "s_endpgm", "s_sleep")


def compile_asm(src):
    from pemp_amd import build
    out = tempfile.mkdtemp()
    asm = os.path.join(out, "conv_dma2.s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc] + build.FLAGS + ["--cuda-device-only", "-S", src, "-o", asm, "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, check=True)
    return asm, r.stderr


def resources(remarks):
    """kernel name -> {field: value} from the kernel-resource-usage remarks"""
    res, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark: +Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: +([^:]+?): (\d+) \[", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return res


def kernels(asm):
    """kernel name -> list of (label, [instructions]) basic blocks"""
    out, cur, blocks = {}, None, None
    with open(asm) as f:
        for line in f:
            m = NAME.match(line) or NAME_P.match(line)
            if m:
                cur = m.group(1)
                blocks = out[cur] = [("entry", [])]
                continue
            if cur is None:
                continue
            if line.startswith(".Lfunc_end"):
                cur = None
                continue
            s = line.strip()
            if re.match(r"^\.LBB\d+_\d+:", s):
                blocks.append((s[:-1].split(":")[0], []))
            elif s and not s.startswith((";", ".")):
                blocks[-1][1].append(s.split(";")[0].strip())
    return out


def mix(insts):
    ops = [i.split()[0] for i in insts if i]
    c = dict(mfma=sum(o.startswith("v_mfma") for o in ops),
             valu=sum(o.startswith("v_") and not o.startswith("v_mfma") for o in ops),
             cvt=sum(o == "v_cvt_pk_bf16_f32" for o in ops),
             salu=sum(o.startswith("s_") and not o.startswith(NOT_SALU) for o in ops),
             ds_read=sum(o.startswith("ds_read") for o in ops),
             vmem=sum(o.startswith(("buffer_", "global_")) for o in ops))
    return c


def kloop(blocks):
    best = None
    for label, insts in blocks:
        if not any(re.search(r"s_cbranch_\w+ " + re.escape(label) + r"$", i) for i in insts):
            continue
        c = mix(insts)
        if best is None or c["mfma"] > best["mfma"]:
            best = c
    return best


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    padv, sk = "--padv" in sys.argv, "--sk" in sys.argv
    src = args[0] if args else os.path.join(ROOT, "pemp_amd", "csrc", "conv_dma2.hip")
    remarks = ""
    if src.endswith(".hip"):
        asm, remarks = compile_asm(src)
    else:
        asm = src
    ks, res = kernels(asm), resources(remarks)
    print(f"{'id':>3} {'block / waves':>14} {'wave tile':>9} {'MFMA':>5} {'VALU':>5} {'cvt':>4} {'SALU':>5} {'ds_read':>7} {'VALU/MFMA':>9}"
          f" {'VGPR+AGPR':>9} {'scratch':>7} {'occ':>4}")
    for tid, (bm, bn, nw) in TILES.items():
        for name, blocks in ks.items():
            m = (NAME_P if tid in PERSISTENT else NAME).match(name + ":")
            if not m or (int(m.group(2)), int(m.group(3)), int(m.group(5))) != (bm, bn, nw) or m.group(6) != str(int(padv)):
                continue
            if tid in PERSISTENT and sk:
                continue
            if tid not in PERSISTENT and m.group(7) != str(int(sk)):
                continue
            wgm = int(m.group(4))
            wm, wn = bm // wgm, bn // (nw // wgm)
            c = kloop(blocks)
            steps = c["mfma"] // (6 * (wm // 32) * (wn // 32) * 2) if c else 0
            r = res.get(name, {})
            regs = (r.get("VGPRs", 0) + r.get("AGPRs", 0)) if r else "-"
            if not c or not steps:
                print(f"{tid:>3} no K loop found in {name}")
                continue
            per = {k: v / steps for k, v in c.items()}
            print(f"{tid:>3} {f'{bm}x{bn} / {nw}':>14} {f'{wm}x{wn}':>9} {per['mfma']:>5.0f} {per['valu']:>5.0f} {per['cvt']:>4.0f} {per['salu']:>5.0f}"
                  f" {per['ds_read']:>7.0f} {per['valu'] / per['mfma']:>9.2f} {regs:>9} {r.get('ScratchSize [bytes/lane]', '-'):>7}"
                  f" {r.get('Occupancy [waves/SIMD]', '-'):>4}")


if __name__ == "__main__":
    main()
