#!/usr/bin/env python3
"""Counts for profiles/stage_chain_code_object.txt from the device assembly of batotp_amd/csrc/batotp_hip.hip
(hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S -o FILE.s csrc/batotp_hip.hip; no GPU needed).

For every sweep kernel: registers, scratch, occupancy, code bytes, instructions, v_cndmask, v_cmp, s_nop, v_min_f64 / v_max_f64, and
the "0/1 round trips": v_cndmask_b32 v, 0, 1, <mask> whose result a v_cmp_ne_u32 .., 0, v reads back within
three instructions -- a lane mask that went through a VGPR on its way to a branch.  --sites prints each round trip with context.

usage: stage_chain_counts.py FILE.s [--sites KERNEL_SUBSTRING] [--context N]"""
import re
import sys

KERNELS = [("k_sweep8_lock<-1>", "_ZN2bk13k_sweep8_lockILin1EEEvNS_9SweepArgsE"),
           ("k_sweep8_lock<0>", "_ZN2bk13k_sweep8_lockILi0EEEvNS_9SweepArgsE"),
           ("k_sweep8<8,-1,1>", "_ZN2bk8k_sweep8ILi8ELin1ELi1EEEvNS_9SweepArgsE"),
           ("k_sweep8<8,0,1>", "_ZN2bk8k_sweep8ILi8ELi0ELi1EEEvNS_9SweepArgsE"),
           ("k_sweep8<8,-1,-1>", "_ZN2bk8k_sweep8ILi8ELin1ELin1EEEvNS_9SweepArgsE"),
           ("k_sweep8<8,0,-1>", "_ZN2bk8k_sweep8ILi8ELi0ELin1EEEvNS_9SweepArgsE"),
           ("k_sweep8<4,-1,1>", "_ZN2bk8k_sweep8ILi4ELin1ELi1EEEvNS_9SweepArgsE"),
           ("k_sweep8<4,0,1>", "_ZN2bk8k_sweep8ILi4ELi0ELi1EEEvNS_9SweepArgsE"),
           ("k_sweep8<4,-1,-1>", "_ZN2bk8k_sweep8ILi4ELin1ELin1EEEvNS_9SweepArgsE"),
           ("k_sweep8<4,0,-1>", "_ZN2bk8k_sweep8ILi4ELi0ELin1EEEvNS_9SweepArgsE")]

INSTR = re.compile(r"^\s+([vs]_[a-z0-9_]+|global_[a-z0-9_]+|ds_[a-z0-9_]+|scratch_[a-z0-9_]+|buffer_[a-z0-9_]+|flat_[a-z0-9_]+)\b(.*)$")
ZERO_ONE = re.compile(r"^\s*(v\d+), 0, 1, (vcc|s\[\d+:\d+\])")


def kernel_body(lines, sym):
    start = next((i for i, l in enumerate(lines) if l.startswith(sym + ":")), None)
    if start is None:
        return None, None
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    meta = {}
    for l in lines[end:end + 80]:
        m = re.match(r";\s*(NumVgprs|ScratchSize|Occupancy|codeLenInByte|NumSgprs)\s*[:=]\s*(\d+)", l.strip())
        if m and m.group(1) not in meta:
            meta[m.group(1)] = int(m.group(2))
    return lines[start:end], meta


def instructions(body):
    out = []
    for l in body:
        m = INSTR.match(l.split(";")[0])
        if m:
            out.append((m.group(1), m.group(2).strip(), l.rstrip()))
    return out


def round_trips(ins):
    sites = []
    for i, (op, args, _) in enumerate(ins):
        if not op.startswith("v_cndmask_b32"):
            continue
        m = ZERO_ONE.match(args)
        if not m:
            continue
        reg = m.group(1)
        for k in range(i + 1, min(i + 4, len(ins))):
            op2, args2, _ = ins[k]
            if op2.startswith("v_cmp_ne_u32") and re.search(r",\s*0,\s*%s\b" % reg, args2):
                sites.append(i)
                break
    return sites


def main():
    path = sys.argv[1]
    want = sys.argv[sys.argv.index("--sites") + 1] if "--sites" in sys.argv else None
    ctx = int(sys.argv[sys.argv.index("--context") + 1]) if "--context" in sys.argv else 8
    lines = open(path).read().split("\n")
    print("kernel               VGPRs scratch occupancy  bytes  instr v_cndmask v_cmp s_nop v_min/max_f64 round-trips")
    for name, sym in KERNELS:
        body, meta = kernel_body(lines, sym)
        if body is None:
            continue
        ins = instructions(body)
        n = lambda p: sum(1 for op, _, _ in ins if op.startswith(p))
        sites = round_trips(ins)
        print(f"{name:20s} {meta.get('NumVgprs', -1):5d} {meta.get('ScratchSize', -1):7d} {meta.get('Occupancy', -1):9d} {meta.get('codeLenInByte', -1):6d} "
              f"{len(ins):6d} {n('v_cndmask'):9d} {n('v_cmp'):5d} {n('s_nop'):5d} {n('v_min_f64') + n('v_max_f64'):13d} {len(sites):11d}")
        if want and want in name:
            for s in sites:
                print(f"--- {name}: instruction {s}")
                for k in range(max(0, s - ctx), min(len(ins), s + ctx)):
                    print(("  > " if k == s else "    ") + ins[k][2].strip())


if __name__ == "__main__":
    main()
