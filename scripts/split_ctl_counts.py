#!/usr/bin/env python3
"""Instruction classes of the role-split kernel's CONTROLLER wave, from hipcc's -S output of k_onestep.hip (static counts: every
side of a scalar branch is counted, e.g. all five ring-row layouts of which a launch runs one).

The controller wave's code is what is reachable from its `s_sleep` (CDPR_CTL_LOAD_DELAY); the two consecutive `s_barrier`s (#1 force
hand-off, #2 tensions back) cut it into the part BEFORE the hand-off and the TAIL after it.

  python scripts/split_ctl_counts.py file.s [kernel-substring ...]     default: cdpr_split_kernel<8, false> and cdpr_split_steady_kernel<8, VEL>
  python scripts/split_ctl_counts.py --build [kernel-substring ...]    compile csrc/k_onestep.hip first"""
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cdpr-simulation_amd", "csrc")
FLAGS = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function --cuda-device-only -S"
CLASSES = ["packed", "plain", "transc", "select", "move", "addr64", "lane r/w", "compare", "accvgpr"]


def classify(op):
    if "accvgpr" in op:
        return "accvgpr"
    if re.match(r"v_(readlane|writelane|readfirstlane)", op):
        return "lane r/w"
    if op.startswith("v_cndmask"):
        return "select"
    if re.match(r"v_(pk_)?mov|v_swap|v_perm", op):
        return "move"
    if op.startswith("v_lshl_add_u64") or op.startswith("v_add_co") or op.startswith("v_addc"):
        return "addr64"
    if op.startswith("v_cmp"):
        return "compare"
    if re.match(r"v_(rsq|rcp|sqrt|sin|cos|exp|log)", op):
        return "transc"
    return "packed" if op.startswith("v_pk_") else "plain"


def regions(body):
    """(before the hand-off, tail) as lists of instruction lines of one kernel's text: the instructions REACHABLE from the controller
    wave's `s_sleep` up to barrier #1, and from behind barrier #2 up to `s_endpgm` (the block layout interleaves the two waves'
    code, so a stretch of text between two markers also holds blocks of the estimator wave)."""
    ins = []
    for l in body.split("\n"):
        t = l.split(";")[0].strip()
        if re.match(r"^\.LBB\d+_\d+:", t):
            ins.append(t)
        elif l.startswith("\t") and t and not t.startswith("."):
            ins.append(t)
    label_at = {t[:-1]: i for i, t in enumerate(ins) if t.endswith(":")}
    other_wave = set()

    def walk(start):
        seen, out, todo = set(), [], [start]
        while todo:
            i = todo.pop()
            while i < len(ins) and i not in seen:
                seen.add(i)
                t = ins[i]
                if t.endswith(":"):
                    if t[:-1] in other_wave:  # the estimator wave's entry: laid out behind the controller's last block
                        break
                    i += 1
                    continue
                if t in ("s_barrier", "s_endpgm"):
                    break
                out.append(t)
                m = re.match(r"s_(cbranch_\w+|branch)\s+(\S+)", t)
                if m and m.group(2) in label_at:
                    todo.append(label_at[m.group(2)])
                    if m.group(1) == "branch":
                        break
                i += 1
        return out

    start = next(i for i, l in enumerate(ins) if l.startswith("s_sleep"))
    other_wave.update(m.group(1) for t in ins[:start] if (m := re.match(r"s_cbranch_\w+\s+(\S+)", t)))  # the role branch of the kernel's prologue
    b1 = next(i for i in range(start, len(ins) - 1) if ins[i] == "s_barrier" and ins[i + 1] == "s_barrier")
    return walk(start), walk(b1 + 2)


def main(argv):
    if argv and argv[0] == "--build":
        path = os.path.join(tempfile.mkdtemp(prefix="split_ctl_counts_"), "k_onestep.s")
        r = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS.split(), "-o", path, "k_onestep.hip"], cwd=CSRC, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(r.stderr[-2000:])
        pats = argv[1:]
    else:
        path, pats = argv[0], argv[1:]
    pats = pats or ["cdpr_split_kernelILi8ELb0E", "cdpr_split_steady_kernelILi8E"]
    s = open(path).read()
    starts = [(m.start(), m.group(1)) for m in re.finditer(r"\n(_ZN4cdpr\w+):", s)]
    meta = {}  # the code object's metadata (amdhsa.kernels): one entry per kernel, `.key: value` lines
    for entry in re.split(r"\n  - ", s[s.find("amdhsa.kernels"):]):
        kv = dict(re.findall(r"\.(\w+):\s+(\S+)", entry))
        if "name" in kv:
            meta[kv["name"]] = kv
    for (pos, name), nxt in zip(starts, starts[1:] + [(len(s), "")]):
        if not re.search(r"cdpr_split_(steady_)?kernel", name) or not any(p in name for p in pats):
            continue
        dn = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().split("(")[0]
        body = s[pos:nxt[0]]
        print(f"{dn}   ({meta.get(name, {}).get('vgpr_count', '?')} VGPRs, {meta.get(name, {}).get('sgpr_spill_count', '?')} spilled SGPRs, "
              f"{meta.get(name, {}).get('private_segment_fixed_size', '?')} B scratch)")
        print(f"  {'region':22s} {'vector':>6s} " + " ".join(f"{c:>8s}" for c in CLASSES) + f" {'scalar':>7s} {'vmem ld':>7s} {'vmem st':>7s} {'lds':>5s}")
        for label, reg in zip(("before the hand-off", "tail after barrier #2"), regions(body)):
            ops = [l.split()[0] for l in reg]
            c = Counter(classify(o) for o in ops if o.startswith("v_"))
            vec = sum(c.values())
            sc = sum(1 for o in ops if o.startswith("s_") and not o.startswith(("s_waitcnt", "s_nop")))
            ld = sum(1 for o in ops if re.match(r"(global|buffer|flat)_load", o))
            stc = sum(1 for o in ops if re.match(r"(global|buffer|flat)_store", o))
            lds = sum(1 for o in ops if o.startswith("ds_"))
            print(f"  {label:22s} {vec:6d} " + " ".join(f"{c[k]:8d}" for k in CLASSES) + f" {sc:7d} {ld:7d} {stc:7d} {lds:5d}")


if __name__ == "__main__":
    main(sys.argv[1:])
