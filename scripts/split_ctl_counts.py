#!/usr/bin/env python3
"""Instruction classes of the role-split kernel's two waves, from hipcc's -S output of k_onestep.hip (static counts: every side of a
scalar branch is counted, e.g. all five ring-row layouts of which a launch runs one).

A wave's code is what is reachable from its entry: the controller wave's from its `s_sleep` (CDPR_CTL_LOAD_DELAY), the estimator wave's
from the target of the role branch in the kernel's prologue.  The workgroup barriers cut it into regions:

  controller wave   before the hand-off (up to the two consecutive `s_barrier`s: #1 force hand-off, #2 tensions back; where the steady
                    kernel takes the estimator wave's IK rows, barrier #0 cuts this part in two) and the TAIL behind barrier #2
  estimator wave    up to barrier #1 (the steady kernel with the shared IK: up to #0, then up to #1) and the tension distribution between
                    #1 and #2.  A backward branch in the part before #1 is the Newton loop: that part is then given as before the loop,
                    loop body and behind the loop, and the EXECUTED count is before + 4 x body + behind (the flagship's four iterations);
                    without a loop (the iterations written out) the executed count is the static one.

  python scripts/split_ctl_counts.py file.s [kernel-substring ...]     default: cdpr_split_kernel<8, false> and cdpr_split_steady_kernel<8, VEL>
  python scripts/split_ctl_counts.py --build [-DNAME=VALUE ...] [kernel-substring ...]    compile csrc/k_onestep.hip first"""
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
NEWTON_ITERATIONS = 4


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


class Kernel:
    """One kernel's instruction lines and labels, and walks over its control flow."""

    def __init__(self, body):
        self.ins = []
        for l in body.split("\n"):
            t = l.split(";")[0].strip()
            if re.match(r"^\.LBB\d+_\d+:", t):
                self.ins.append(t)
            elif l.startswith("\t") and t and not t.startswith("."):
                self.ins.append(t)
        self.label_at = {t[:-1]: i for i, t in enumerate(self.ins) if t.endswith(":")}
        self.sleep = next(i for i, l in enumerate(self.ins) if l.startswith("s_sleep"))
        # the role branch of the kernel's prologue: its target is the estimator wave's entry, laid out behind the controller's last block
        self.est_labels = {m.group(1) for t in self.ins[: self.sleep] if (m := re.match(r"s_cbranch_\w+\s+(\S+)", t))}

    def walk(self, start, fence=()):
        """(indices of the instructions reachable from `start` up to the next `s_barrier` / `s_endpgm`, indices of the barriers met);
        labels in `fence` are not entered."""
        ins, seen, out, ends, todo = self.ins, set(), [], set(), [start]
        while todo:
            i = todo.pop()
            while i < len(ins) and i not in seen:
                seen.add(i)
                t = ins[i]
                if t.endswith(":"):
                    if t[:-1] in fence:
                        break
                    i += 1
                    continue
                if t == "s_barrier":
                    ends.add(i)
                    break
                if t == "s_endpgm":
                    break
                out.append(i)
                m = re.match(r"s_(cbranch_\w+|branch)\s+(\S+)", t)
                if m and m.group(2) in self.label_at:
                    todo.append(self.label_at[m.group(2)])
                    if m.group(1) == "branch":
                        break
                i += 1
        return sorted(out), sorted(ends)

    def successors(self, i):
        t = self.ins[i]
        m = re.match(r"s_(cbranch_\w+|branch)\s+(\S+)", t)
        out = []
        if m and m.group(2) in self.label_at:
            j = self.label_at[m.group(2)]
            while self.ins[j].endswith(":"):
                j += 1
            out.append(j)
            if m.group(1) == "branch":
                return out
        j = i + 1
        while j < len(self.ins) and self.ins[j].endswith(":"):
            j += 1
        return out + [j]

    def reach(self, starts, within):
        """Instructions of `within` reachable from `starts` over at least one edge (the block layout is not the control flow's order)."""
        seen, todo = set(), list(starts)
        while todo:
            for j in self.successors(todo.pop()):
                if j in within and j not in seen:
                    seen.add(j)
                    todo.append(j)
        return seen

    def cycle(self, idx):
        """The instructions of `idx` that lie on a cycle within it (the Newton loop), sorted; empty without one."""
        within = set(idx)
        branches = [i for i in idx if re.match(r"s_cbranch_", self.ins[i])]  # every cycle passes a conditional branch
        on = set()
        for b in branches:
            r = self.reach([b], within)
            if b in r:
                on |= {i for i in r if b in self.reach([i], within)}
        return sorted(on)

    def regions_of(self, start, fence=()):
        """The wave's regions in order: [(instruction indices, True if the region ends at two consecutive barriers)]."""
        out = []
        while True:
            idx, ends = self.walk(start, fence)
            if not ends:
                out.append((idx, False))
                return out
            assert len(ends) == 1, "a region of a wave ends at ONE barrier"
            double = self.ins[ends[0] + 1] == "s_barrier"
            out.append((idx, double))
            start = ends[0] + (2 if double else 1)

    def controller(self):
        """[(label, instruction lines)]: before the hand-off (in two parts where barrier #0 cuts it), the tail."""
        regs = self.regions_of(self.sleep, self.est_labels)
        cut = next(k for k, (_, double) in enumerate(regs) if double)
        assert cut in (0, 1) and len(regs) == cut + 2
        names = ["before the hand-off"] if cut == 0 else ["up to barrier #0", "#0 to the hand-off"]
        return [(n, [self.ins[i] for i in idx]) for n, (idx, _) in zip(names + ["tail after barrier #2"], regs)]

    def estimator(self):
        """([(label, instruction lines)], executed vector instructions of the whole wave)."""
        entry = min(self.label_at[l] for l in self.est_labels if l in self.label_at and self.label_at[l] > self.sleep)
        regs = [idx for idx, _ in self.regions_of(entry)]
        assert len(regs) in (3, 4) and not regs[-1], "estimator wave: [#0,] #1, #2, then nothing but the end of the program"
        regs = regs[:-1]
        names = ["up to barrier #1"] if len(regs) == 2 else ["up to barrier #0", "#0 to barrier #1"]
        out, executed = [], 0
        vec = lambda idx: sum(1 for i in idx if self.ins[i].startswith("v_"))
        for n, idx in zip(names + ["#1 to #2 (TD)"], regs):
            loop = self.cycle(idx)
            if loop:
                inside, idx_set = set(loop), set(idx)
                behind = self.reach(loop, idx_set) - inside
                parts = [("before the loop", [i for i in idx if i not in inside and i not in behind]), ("loop body", loop), ("behind the loop", sorted(behind))]
                out += [(f"{n}: {p}", [self.ins[i] for i in sub]) for p, sub in parts]
                executed += vec(parts[0][1]) + NEWTON_ITERATIONS * vec(parts[1][1]) + vec(parts[2][1])
            else:
                out.append((n, [self.ins[i] for i in idx]))
                executed += vec(idx)
        return out, executed


def main(argv):
    if argv and argv[0] == "--build":
        defs = [x for x in argv[1:] if x.startswith("-D")]
        path = os.path.join(tempfile.mkdtemp(prefix="split_ctl_counts_"), "k_onestep.s")
        r = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS.split(), *defs, "-o", path, "k_onestep.hip"], cwd=CSRC, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(r.stderr[-2000:])
        pats = [x for x in argv[1:] if not x.startswith("-D")]
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
        occ = re.search(r"; Occupancy: (\d+)", body)
        m = meta.get(name, {})
        print(f"{dn}   ({m.get('vgpr_count', '?')} VGPRs, {m.get('agpr_count', '?')} AGPRs, {m.get('vgpr_spill_count', '?')} spilled VGPRs, {m.get('sgpr_spill_count', '?')} spilled SGPRs, "
              f"{m.get('private_segment_fixed_size', '?')} B scratch, {m.get('group_segment_fixed_size', '?')} B LDS, occupancy {occ.group(1) if occ else '?'} waves per SIMD)")
        print(f"  {'region':42s} {'vector':>6s} " + " ".join(f"{c:>8s}" for c in CLASSES) + f" {'scalar':>7s} {'vmem ld':>7s} {'vmem st':>7s} {'lds':>5s}")
        k = Kernel(body)
        est, est_executed = k.estimator()
        ctl = k.controller()
        for wave, regs in (("controller", ctl), ("estimator", est)):
            for label, reg in regs:
                ops = [l.split()[0] for l in reg]
                c = Counter(classify(o) for o in ops if o.startswith("v_"))
                vec = sum(c.values())
                sc = sum(1 for o in ops if o.startswith("s_") and not o.startswith(("s_waitcnt", "s_nop")))
                ld = sum(1 for o in ops if re.match(r"(global|buffer|flat)_load", o))
                stc = sum(1 for o in ops if re.match(r"(global|buffer|flat)_store", o))
                lds = sum(1 for o in ops if o.startswith("ds_"))
                print(f"  {wave[:3] + ' ' + label:42s} {vec:6d} " + " ".join(f"{c[x]:8d}" for x in CLASSES) + f" {sc:7d} {ld:7d} {stc:7d} {lds:5d}")
        ctl_static = sum(sum(1 for l in reg if l.startswith("v_")) for _, reg in ctl)
        print(f"  vector instructions per 64 robots: controller wave {ctl_static} (static), estimator wave {est_executed} (executed at {NEWTON_ITERATIONS} Newton iterations), "
              f"together {ctl_static + est_executed}")


if __name__ == "__main__":
    main(sys.argv[1:])
