#!/usr/bin/env python3
"""Device code of two source trees, kernel by kernel (no GPU needed): did a change of the sources move any kernel's
code or resources?

  python scripts/isa_compare.py emit [--jobs 8] CSRC_DIR OUT_DIR [unit ...]   # device-only assembly of every k_*.hip unit
  python scripts/isa_compare.py table OUT_DIR_A OUT_DIR_B                      # the comparison, A -> B
  python scripts/isa_compare.py rule [--band 1.0] OUT_DIR_A OUT_DIR_B          # the stage-factoring rule on that comparison

`emit` compiles with the unit's flags from csrc/Makefile (FLAGS and the NOVC / NOSLP / k_f64_hold_long additions, read
from the Makefile of CSRC_DIR).  `table` prints one line per kernel (and per non-inlined device function): "identical"
where the instruction stream is the same text, else the total and vector instruction counts A -> B; then the resource
fields of the code object's metadata and the occupancy, and "RESOURCES MOVED" where one of them differs.  A unit whose
whole text is equal apart from the __hip_cuid_ symbol is reported in one line.  Exit status 1 if any resource moved.  `rule` checks, per kernel, what a stage function may not move
(csrc/cdpr_step_stages_f64.hpp): scratch, spilled VGPRs, LDS and occupancy equal and the vector instruction count not more than
--band per cent up; it lists the kernels that fail and the ones whose spilled-SGPR, VGPR or AGPR counts moved (allowed, recorded);
exit status 1 if a kernel fails."""
import argparse
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # as csrc/Makefile
RES_KEYS = [".vgpr_count", ".agpr_count", ".sgpr_spill_count", ".vgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size"]


def unit_flags(csrc):
    mk = open(os.path.join(csrc, "Makefile")).read()
    base = re.search(r"^FLAGS := (.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").split()
    extra = {}
    for var, add in re.findall(r"^\$\((\w+):%=\$\(OBJDIR\)/%\.o\): FLAGS \+= (.*)$", mk, re.M):
        for u in re.search(r"^%s := (.*)$" % var, mk, re.M).group(1).split():
            extra.setdefault(u, []).extend(add.split())
    for u, add in re.findall(r"^\$\(OBJDIR\)/(\w+)\.o: FLAGS \+= (.*)$", mk, re.M):
        extra.setdefault(u, []).extend(add.split())
    return base, extra


def emit(csrc, out, jobs, units):
    os.makedirs(out, exist_ok=True)
    base, extra = unit_flags(csrc)
    units = units or sorted(f[:-4] for f in os.listdir(csrc) if f.startswith("k_") and f.endswith(".hip"))

    def one(u):
        cmd = [HIPCC, *base, *extra.get(u, []), "--offload-device-only", "-S", "-o", os.path.join(os.path.abspath(out), u + ".s"), u + ".hip"]
        r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
        return u, r.returncode, r.stderr

    bad = 0
    with ThreadPoolExecutor(jobs) as ex:
        for u, rc, err in ex.map(one, units):
            err = "".join(l for l in err.splitlines(True) if "argument unused during compilation" not in l)
            print(f"{u}: {'ok' if rc == 0 else 'FAILED'}{' (warnings)' if rc == 0 and 'warning' in err else ''}", flush=True)
            sys.stderr.write(err)
            bad |= rc != 0
    return 1 if bad else 0


def functions(text):
    """name -> (instruction lines, occupancy) for every function of one assembly file."""
    out = {}
    starts = [(m.start(), m.end(), m.group(1)) for m in re.finditer(r"^(_Z\w+):[^\n]*\n", text, re.M)]
    for (_, pos, name), nxt in zip(starts, starts[1:] + [(len(text), 0, "")]):
        seg = text[pos:nxt[0]]
        end = re.search(r"^\.Lfunc_end\d+:", seg, re.M)
        if not end:
            continue
        body, tail = seg[:end.start()], seg[end.end():]
        ins = []
        for l in body.split("\n"):
            l = l.split(";")[0].strip()
            if not l or l.startswith(".") or l.endswith(":"):
                continue
            # (.LBB<i>_<j>: block j of the unit's i-th function - i moves when a function in front of this one comes or goes)
            ins.append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s+", " ", l)))
        occ = re.search(r"; Occupancy: (\d+)", tail)
        out[name] = (ins, int(occ.group(1)) if occ else -1)
    return out


def metadata(text):
    """kernel name -> resource fields of the code object's metadata."""
    out = {}
    md = text[text.find("amdhsa.kernels:"):]
    for block in re.split(r"^  - (?=\.\w+:)", md, flags=re.M)[1:]:  # one list item per kernel, whatever its first key
        block = "    " + block  # (the item's first key follows the dash)
        name = re.search(r"^    \.name:\s+(\S+)", block, re.M)  # (the kernel's own .name: four spaces; argument names sit deeper)
        if not name or not all(re.search(r"^    " + re.escape(k) + r":", block, re.M) for k in RES_KEYS):
            continue
        out[name.group(1)] = {k: int(re.search(r"^    " + re.escape(k) + r":\s+(\d+)", block, re.M).group(1)) for k in RES_KEYS}
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return [re.sub(r"\((cdpr::)?\w+Args(, (cdpr::)?GenCtl)?\)$", "", n.replace("void cdpr::", "").replace("cdpr::", "")) for n in r.stdout.split("\n")]


def table(da, db):
    moved = 0
    for f in sorted(os.listdir(da)):
        if not f.endswith(".s"):
            continue
        ta, tb = open(os.path.join(da, f)).read(), open(os.path.join(db, f)).read()
        strip = lambda t: re.sub(r"__hip_cuid_\w+", "__hip_cuid_", t)
        fa, fb, ma, mb = functions(ta), functions(tb), metadata(ta), metadata(tb)
        if strip(ta) == strip(tb):
            print(f"== {f[:-2]}: {len(fa)} functions, the whole unit identical apart from __hip_cuid_")
            continue
        print(f"== {f[:-2]}")
        if set(fa) != set(fb):
            print(f"   SYMBOLS DIFFER: only in A {sorted(set(fa) - set(fb))}, only in B {sorted(set(fb) - set(fa))}")
            moved += 1
        names = [n for n in fa if n in fb]
        for n, dn in zip(names, demangle(names)):
            (ia, oa), (ib, ob) = fa[n], fb[n]
            va, vb = sum(i.startswith("v_") for i in ia), sum(i.startswith("v_") for i in ib)
            code = "identical" if ia == ib else f"total {len(ia)} -> {len(ib)}, vector {va} -> {vb}"
            ra, rb = dict(ma.get(n, {}), occupancy=oa), dict(mb.get(n, {}), occupancy=ob)
            res = "resources equal" if ra == rb else "RESOURCES MOVED " + ", ".join(f"{k} {ra[k]} -> {rb[k]}" for k in ra if ra[k] != rb.get(k))
            moved += ra != rb
            r = ra
            kind = "" if n in ma else " [function]"
            summary = f"V{r.get('.vgpr_count', '-')} A{r.get('.agpr_count', '-')} spillS {r.get('.sgpr_spill_count', '-')} spillV {r.get('.vgpr_spill_count', '-')} " \
                      f"scratch {r.get('.private_segment_fixed_size', '-')} lds {r.get('.group_segment_fixed_size', '-')} occ {oa}"
            print(f"   {dn}{kind}: {code}; {res} ({summary})")
    print(f"# kernels or functions whose resources moved: {moved}")
    return 1 if moved else 0


HARD_KEYS = [".vgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size", "occupancy"]


def rule(da, db, band):
    n = ident = failing = 0
    worst, soft_lines = 0.0, []
    for f in sorted(os.listdir(da)):
        if not f.endswith(".s") or not os.path.exists(os.path.join(db, f)):
            continue
        ta, tb = open(os.path.join(da, f)).read(), open(os.path.join(db, f)).read()
        fa, fb, ma, mb = functions(ta), functions(tb), metadata(ta), metadata(tb)
        names = [k for k in fa if k in fb and k in ma]
        for k, dn in zip(names, demangle(names)):
            (ia, oa), (ib, ob) = fa[k], fb[k]
            n += 1
            ident += ia == ib
            va, vb = sum(i.startswith("v_") for i in ia), sum(i.startswith("v_") for i in ib)
            growth = 100.0 * (vb - va) / va if va else 0.0
            worst = max(worst, growth)
            ra, rb = dict(ma[k], occupancy=oa), dict(mb.get(k, {}), occupancy=ob)
            hard = [f"{x} {ra[x]} -> {rb.get(x)}" for x in HARD_KEYS if ra[x] != rb.get(x)]
            soft = [f"{x} {ra[x]} -> {rb.get(x)}" for x in ra if x not in HARD_KEYS and ra[x] != rb.get(x)]
            if hard or growth > band:
                failing += 1
                print(f"FAIL {f[:-2]} {dn}: vector {va} -> {vb} ({growth:+.2f} %){'; ' if hard else ''}{', '.join(hard)}")
            elif soft:
                soft_lines.append(f"soft {f[:-2]} {dn}: vector {va} -> {vb} ({growth:+.2f} %); {', '.join(soft)}")
    print("\n".join(soft_lines))
    print(f"# {n} kernels compared, {ident} identical text, {len(soft_lines)} with only spilled-SGPR / VGPR / AGPR counts moved, "
          f"worst vector growth {worst:+.2f} %, failing the rule (band {band} %): {failing}")
    return 1 if failing else 0


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    e = sub.add_parser("emit")
    e.add_argument("csrc")
    e.add_argument("out")
    e.add_argument("units", nargs="*")
    e.add_argument("--jobs", type=int, default=8)
    t = sub.add_parser("table")
    t.add_argument("a")
    t.add_argument("b")
    r = sub.add_parser("rule")
    r.add_argument("a")
    r.add_argument("b")
    r.add_argument("--band", type=float, default=1.0)
    a = ap.parse_args()
    sys.exit(emit(a.csrc, a.out, a.jobs, a.units) if a.cmd == "emit" else rule(a.a, a.b, a.band) if a.cmd == "rule" else table(a.a, a.b))


if __name__ == "__main__":
    main()
