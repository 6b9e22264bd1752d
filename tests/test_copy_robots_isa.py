"""The copy kernels' translation unit on the checks every shipped kernel passes, with the flags of the shipped build (no GPU needed:
hipcc cross-compiles): scripts/exec_lint.py finds nothing in cdpr_engine_copy, and the three kernels use no scratch, no LDS and spill
nothing, as csrc/cdpr_copy.hpp says (a batch of eight rows in flight must stay in registers)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exec_lint_over_the_new_unit():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "exec_lint.py"), "--build", "cdpr_engine_copy"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert "0 finding(s) in 1 file(s)" in r.stdout


def test_the_copy_kernels_use_no_scratch_and_no_lds():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "resource_usage.py"), "--all", "cdpr_engine_copy"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [l for l in r.stdout.splitlines() if re.search(r"\bcdpr_copy_(fast|gen|f64)_kernel\b", l)]
    assert len(rows) == 3, r.stdout
    for l in rows:
        assert re.search(r"scratch 0\s", l) and re.search(r"spillS 0\s", l) and re.search(r"spillV 0\s", l) and re.search(r"lds 0\s*$", l) and re.search(r"occ 8\s", l), l
