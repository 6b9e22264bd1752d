"""The translation units of the kernels over chosen robots (csrc/cdpr_robot_records.hpp: latch and flush in cdpr_engine_launch, reset in
cdpr_engine_reset, copy in cdpr_engine_copy) on the checks every shipped kernel passes, with the flags of the shipped build (no GPU
needed: hipcc cross-compiles): scripts/exec_lint.py finds nothing in them, and the ten kernels use no scratch, no LDS and spill
nothing (a copy's batch of eight rows in flight must stay in registers)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLEAN = (r"scratch 0\s", r"spillS 0\s", r"spillV 0\s", r"lds 0\s*$", r"occ 8\s")


def lint(*units):
    env = dict(os.environ, EXEC_LINT_JOBS="2")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "exec_lint.py"), "--build", *units], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert f"0 finding(s) in {len(units)} file(s)" in r.stdout


def resource_rows(unit, pattern):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "resource_usage.py"), "--all", unit], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return [l for l in r.stdout.splitlines() if re.search(pattern, l)], r.stdout


def test_exec_lint_over_the_new_unit():
    lint("cdpr_engine_copy")


def test_the_copy_kernels_use_no_scratch_and_no_lds():
    rows, out = resource_rows("cdpr_engine_copy", r"\bcdpr_copy_(fast|gen|f64)_kernel\b")
    assert len(rows) == 3, out
    for l in rows:
        assert all(re.search(p, l) for p in CLEAN), l


def test_exec_lint_over_the_latch_and_reset_units():
    lint("cdpr_engine_launch", "cdpr_engine_reset")


@pytest.mark.parametrize("unit, pattern, count", [
    ("cdpr_engine_launch", r"\bcdpr_(latch_fast|gen_latch|latch_f64|gen_flush_hot)_kernel\b", 4),
    ("cdpr_engine_reset", r"\bcdpr_reset_(fast|gen|f64)_kernel\b", 3),
])
def test_the_latch_flush_and_reset_kernels_use_no_scratch_and_no_lds(unit, pattern, count):
    rows, out = resource_rows(unit, pattern)
    assert len(rows) == count, out
    for l in rows:
        assert all(re.search(p, l) for p in CLEAN), l
