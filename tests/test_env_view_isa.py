"""The environment view's translation units on the checks every shipped kernel passes, with the flags of the shipped build (no GPU
needed: hipcc cross-compiles): scripts/exec_lint.py finds no vector work in front of an exec restore in k_env and cdpr_engine_env
(tests/test_isa_lint.py runs the same lint over the units that existed before), and the two kernels use no scratch and spill nothing,
as csrc/cdpr_env.hpp says (their LDS is dynamic - 30 720 B at the widest observation - and does not show in the compiler's table)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exec_lint_over_the_new_units():
    env = dict(os.environ, EXEC_LINT_JOBS="2")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "exec_lint.py"), "--build", "k_env", "cdpr_engine_env"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert "0 finding(s) in 2 file(s)" in r.stdout


def test_the_view_kernels_use_no_scratch():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "resource_usage.py"), "--all", "k_env"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [l for l in r.stdout.splitlines() if re.search(r"\bcdpr_env(_f64)?_kernel<128>", l)]
    assert len(rows) == 2, r.stdout
    for l in rows:
        assert re.search(r"scratch 0\s", l) and re.search(r"spillS 0\s", l) and re.search(r"spillV 0\s", l) and re.search(r"occ [78]\s", l), l
