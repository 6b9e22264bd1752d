"""The helper modules of the suite, on the CPU: the comparison of tests/parity.py can fail (stub simulators returning fixed arrays: no
GPU, no oracle library), no module imports a test module, and ROUTING_OVERRIDES names every override cdpr_select.hpp reads."""
import ast
import glob
import os
import re
import types

import numpy as np
import pytest

import parity
from parity import NAMES, TOL, TOL64

HERE = os.path.dirname(os.path.abspath(__file__))
B, N = 3, 2
SHAPES = {"pose": (B, 7), "twist": (B, 6), "q": (B, N), "qd": (B, N), "eff": (B, N)}


class StubOracle:
    """platform_state + joint_states of five fixed arrays (float64 zeros unless given)"""

    def __init__(self, batch=B, dtype=np.float64, **arrays):
        self.a = {k: np.zeros((batch,) + SHAPES[k][1:], dtype) for k in NAMES}
        self.a.update(arrays)

    def platform_state(self):
        return self.a["pose"], self.a["twist"]

    def joint_states(self):
        return self.a["q"], self.a["qd"], self.a["eff"]

    def set_platform_state(self, **kw):
        pass

    def update(self, steps):
        pass


class StubEngine(StubOracle):
    def observables_f64(self):
        return self.a["q"], self.a["qd"], self.a["eff"], self.a["pose"], self.a["twist"]


def one_entry(name, value, robot=1, dtype=np.float64):
    x = np.zeros(SHAPES[name], dtype)
    x[robot, -1] = value
    return x


def front_ends(table):
    """every front-end of the core on this tolerance table: call(engine, oracle)"""
    if table == "TOL64":
        return TOL64, np.float64, [lambda e, o: parity.compare64(e, o, "stub"), lambda e, o: parity.against_the_oracle(e, o, True, "stub")]
    return TOL, np.float32, [lambda e, o: parity.compare(e, o, where="stub"), lambda e, o: parity.against_the_oracle(e, o, False, "stub")]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("table", ["TOL", "TOL64"])
def test_the_comparison_can_fail(table, name):
    tol, dtype, calls = front_ends(table)
    above = float(np.nextafter(tol[name], np.inf))
    f64 = table == "TOL64"
    # the engine reads zero, the oracle -tolerance: the error is the tolerance to the bit, and passes
    eng, ora = StubEngine(dtype=dtype), StubOracle(**{name: one_entry(name, -tol[name])})
    worst = parity.worst_errors(parity.observed(eng, f64), parity.observed(ora), "stub", f64=f64)
    assert {k: v[0] for k, v in worst.items()} == dict(dict.fromkeys(NAMES, 0.0), **{name: tol[name]}) and worst[name][1:] == (1, SHAPES[name][1] - 1)
    for call in calls:
        call(eng, ora)
        with pytest.raises(AssertionError, match=rf"stub: {name} differs from the oracle by .* \(tolerance "):
            call(StubEngine(dtype=dtype), StubOracle(**{name: one_entry(name, -above)}))
        for bad in (np.nan, np.inf, -np.inf):
            with pytest.raises(AssertionError, match=rf"stub: {name} is not finite"):
                call(StubEngine(dtype=dtype, **{name: one_entry(name, bad, dtype=dtype)}), StubOracle())
        if table == "TOL64":
            with pytest.raises(AssertionError, match=rf"stub: {name} is float32, not float64"):
                call(StubEngine(**{name: np.zeros(SHAPES[name], np.float32)}), StubOracle())


def test_compare_returns_nothing_and_compare64_the_worst_errors():
    assert parity.compare(StubEngine(dtype=np.float32), StubOracle()) is None
    assert parity.compare64(StubEngine(), StubOracle(), "stub") == dict.fromkeys(NAMES, 0.0)


def test_the_worst_error_comes_with_its_robot_and_column():
    got = StubEngine(eff=one_entry("eff", 0.25, robot=2)).a
    worst = parity.worst_errors([got[k] for k in NAMES], [np.zeros(SHAPES[k]) for k in NAMES], "stub")
    assert worst["eff"] == (0.25, 2, N - 1) and worst["pose"][0] == 0.0


@pytest.mark.parametrize("name", NAMES)
def test_check_slice_sees_the_robots_of_the_slice_only(name):
    sl = slice(1, 3)
    pkg = types.SimpleNamespace(Config=lambda batch, **kw: types.SimpleNamespace(to_struct=lambda: batch))
    oracle = types.SimpleNamespace(DERIV_EXACT=0, OracleSim=lambda batch, deriv: StubOracle(batch))
    pose = np.zeros((B, 7), np.float32)
    above = np.float32(np.nextafter(np.float32(TOL[name]), np.float32(np.inf)))

    def got(robot):
        return [one_entry(k, above if k == name else 0.0, robot, np.float32) for k in NAMES]

    parity.check_slice(pkg, oracle, {}, sl, pose, [(5, None)], got(0))  # (outside the slice)
    for robot in (1, 2):
        with pytest.raises(AssertionError, match=rf"robots 1 \.\. 2: {name} differs from the oracle by "):
            parity.check_slice(pkg, oracle, {}, sl, pose, [(5, None)], got(robot))
    assert parity.worst_errors(got(2), [np.zeros((2,) + SHAPES[k][1:]) for k in NAMES], "stub", rows=sl)[name][1:] == (2, SHAPES[name][1] - 1)


def test_start_poses_reach_the_simulators_as_the_callers_had_them():
    """pair and oracle_at: float32 values on both sides; pair64: the doubles as given; start of the pid-limit tests (through_f32 false):
    an fp32 engine rounds, the oracle does not."""
    class Sim:
        def __init__(self, *a):
            self.got = {}

        def set_platform_state(self, pose7=None, twist6=None):
            self.got["f32" if isinstance(self, Eng) else "ora"] = pose7

        def set_platform_state_f64(self, pose7=None, twist6=None):
            self.got["f64"] = pose7

    Eng = type("Eng", (Sim,), {})
    pkg, oracle = types.SimpleNamespace(Engine=Eng), types.SimpleNamespace(OracleSim=Sim, DERIV_EXACT=0)
    cfg32, cfg64 = (types.SimpleNamespace(precision=p, to_struct=lambda: None) for p in (32, 64))
    pose = np.full((B, 7), 0.1)  # (no float32)
    rounded = pose.astype(np.float32)
    eng, ora = parity.pair(pkg, oracle, cfg32, pose)
    assert eng.got["f32"].dtype == np.float32 and ora.got["ora"].dtype == np.float64 and np.array_equal(ora.got["ora"], rounded.astype(np.float64))
    eng, ora = parity.pair64(pkg, oracle, cfg64, pose)
    assert np.array_equal(eng.got["f64"], pose) and np.array_equal(ora.got["ora"], pose) and eng.got["f64"].dtype == np.float64
    assert np.array_equal(parity.oracle_at(oracle, cfg64, pose).got["ora"], rounded.astype(np.float64))
    assert [set(e.got) for e in parity.engines(pkg, cfg64, rounded, 2)] == [{"f64"}, {"f64"}] and parity.pair(pkg, oracle, cfg32)[0].got == {}
    (eng,), ora = parity.sims_at(pkg, oracle, cfg32, pose, through_f32=False)
    assert np.array_equal(eng.got["f32"], rounded) and np.array_equal(ora.got["ora"], pose)


@pytest.mark.parametrize("floor", [1e-6, 1e-9])
def test_rollout_cost_tol(floor):
    cost = np.array([[0.5, -3.0], [2.0, 1.0]])
    assert parity.rollout_cost_tol(cost, floor) == floor + 2e-4 * 3.0
    assert parity.rollout_cost_tol(cost.astype(np.float32), floor) == floor + 2e-4 * 3.0


def test_no_module_imports_a_test_module():
    found = []
    for path in sorted(glob.glob(os.path.join(HERE, "*.py"))):
        for node in ast.walk(ast.parse(open(path).read(), path)):
            modules = [a.name for a in node.names] if isinstance(node, ast.Import) else [node.module or ""] if isinstance(node, ast.ImportFrom) else []
            found += [f"{os.path.basename(path)}:{node.lineno}: {m}" for m in modules if m.split(".")[-1].startswith("test_")]
    assert not found, "shared things live in helper modules (tests/parity.py and its neighbours), not in test modules:\n" + "\n".join(found)


def test_routing_overrides_are_those_the_selection_reads():
    text = open(os.path.join(HERE, "..", "cdpr-simulation_amd", "csrc", "cdpr_select.hpp")).read()
    read = set(re.findall(r'\benv\("(CDPR_[A-Z0-9_]+)"\)', text))
    assert len(read) >= 10 and read <= set(parity.ROUTING_OVERRIDES), f"not in parity.ROUTING_OVERRIDES: {sorted(read - set(parity.ROUTING_OVERRIDES))}"
    assert len(set(parity.ROUTING_OVERRIDES)) == len(parity.ROUTING_OVERRIDES)
