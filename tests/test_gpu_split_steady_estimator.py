"""The role-split steady kernel's estimator wave (split_estimator_wave<..., STEADY = true>, csrc/cdpr_onestep_kernel.hpp): the Newton stage as
four iterations written out without the convergence test, and the IK rows at the true state evaluated once per robot and handed to the
controller wave through LDS behind a workgroup barrier of their own.

The host takes the steady kernel for a launch only where it also knows fk_tolerance == 0 and fk_max_iterations == 4 (split_steady_launch,
csrc/cdpr_engine_launch.hip); CDPR_SPLIT_STEADY=0 keeps every launch on the generic kernel, which is the reference here.  The comparison is
BIT EQUALITY, no tolerance: the same scenarios run in two fresh child processes, one per setting of CDPR_SPLIT_STEADY, and after every
world step the observables (joint positions, rates, efforts, pose, twist), the `fk` rows (estimate, residual, iteration count) and the
tension rows (tensions, flag) are hashed; the platform rows are read at the end.

1. Steady launches: n = 6, 7, 8, Velocity and Position mode, batch 65 (two workgroups: the second role-swapped and ragged, 63 masked lanes)
   and batch 1, 25 world steps with a new command every 10, from poses across the workspace (tests/workspace_poses.py: box W and the
   special poses).  cdpr_debug_last_variant reports the steady variant from the step on that fills the derivative window.
2. Handles whose estimator contract the steady kernel does not serve - tolerance 1e-6 with 4 iterations, tolerance 0 with 3 and with 8 -
   stay generic on every launch, and both settings agree.  On the tolerance handle the published iteration counts are the fp64 oracle's.
3. A mode switch Velocity -> Position -> Velocity: generic while the window refills, steady again after, the same bits throughout.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import workspace_poses as wp
from parity import ROUTING_OVERRIDES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "cdpr_split_kernel<%d, false>"
STEPS, REFRESH = 25, 10
SWITCH = (("velocity", 20), ("position", 20), ("velocity", 20))  # the mode switch: segments of world steps, a new command every REFRESH
FK_VARIANTS = {"tolerance 1e-6 x 4": dict(fkTolerance=1e-6, fkMaxIterations=4), "tolerance 0 x 3": dict(fkMaxIterations=3), "tolerance 0 x 8": dict(fkMaxIterations=8)}
STEADY = [(f"{mode} n{n} b{b}", n, b, mode) for n in (6, 7, 8) for mode in ("velocity", "position") for b in (65, 1)]
GENERIC = [(f"generic handle: {name}", 8, 65, name) for name in FK_VARIANTS]
SCENARIOS = STEADY + GENERIC + [("mode switch n8 b65", 8, 65, "switch")]
OVERRIDES = ROUTING_OVERRIDES + ("CDPR_SPLIT_STEADY", "CDPR_NO_GRAPH", "CDPR_LIB")


def poses(pkg, model, batch, seed):
    """Start poses over the workspace, float32: the 26 special poses (yaw pi and +-pi / 2, the largest tilts, the corners of W's position
    box, each once more with the quaternion negated) behind poses drawn from box W; a batch of one is one pose from the box."""
    rng = np.random.default_rng(seed)
    if batch <= 2 * wp.N_SPECIAL:
        return wp.box_poses(model, batch, rng, "W").astype(np.float32)
    return np.concatenate([wp.box_poses(model, batch - 2 * wp.N_SPECIAL, rng, "W"), wp.special_poses(model)]).astype(np.float32)


def commands(batch, n, seed):
    """(velocity commands j -> float32[B, n] in +-0.03 m/s, position offsets j -> float32[B, n] in +-0.004 m): workspace_poses' script ranges."""
    rng = np.random.default_rng(seed)
    v, off = rng.uniform(-0.03, 0.03, (8, batch, n)).astype(np.float32), rng.uniform(-0.004, 0.004, (8, batch, n)).astype(np.float32)
    return (lambda j: v[j]), (lambda j: off[j])


def command(eng, mode, j, vel, off):
    """Command j of a segment in `mode`; position targets are the engine's current joint positions plus the offset (equal in both runs as
    long as the runs are: a difference shows in the step before)."""
    if mode == "velocity":
        eng.set_velocity_command(vel(j))
    else:
        eng.set_position_command((eng.joint_states()[0] + off(j)).astype(np.float32))


def digest(arrays):
    return hashlib.sha256(b"".join(np.ascontiguousarray(x).tobytes() for x in arrays)).hexdigest()


def run_scenarios():
    """(child process) Every scenario on the library as the environment selects it -> {name: {digest: [per step, final], variant, kernel, finite}}."""
    import cdpr_simulation_amd as pkg

    out = {}
    for name, n, batch, kind in SCENARIOS:
        model = wp.cell_model(pkg, n)
        eng = pkg.Engine(pkg.Config(model=model, batch=batch, stages=3, **FK_VARIANTS.get(kind, {})), 0)
        eng.set_platform_state(pose7=poses(pkg, model, batch, 1000 * n + batch))
        vel, off = commands(batch, n, 77 * n + batch)
        segments = SWITCH if kind == "switch" else ((kind if kind in ("velocity", "position") else "velocity", STEPS),)
        dig, variant, kernel, j = [], [], set(), 0
        for mode, steps in segments:
            for k in range(steps):
                if k % REFRESH == 0:
                    command(eng, mode, j, vel, off)
                    j += 1
                eng.update(1)
                dig.append(digest(list(eng.observables()) + list(eng.fk_state()) + list(eng.td_state())))
                variant.append(eng.last_variant)
                kernel.add(eng.kernel_name)
        final = list(eng.raw_state()) + list(eng.fk_state()) + list(eng.td_state())
        dig.append(digest(final))
        out[name] = {"digest": dig, "variant": variant, "kernel": sorted(kernel), "finite": bool(all(np.isfinite(x).all() for x in final)),
                     "iterations": sorted(set(int(i) for i in eng.fk_state()[2]))}
        eng.close()
    print(json.dumps(out))


_runs = {}


def child(setting):
    """The scenarios in a fresh process with CDPR_SPLIT_STEADY unset (None) or set; run once per setting."""
    if setting not in _runs:
        env = dict(os.environ)
        for k in OVERRIDES:
            env.pop(k, None)
        if setting is not None:
            env["CDPR_SPLIT_STEADY"] = setting
        env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, f"CDPR_SPLIT_STEADY={setting}: the scenario run failed\n{r.stdout[-1000:]}\n{r.stderr[-3000:]}"
        _runs[setting] = json.loads(r.stdout.strip().splitlines()[-1])
    return _runs[setting]


def same_bits(name, n):
    steady, generic = child(None)[name], child("0")[name]
    assert steady["kernel"] == generic["kernel"] == [KERNEL % n]
    assert not any(generic["variant"]), "CDPR_SPLIT_STEADY=0 must keep every launch on the generic kernel"
    assert steady["finite"] and generic["finite"], f"{name}: the final state is not finite"
    moved = [k for k, (a, b) in enumerate(zip(steady["digest"], generic["digest"])) if a != b]
    assert len(steady["digest"]) == len(generic["digest"]) and not moved, f"{name}: steps {moved} differ (the last entry is the final state)"
    return steady


@pytest.mark.parametrize("name,n,batch,mode", STEADY, ids=[s[0] for s in STEADY])
def test_steady_launches_match_the_generic_kernel(pkg, name, n, batch, mode):
    steady = same_bits(name, n)
    nbuf = getattr(pkg.Config(), mode + "Controller").dBufferLength
    # Pid call k - 1 happens at world step k, so the window of nbuf errors is full from world step nbuf + 1 on
    assert steady["variant"] == [0] * (nbuf + 1) + [1] * (STEPS - nbuf - 1), steady["variant"]
    assert steady["iterations"] == [4]


@pytest.mark.parametrize("name,n,batch,variant", GENERIC, ids=[s[0] for s in GENERIC])
def test_other_estimator_contracts_stay_generic(name, n, batch, variant):
    steady = same_bits(name, n)
    assert not any(steady["variant"]), f"{name}: the steady kernel has no code for this handle's Newton stage"
    if "fkMaxIterations" in FK_VARIANTS[variant] and "fkTolerance" not in FK_VARIANTS[variant]:
        assert steady["iterations"] == [FK_VARIANTS[variant]["fkMaxIterations"]]


def test_iteration_counts_with_a_tolerance_are_the_oracles(pkg, oracle, monkeypatch):
    """tolerance 1e-6 x 4, the scenario of test_other_estimator_contracts_stay_generic, beside the fp64 oracle: after the last step the
    published iteration counts are equal.  Left out are robots of workspace_poses' exit class at that step: the residual the ORACLE tests
    before one of its iterations lies within FK_EXIT_MARGIN (2e-7 m, 3 ulp of a cable length) of the tolerance, where float32 and float64
    may leave the loop an iteration apart."""
    for k in OVERRIDES:
        monkeypatch.delenv(k, raising=False)
    n, batch, kw = 8, 65, FK_VARIANTS["tolerance 1e-6 x 4"]
    model = wp.cell_model(pkg, n)
    cfg = pkg.Config(model=model, batch=batch, stages=3, **kw)
    eng, ora = pkg.Engine(cfg, 0), oracle.OracleSim(cfg.to_struct())
    pose = poses(pkg, model, batch, 1000 * n + batch)
    eng.set_platform_state(pose7=pose), ora.set_platform_state(pose7=pose.astype(np.float64))
    vel, _ = commands(batch, n, 77 * n + batch)
    for k in range(STEPS):
        if k % REFRESH == 0:
            eng.set_velocity_command(vel(k // REFRESH)), ora.set_velocity_command(vel(k // REFRESH))
        if k == STEPS - 1:
            (true_pose, true_twist), seed = ora.platform_state(), ora.fk_state()[0]
        eng.update(1), ora.update(1)
        assert eng.last_variant == 0 and eng.kernel_name == KERNEL % n
    it, oit = eng.fk_state()[2], ora.fk_state()[2]
    # the residual the oracle tests before iteration k of the last step (column k: after k iterations)
    res_seq = np.empty((batch, kw["fkMaxIterations"] + 1))
    for k in range(kw["fkMaxIterations"] + 1):
        sk = pkg.Config(model=model, batch=1, stages=3, fkMaxIterations=max(k, 1), fkTolerance=0.0 if k else 1e9).to_struct()
        for r in range(batch):
            lengths = oracle.ik(cfg.to_struct(), true_pose[r], true_twist[r])[2]
            res_seq[r, k] = oracle.fk(sk, lengths, seed[r])[1]
    exit_class = wp.fk_exit_class(dict(res_seq=res_seq, fk_tolerance=kw["fkTolerance"]))
    print(f"iteration counts: engine {np.bincount(it, minlength=5)}, oracle {np.bincount(oit, minlength=5)}, exit class {int(exit_class.sum())} of {batch} robots")
    assert exit_class.mean() <= 0.1
    assert np.array_equal(it[~exit_class], oit[~exit_class]), (it, oit, res_seq)
    eng.close()


def test_mode_switch_refills_the_window_on_the_generic_kernel(pkg):
    steady = same_bits("mode switch n8 b65", 8)
    v, at = steady["variant"], 0
    for i, (mode, steps) in enumerate(SWITCH):
        nbuf = getattr(pkg.Config(), mode + "Controller").dBufferLength
        # the first segment starts at world step 0 (no Pid call); a later one at a mode change, whose Pid reset empties the window: the
        # launch that makes call nbuf is the first to see it full
        fill = nbuf + 1 if i == 0 else nbuf
        assert v[at:at + fill] == [0] * fill and all(v[at + fill + 1:at + steps]), (mode, at, v)
        at += steps


if __name__ == "__main__":
    run_scenarios()
