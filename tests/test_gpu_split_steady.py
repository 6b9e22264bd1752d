"""The role-split kernel's steady-state controller wave (split_controller_wave<N, false, true, VEL>, csrc/cdpr_onestep_kernel.hpp).

The host takes it for a launch of cdpr_split_kernel<N, false> when the handle is uniform and in Velocity or Position mode, the
launch is not world step 0, the derivative window is full, every step is published and neither the `pid` topic nor the travel
flags are on (split_steady_launch, csrc/cdpr_engine.hip); CDPR_SPLIT_STEADY=0 keeps every launch on the generic instantiation.

1. Both instantiations compute the same BITS: the same scenarios run in two fresh child processes, one per setting of
   CDPR_SPLIT_STEADY, and every step's observables (update(1) + read-out) are byte-equal.  The controller rows (derivative ring,
   integrals) have no getter of their own: a row written by step k decides the efforts of steps k + 1 .. k + 10, so every scenario
   runs 11 steps past its last command and the platform rows (true pose and twist, FK estimate) are read at the end.
2. The steady instantiation is really taken where the host knows those facts and really left where it does not
   (cdpr_debug_last_variant; cdpr_kernel_name does not change).
3. The steady path against the fp64 oracle on the benchmark's workload."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (1, 63, 64, 65, 130)  # one lane, a ragged tail, a full wave, two workgroups (both parities of the role swap), three
STEPS, TAIL, REFRESH = 35, 11, 10
KERNEL = "cdpr_split_kernel<%d, false>"


def model_of(pkg, n):
    full = pkg.eight_cable_model()
    if n == 8:
        return full
    keep = [0, 1, 2, 3, 4, 5, 6]  # n = 7: a padding cable in the last pair, an odd integral row
    return pkg.Model(full.frame_anchors[keep], full.platform_anchors[keep])


def sine_commands(batch, n, seed):
    """Per-robot sine velocity commands, a new sample every REFRESH world steps (the benchmark's recipe, per cable here)."""
    rng = np.random.default_rng(seed)
    amp, freq, phase = rng.uniform(0.01, 0.05, (batch, n)), rng.uniform(0.05, 0.5, (batch, n)), rng.uniform(0.0, 2 * np.pi, (batch, n))
    return lambda j: (amp * np.sin(2 * np.pi * freq * (j * REFRESH * 1e-3) + phase)).astype(np.float32)


SCENARIOS = [(f"velocity n{n} b{b}", n, b, "velocity") for n in (8, 7) for b in BATCHES] + [
    ("position n8 b130", 8, 130, "position"),
    ("position n7 b65", 7, 65, "position"),
    ("mode change n8 b130", 8, 130, "change"),
    ("mode change n7 b63", 7, 63, "change"),
    ("graph replay n8 b65", 8, 65, "graph"),
]


def run_scenarios():
    """(child process) Every scenario on the library as the environment selects it -> {name: {digest: [per step], variant, kernel}}."""
    import cdpr_simulation_amd as pkg

    out = {}
    for name, n, batch, kind in SCENARIOS:
        eng = pkg.Engine(pkg.Config(model=model_of(pkg, n), batch=batch, stages=3), 0)
        command = sine_commands(batch, n, 100 * n + batch)
        digest, variant, kernel = [], [], set()
        if kind == "graph":  # whole updates (ten launches per captured graph once the Pid call count has saturated) instead of single steps
            for j in range(9):
                eng.set_velocity_command(command(j))
                eng.update(REFRESH)
                digest.append(hashlib.sha256(b"".join(np.ascontiguousarray(x).tobytes() for x in eng.observables())).hexdigest())
                variant.append(eng.last_variant)
                kernel.add(eng.kernel_name)
        else:
            for k in range(STEPS + TAIL):
                if k % REFRESH == 0 and k < STEPS:
                    position = kind == "position" or (kind == "change" and k >= 20)
                    (eng.set_position_command if position else eng.set_velocity_command)(command(k // REFRESH) * (0.1 if position else 1.0))
                eng.update(1)
                digest.append(hashlib.sha256(b"".join(np.ascontiguousarray(x).tobytes() for x in eng.observables())).hexdigest())
                variant.append(eng.last_variant)
                kernel.add(eng.kernel_name)
        final = list(eng.raw_state()) + list(eng.fk_state()) + list(eng.td_state())
        digest.append(hashlib.sha256(b"".join(np.ascontiguousarray(x).tobytes() for x in final)).hexdigest())
        out[name] = {"digest": digest, "variant": variant, "kernel": sorted(kernel)}
        eng.close()
    print(json.dumps(out))


_runs = {}


def child(setting):
    """The scenarios in a fresh process with CDPR_SPLIT_STEADY unset (None) or set; run once per setting."""
    if setting not in _runs:
        env = dict(os.environ)
        env.pop("CDPR_SPLIT_STEADY", None)
        for k in ("CDPR_MAPPING", "CDPR_SPLIT", "CDPR_ONESTEP", "CDPR_LOWREG", "CDPR_PERSIST", "CDPR_CHUNK", "CDPR_NO_GRAPH", "CDPR_LIB"):
            env.pop(k, None)
        if setting is not None:
            env["CDPR_SPLIT_STEADY"] = setting
        env["PYTHONPATH"] = os.pathsep.join([ROOT] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, f"CDPR_SPLIT_STEADY={setting}: the scenario run failed\n{r.stdout[-1000:]}\n{r.stderr[-3000:]}"
        _runs[setting] = json.loads(r.stdout.strip().splitlines()[-1])
    return _runs[setting]


@pytest.mark.parametrize("name,n,batch,kind", SCENARIOS, ids=[s[0] for s in SCENARIOS])
def test_steady_and_generic_controller_waves_are_bit_identical(name, n, batch, kind):
    steady, generic = child(None)[name], child("0")[name]
    assert steady["kernel"] == generic["kernel"] == [KERNEL % n]
    assert not any(generic["variant"]), "CDPR_SPLIT_STEADY=0 must keep every launch on the generic instantiation"
    if kind == "graph":
        assert steady["variant"] == [0] + [1] * 8  # (of each update's last launch; the window is full from world step 12 on, the replays start once the call count has saturated)
    else:
        assert steady["variant"][0] == 0 and all(steady["variant"][12:20]), steady["variant"]  # world step 0, ..., the switch into steady
        if kind == "change":  # the Pid reset of the mode change empties the window: generic until it has refilled, steady again
            assert steady["variant"][20:31] == [0] * 11 and all(steady["variant"][32:]), steady["variant"]
        else:
            assert all(steady["variant"][12:]), steady["variant"]
    moved = [k for k, (a, b) in enumerate(zip(steady["digest"], generic["digest"])) if a != b]
    assert len(steady["digest"]) == len(generic["digest"]) and not moved, f"{name}: observables differ at steps {moved} (the last entry is the final state)"


def stepped(eng, steps):
    """(last_variant, kernel_name) after each of `steps` single-step updates."""
    out = []
    for _ in range(steps):
        eng.update(1)
        out.append((eng.last_variant, eng.kernel_name))
    return out


def test_the_steady_variant_is_taken_and_left(pkg, monkeypatch):
    for k in ("CDPR_SPLIT_STEADY", "CDPR_MAPPING", "CDPR_SPLIT", "CDPR_ONESTEP", "CDPR_LOWREG", "CDPR_PERSIST", "CDPR_CHUNK"):
        monkeypatch.delenv(k, raising=False)
    batch, name = 65, KERNEL % 8
    cmd = sine_commands(batch, 8, 5)(3)
    nbuf = pkg.Config().velocityController.dBufferLength

    def engine(model=None, **kw):
        return pkg.Engine(pkg.Config(model=model or pkg.eight_cable_model(), batch=batch, stages=kw.pop("stages", 3), **kw), 0)

    # a plain run: world step 0 and the filling window (Pid call k - 1 at world step k: full from k = nbuf + 1 on) are generic
    eng = engine()
    eng.set_velocity_command(cmd)
    got = stepped(eng, 30)
    assert all(k == name for _, k in got)
    assert [v for v, _ in got[: nbuf + 1]] == [0] * (nbuf + 1), got
    assert all(v == 1 for v, _ in got[12:]), got
    # Force mode runs no Pid: generic; the velocity command after it resets nothing it did not own but the window was not fed
    eng.set_force_command(np.full((batch, 8), 20.0, np.float32))
    got = stepped(eng, 15)
    assert all(v == 0 and k == name for v, k in got), got
    eng.set_velocity_command(cmd)
    got = stepped(eng, 30)
    assert got[0][0] == 0 and all(v == 1 for v, _ in got[-10:]) and all(k == name for _, k in got), got
    eng.close()
    # publish decimation, the `pid` topic, the travel flags: generic on every step
    limited = pkg.eight_cable_model()
    limited.travel_lower, limited.travel_upper = -0.004, 0.004
    for label, eng in (("publishPeriod", engine(publishPeriod=0.002)), ("pid topic", engine(stages=3 | pkg._abi.STAGE_PID_DEBUG)), ("travel flags", engine(limited))):
        eng.set_velocity_command(cmd)
        got = stepped(eng, 30)
        assert all(v == 0 and k == name for v, k in got), (label, got)
        eng.close()


def test_steady_path_against_the_oracle_on_the_benchmark_workload(pkg, oracle, monkeypatch):
    """128 robots x 8 cables, 200 steps of bench.make_workload (seed 1235, a new command every 10 steps); tolerances of
    tests/parity.py (TOL: the 200-step runs of tests/test_gpu_parity.py use them unchanged)."""
    import bench
    from parity import TOL, compare

    monkeypatch.delenv("CDPR_SPLIT_STEADY", raising=False)
    batch, steps = 128, 200
    model, pose, command, n_cmd = bench.make_workload(pkg, batch, 8, 1235, steps)
    cfg = pkg.Config(model=model, batch=batch, stages=3)
    eng, ora = pkg.Engine(cfg, 0), oracle.OracleSim(cfg.to_struct(), oracle.DERIV_EXACT)
    eng.set_platform_state(pose7=pose)
    ora.set_platform_state(pose7=pose.astype(np.float64))
    for j in range(n_cmd):
        c = command(j)
        eng.set_velocity_command(c), ora.set_velocity_command(c)
        for _ in range(10):
            eng.update(1)
        ora.update(10)
        assert eng.kernel_name == KERNEL % 8 and eng.last_variant == (1 if j >= 1 else 0)  # (of the update's last launch: the window is full from world step 12 on)
        if j % 5 == 4:
            compare(eng, ora, tol=TOL, where=f"after {10 * (j + 1)} steps")
    eng.close()


if __name__ == "__main__":
    run_scenarios()
