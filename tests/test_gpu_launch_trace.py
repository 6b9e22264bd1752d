"""Which kernel, which instantiation of it and how many launches every call of a fixed script produces, on the smallest handles
that reach every branch of the host's launch chain (csrc/cdpr_engine_launch.hip): one-step and several-steps launches, the
role-split kernel's steady variant, hipGraph replay and its absence, publish decimation, chunked launches, the lane-pair kernels
with the stream kernel inside a schedule, per-robot handles, the general controller path and precision = 64.

Bit-level results cannot see any of this (the kernels of a family compute the same bits); tests/golden/launch_trace.json pins it.
The golden was recorded with the library of the commit before the launch chain was rewritten (`python tests/test_gpu_launch_trace.py`
with CDPR_LIB selecting that build): the test passes on that library and on every later one."""
import contextlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_trace.json")
ROUTING = ("CDPR_SPLIT_STEADY", "CDPR_MAPPING", "CDPR_SPLIT", "CDPR_ONESTEP", "CDPR_LOWREG", "CDPR_PERSIST", "CDPR_CHUNK", "CDPR_NO_GRAPH", "CDPR_PAIR_STREAM",
           "CDPR_GEN_SPLIT", "CDPR_GEN_LEAN", "CDPR_GEN_HOT", "CDPR_F64_SPLIT", "CDPR_F64_RING_LDS", "CDPR_F64_JCACHE")

# name -> (cables, batch, Config fields, environment)
FK_TD = {"stages": 3}
CASES = {
    "split n8 b65": (8, 65, FK_TD, {}),
    "split n8 b65 no graph": (8, 65, FK_TD, {"CDPR_NO_GRAPH": "1"}),
    "split n8 b65 publish 3 ms": (8, 65, dict(FK_TD, publishPeriod=0.003), {}),
    "split n8 b130 chunk 64": (8, 130, FK_TD, {"CDPR_CHUNK": "64"}),
    "pair n4 b65": (4, 65, {}, {}),
    "per-robot n8 b130": (8, 130, dict(FK_TD, perRobotCommands=True), {}),
    "general n4 b65": (4, 65, {"velocityEpsilon": 0.001}, {}),
    "general n8 b65": (8, 65, dict(FK_TD, velocityEpsilon=0.001), {}),
    "general n8 b65 publish 3 ms": (8, 65, dict(FK_TD, velocityEpsilon=0.001, publishPeriod=0.003), {}),
    "f64 n8 b65": (8, 65, dict(FK_TD, precision=64), {}),
    "f64 hold n8 b65": (8, 65, dict(FK_TD, precision=64, velocityEpsilon=0.001), {}),
}


@contextlib.contextmanager
def routing(env):
    """The routing overrides cleared, then only what the case names; the caller's environment back afterwards."""
    saved = {k: os.environ.get(k) for k in ROUTING}
    try:
        for k in ROUTING:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def trace(pkg, name):
    """[step_count, kernel_name, last_variant, launches of the call] after every call of the script."""
    n, batch, fields, env = CASES[name]
    rng = np.random.default_rng(17)
    velocity = rng.uniform(-0.02, 0.02, (batch, n)).astype(np.float32)
    position = rng.uniform(-0.003, 0.003, (batch, n)).astype(np.float32)
    force = (7.0 + rng.uniform(-1.0, 1.0, (batch, n))).astype(np.float32)
    schedule = rng.uniform(-0.02, 0.02, (4, batch, n)).astype(np.float32)
    with routing(env):
        cfg = pkg.Config(model=pkg.eight_cable_model() if n == 8 else pkg.cube_model(), batch=batch, **fields)
        eng = pkg.Engine(cfg, 0)
        d_schedule = eng.device_upload(schedule)
        script = [
            lambda: eng.update(1),
            lambda: eng.update(1),
            lambda: eng.set_velocity_command(velocity),
            lambda: eng.update(12),
            lambda: eng.update(70),  # the Pid call count passes its saturation point (kCallSat = 64)
            lambda: eng.update(25),
            lambda: eng.set_position_command(position),
            lambda: eng.update(3),
            lambda: eng.update(14, 5),
        ]
        if cfg.publishPeriod == 0.0:
            script.append(lambda: eng.update_record(6, 3))
        script += [
            lambda: eng.set_force_command(force),
            lambda: eng.update(11),
            lambda: eng.update_scheduled(20, 5, d_schedule, kind="velocity"),
        ]
        out = []
        for call in script:
            eng.profile_begin()
            call()
            _, launches = eng.profile_end()
            out.append([eng.step_count, eng.kernel_name, eng.last_variant, int(launches)])
        assert np.isfinite(eng.platform_state()[0]).all()
        eng.device_free(d_schedule)
        eng.close()
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_every_call_takes_the_recorded_kernel_variant_and_launch_count(pkg, name):
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = trace(pkg, name)
    for k, (g, w) in enumerate(zip(got, golden[name])):
        assert g == w, f"{name}: call {k} of the script gave {g}, recorded {w}"
    assert len(got) == len(golden[name])


if __name__ == "__main__":  # record the golden (or the file named) with the library CDPR_LIB selects
    sys.path.insert(0, ROOT)
    import cdpr_simulation_amd

    with open(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, "w") as f:
        json.dump({name: trace(cdpr_simulation_amd, name) for name in CASES}, f, indent=1)
        f.write("\n")
