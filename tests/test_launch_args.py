"""The bytes a kernel receives, pinned without a GPU: cdpr_debug_launch_args (csrc/cdpr_engine.hip over csrc/cdpr_launch_args.hpp) writes the
argument record(s) a launch copies for a configuration and a mode - pointers null, the per-launch fields zero, the path's uploaded tables
appended - and every cell of
  cables {1, 4, 7, 8, 12} x the six handle kinds of csrc/dispatch_check.hip x per-robot commands {0, 1} x precision {32, 64}
  x mode {Force, Position, Velocity}, batch 65
is pinned to the SHA-256 of those bytes in tests/golden/launch_args.json (a refused cell: to its return code).  The golden was recorded
from the fillers of the commit named in its `provenance`, before the arguments moved into one header: a digest that changes is a byte
of some kernel's arguments that changed.  Regenerate (after a deliberate change of an argument): python tests/test_launch_args.py --write."""
import ctypes as C
import hashlib
import json
import os
import sys

from parity import ROUTING_OVERRIDES, clean_env_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_args.json")
CABLES = (1, 4, 7, 8, 12)
KINDS = ("plain", "hold", "long", "hold+long", "physics", "cascade")
MODES = ("force", "position", "velocity")  # JFC.h:35-37: 0, 1, 2

clean_env = clean_env_fixture("CDPR_SPLIT_SWAP")


def config(abi, n, kind, per_robot, precision):
    """dispatch_check.hip's base_config and its handle kinds, with values that make every field of the arguments speak: distinct gains per
    Pid, an i_gain of 0 ("long"), a negative i_limit and a negative cmd_limit ("physics": the |limit| rules, Pid.cpp:70-73)."""
    c = abi.ConfigStruct()
    c.abi_version, c.n_cables, c.batch, c.dt, c.mass = abi.ABI_VERSION, n, 65, 1e-3, 1.25
    c.inertia[0], c.inertia[1], c.inertia[2], c.inertia[3] = 0.1, 0.12, 0.15, 0.01
    c.gravity[2] = -9.81
    c.home_pose[2], c.home_pose[6] = 0.5, 1.0
    for i in range(n):
        c.cable_ref_length[i] = 1.0 + 0.01 * i
        c.frame_anchor[i][0], c.frame_anchor[i][1], c.frame_anchor[i][2] = 1.0 + i, -1.0 + 0.5 * i, 2.0
        c.platform_anchor[i][0], c.platform_anchor[i][1], c.platform_anchor[i][2] = 0.1 * i, 0.05, -0.1
    c.joint_damping, c.effort_limit, c.velocity_limit, c.unilateral_cables = 0.3, 150.0, 2.5, 1
    for k, p in enumerate((c.velocity_pid, c.position_pid)):
        p.forward_gain, p.p_gain, p.i_gain, p.d_gain = 0.1 + k, 40.0 + k, 3.0 + k, 0.7 + k
        p.d_degree, p.d_buffer_length, p.i_limit, p.cmd_limit = 2, 11, 1.0 + k, 100.0 + k
    c.velocity_epsilon, c.precision, c.per_robot_commands = -1.0, precision, per_robot
    c.stages = 3 if n >= 6 else 0  # FK + TD from six cables on
    c.fk_max_iterations, c.fk_lambda, c.fk_tolerance, c.td_f_min, c.td_f_max = 4, 1e-6, 1e-9, 5.0, 100.0
    if kind in ("hold", "hold+long"):
        c.velocity_epsilon = 0.001
    if kind == "long":
        c.velocity_pid.d_buffer_length = c.position_pid.d_buffer_length = 21
        c.position_pid.i_gain = 0.0
    if kind == "hold+long":
        c.velocity_pid.d_buffer_length = 21
    if kind == "physics":
        c.travel_lower, c.travel_upper, c.travel_stop, c.leg_inertia = -0.01, 0.01, 2, 0.004
        c.velocity_pid.i_limit, c.position_pid.cmd_limit = -0.7, -50.0
    if kind == "cascade":
        f = c.velocity_pid.p_filter
        f.cascade, f.rel_cutoff, f.quality = 1, 0.1, 0.7
        c.leg_inertia = 0.004
    return c


def cells(abi):
    for n in CABLES:
        for kind in KINDS:
            for per_robot in (0, 1):
                for precision in (32, 64):
                    for mode, name in enumerate(MODES):
                        yield f"n{n} {kind} pr{per_robot} fp{precision} {name}", config(abi, n, kind, per_robot, precision), mode


def digest(cfg, mode):
    """SHA-256 of the argument bytes, or "rc <code>" where plan_kernels refuses the configuration."""
    from cdpr_simulation_amd._native import lib

    size = lib().cdpr_debug_launch_args(C.byref(cfg), mode, None, 0)
    if size <= 0:
        return f"rc {size}"
    buf = C.create_string_buffer(size)
    assert lib().cdpr_debug_launch_args(C.byref(cfg), mode, buf, size) == size
    return hashlib.sha256(buf.raw).hexdigest()


def table(abi):
    return {key: digest(cfg, mode) for key, cfg, mode in cells(abi)}


def test_launch_arguments_are_the_recorded_bytes(pkg, clean_env):
    got = table(pkg._abi)
    want = json.load(open(GOLDEN))["cells"]
    assert set(got) == set(want)
    diff = sorted(k for k in got if got[k] != want[k])
    assert not diff, f"{len(diff)} of {len(got)} cells changed, e.g. {diff[:8]}"
    served = [k for k, v in got.items() if not v.startswith("rc ")]
    assert len(served) >= 200  # (the matrix is mostly served: a table of refusals would pin nothing)
    # ... and says something: the mode, the kind and the Pid limits reach the bytes
    assert got["n8 plain pr0 fp32 position"] != got["n8 plain pr0 fp32 velocity"] != got["n8 plain pr0 fp32 force"]
    assert got["n8 plain pr0 fp64 position"] != got["n8 plain pr0 fp64 velocity"]
    assert len({got[f"n8 {kind} pr0 fp32 velocity"] for kind in KINDS}) == len(KINDS)


def test_the_limit_rules_reach_the_bytes(pkg, clean_env):
    """|i_limit| and |cmd_limit| (Pid.cpp:70-73): the sign of a limit changes no byte, its magnitude does - on every record layout."""
    abi = pkg._abi
    for kind in ("physics", "hold"):
        for per_robot in (0, 1):
            for precision in (32, 64):
                for mode in range(3):
                    base = config(abi, 8, kind, per_robot, precision)
                    want = digest(base, mode)
                    if want.startswith("rc "):
                        continue
                    for pid in ("velocity_pid", "position_pid"):
                        for limit in ("i_limit", "cmd_limit"):
                            c = config(abi, 8, kind, per_robot, precision)
                            setattr(getattr(c, pid), limit, -getattr(getattr(c, pid), limit))
                            assert digest(c, mode) == want, (kind, per_robot, precision, mode, pid, limit)
                    c = config(abi, 8, kind, per_robot, precision)
                    c.velocity_pid.i_limit *= 2.0
                    c.position_pid.i_limit *= 2.0
                    assert digest(c, mode) != want, (kind, per_robot, precision, mode)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import cdpr_simulation_amd as pkg_

    for k_ in ROUTING_OVERRIDES + ("CDPR_SPLIT_SWAP",):
        os.environ.pop(k_, None)
    if "--write" in sys.argv:
        provenance = sys.argv[sys.argv.index("--write") + 1] if len(sys.argv) > sys.argv.index("--write") + 1 else json.load(open(GOLDEN))["provenance"]
        json.dump({"provenance": provenance, "cells": table(pkg_._abi)}, open(GOLDEN, "w"), indent=0, sort_keys=True)
        print("wrote", GOLDEN)
    else:
        print(json.dumps(table(pkg_._abi), indent=0, sort_keys=True))
