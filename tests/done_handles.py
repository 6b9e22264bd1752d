"""The handles the done-rule and environment-view tests run on, and the engine calls both modules make on them: one kind per record
layout of tests/per_robot_kinds.py (fast_n8, general_lean_hot, fp64_hold_n8: per-robot commands), a uniform n = 8 handle with FK + TD, a
uniform n = 4 lane-pair handle, a uniform n = 12 handle.  The rules themselves and their reference are tests/done_rules.py.

B = 130: two full wavefronts and a ragged one, stride 192.
"""
from dataclasses import replace

import numpy as np

import done_rules as dr
import parity
import per_robot_kinds as prk
import robot_histories as ri

B = dr.B
STRIDE = 192
LAYOUTS = prk.LAYOUTS  # fast_n8, general_lean_hot, fp64_hold_n8
UNIFORM = {  # kind: (cables, Config arguments)
    "uniform_n8": (8, dict(stages=3)),
    "uniform_n4_pair": (4, dict(stages=0, mapping=2)),  # _abi.MAP_LANE_PAIR
    "uniform_n12": (12, dict(stages=3)),
}
KINDS = LAYOUTS + list(UNIFORM)


def config_of(pkg, kind, monkeypatch, model_edit=None, **extra):
    """The Config of a handle kind, the routing overrides cleared but for the kind's own; model_edit(model) -> model and extra Config
    arguments for the cases that need limits."""
    parity.clear_overrides(monkeypatch, ("CDPR_NO_GRAPH",))
    if kind in UNIFORM:
        n, kw = UNIFORM[kind]
        per_robot = False
    else:
        n, kw, env, _ = prk.HANDLES[kind]
        per_robot = True
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    model = ri.model_of(pkg, n)
    if model_edit is not None:
        model = model_edit(model)
    return pkg.Config(model=model, batch=B, perRobotCommands=per_robot, **{**kw, **extra})


def put(eng, cfg, pose, twist=None):
    if cfg.precision == 64:
        eng.set_platform_state_f64(pose7=None if pose is None else np.asarray(pose, dtype=np.float64), twist6=None if twist is None else np.asarray(twist, dtype=np.float64))
    else:
        eng.set_platform_state(pose7=pose, twist6=twist)


def getters(eng, cfg):
    """what the verdict is a function of, as the getters hand it out"""
    f64 = cfg.precision == 64
    pose, twist = eng.raw_state_f64() if f64 else eng.raw_state()
    fk, td = bool(cfg.stages & 1), bool(cfg.stages & 2)
    return dict(pose=pose, twist=twist, fk_residual=eng.fk_state()[1] if fk else None, infeasible=eng.td_state()[1] if td else None,
                limit_mask=eng.limit_state(), start=eng.episode_start(), step_count=eng.step_count, f64=f64)


def expect(eng, cfg, rule):
    return dr.done_reference(rule, **getters(eng, cfg))


def assert_verdict(got, want, where):
    for name, g, w in zip(("mask", "reason", "counts"), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), f"{where}: {name} differs from the reference at {np.nonzero(np.asarray(g) != np.asarray(w))[0][:8]}"


def drive(engs, cfg, h, steps):
    """the history of the reset tests on a per-robot handle (modes by index mod 3); one velocity Joy on a uniform handle"""
    if cfg.perRobotCommands:
        ri.play_history(engs, h, steps)
    else:
        for e in engs:
            rc = e.set_velocity_command(h["v"])
            assert rc == 0, f"drive: set_velocity_command returned {rc}"
            e.update(steps)


def limited(model):
    return replace(model, travel_lower=-0.015, travel_upper=0.015)
