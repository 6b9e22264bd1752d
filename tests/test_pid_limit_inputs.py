"""The conditions tests/test_gpu_pid_limits.py relies on, re-established on the fp64 oracle alone (no GPU) with the seeds, limits
and commands of tests/pid_limits.py, so that a change of seed or value cannot quietly empty the GPU module.  They are conditions on
the INPUTS; none of them is measured on a kernel.  Where one fails, the inputs change, not the thresholds.

  sensitivity   every case run twice from start poses one float32 rounding apart: everything finite, effort within 2e-4 N, twist
                within 2e-6 (the tolerances of the GPU comparison are 100x above).
  clamps bite   every case run once more with ONE limit out of reach (iLimit 1e6, cmdLimit 1e6 or effort limit -1): the efforts
                differ by more than 10 x the fp32 effort tolerance on >= 20 % of the robots at two checkpoints or more.  `integral`:
                the integral limit; `command`: the command limit; `command_low_effort`: the effort limit without the tension
                distribution, the command limit with it (its bounds keep the efforts under SetForce's clamp).
  branches      without the tension distribution, under `command`, some effort lies BEYOND cmdLimit (the anti-windup's one
                increment past the clamp, Pid.cpp:181-184) and the same cable comes back under it later; under `integral` no
                effort reaches the shipped 100 (neither the command clamp nor SetForce's is met).
  price         fp32 and fp64 may see cmd cross cmdLimit on different steps; the effort then differs by one anti-windup increment
                iGain dt |target - actual|.  In the `command` variants it stays <= 1e-2 N (half the fp32 effort tolerance) for
                every cable at every step, computed from the oracle's joint states.  (`integral`, whose increments are larger,
                never meets the command clamp: see branches.)
  same kernels  cdpr_plan_kernel names the same kernels for the Config under the variant as for the cell's own Config.
  ladder        every value occurs with both signs, both branches occur, the float32 rule with the rounded threshold classifies
                every float32 near the threshold as the double rule does, float32(eps) rounds up for 0.001 and 0.004 and down for
                0.01; on the oracle a threshold of double(float32(eps)) moves efforts by newtons where float32(eps) rounds up.
  rollout       with cmdLimit out of reach the costs of the rollout case differ by more than 10 x its tolerance in >= 20 % of
                the samples; twin runs agree 100 x better than the tolerance.
"""
import numpy as np
import pytest

import pid_limits as pl
import workspace_poses as wp
from parity import NAMES, TOL, clean_env_fixture, rollout_cost_tol

_BASE = {}
clean_env = clean_env_fixture()


def run(oracle, cfg, variant, pose, cmds, stepwise=False):
    """The script on the oracle.  Returns (observables after every run, per-step records).  A per-step record is (segment index,
    q and qdot before the step, effort after it)."""
    ora = oracle.OracleSim(cfg.to_struct(), oracle.DERIV_EXACT)
    ora.set_platform_state(pose7=pose.astype(np.float64))
    out, steps = [], []
    for j, k in pl.play(variant, cmds, (ora,)):
        if stepwise:
            for _ in range(k):
                q, qd, _ = ora.joint_states()
                ora.update(1)
                steps.append((j, q, qd, ora.joint_states()[2]))
        else:
            ora.update(k)
        out.append(ora.platform_state() + ora.joint_states())
    ora.close()
    return out, steps


def base(pkg, oracle, cell, variant):
    """The case's own run, step by step, computed once and shared (read only)."""
    if (cell, variant) not in _BASE:
        own, cfg, env, pose, cmds = pl.case_inputs(pkg, cell, variant)
        out, steps = run(oracle, cfg, variant, pose, cmds, stepwise=True)
        _BASE[(cell, variant)] = (own, cfg, env, pose, cmds, out, steps)
    return _BASE[(cell, variant)]


def test_variants_change_limits_gains_and_tension_bounds_only(pkg):
    for cell, variant in pl.CASES:
        own, cfg, _, _ = pl.case_config(pkg, cell, variant)
        a, b = own.to_struct(), cfg.to_struct()
        for pa, pb in ((a.velocity_pid, b.velocity_pid), (a.position_pid, b.position_pid)):
            pb.i_limit, pb.cmd_limit, pb.i_gain = pa.i_limit, pa.cmd_limit, pa.i_gain
        b.effort_limit, b.td_f_min, b.td_f_max = a.effort_limit, a.td_f_min, a.td_f_max
        assert bytes(a) == bytes(b), (cell, variant)
        if cfg.stages & 2:  # the middle of the tension bounds inside the effort limit
            s = cfg.to_struct()
            assert 0.5 * (s.td_f_min + s.td_f_max) < s.effort_limit and s.td_f_max <= s.effort_limit, (cell, variant)
    assert len(pl.CASES) == 2 * len(wp.CELLS) + len(pl.LOW_EFFORT_CELLS)


@pytest.mark.parametrize("cell,variant", pl.CASES)
def test_oracle_sensitivity_to_one_rounding_of_the_start_pose(pkg, oracle, clean_env, cell, variant):
    own, cfg, env, pose, cmds, a, _ = base(pkg, oracle, cell, variant)
    seed = pl.case_config(pkg, cell, variant)[3]
    twin = np.nextafter(pose, np.where(np.random.default_rng(seed + 1).random(pose.shape) < 0.5, -np.inf, np.inf).astype(np.float32))
    assert pose.dtype == np.float32 and twin.dtype == np.float32 and (twin != pose).all()
    b, _ = run(oracle, cfg, variant, twin, cmds)
    worst = dict.fromkeys(NAMES, 0.0)
    for sa, sb in zip(a, b):
        for name, x, y in zip(NAMES, sa, sb):
            assert np.isfinite(x).all() and np.isfinite(y).all(), (cell, variant, name)
            worst[name] = max(worst[name], float(np.abs(x - y).max()))
    print(f"sensitivity {cell:12s} {variant:18s} " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst["eff"] <= 2e-4 and worst["twist"] <= 2e-6, (cell, variant, worst)


def limit_under_test(cfg, variant):
    if variant == "integral":
        return "i_limit"
    if variant == "command_low_effort" and not cfg.stages & 2:
        return "effort_limit"
    return "cmd_limit"


@pytest.mark.parametrize("cell,variant", pl.CASES)
def test_each_clamp_matters(pkg, oracle, clean_env, cell, variant):
    own, cfg, env, pose, cmds, a, _ = base(pkg, oracle, cell, variant)
    limit = limit_under_test(cfg, variant)
    b, _ = run(oracle, pl.without(cfg, limit), variant, pose, cmds)
    share = [float((np.abs(sa[4] - sb[4]).max(axis=1) > 10.0 * TOL["eff"]).mean()) for sa, sb in zip(a, b)]
    print(f"without {limit:12s} {cell:12s} {variant:18s} robots whose effort moves by > {10.0 * TOL['eff']:.1f} N per checkpoint: " + " ".join(f"{s:.2f}" for s in share))
    assert sum(s >= 0.2 for s in share) >= 2, (cell, variant, limit, share)


def increments(cfg, variant, cmds, steps):
    """iGain dt |target - actual| of the Pid in charge of every cable at every step, from the oracle's joint states before the
    step [steps, B, n]; dt is the time since that Pid's call before (Pid.cpp:131), 0 at its first call after a reset (no command
    is computed then).  The Pid in charge follows JFC.cpp:59-119: from Load the position Pid with target 0; after a Joy on
    jointVelocities the velocity Pid where abs(target) > epsilon, else the position Pid on the position of the last step at which
    the cable was not held; after a Joy on jointPositions the position Pid; a Joy that changes the mode resets the Pid it selects."""
    script = pl.SCRIPTS[variant]
    gain = {"vel": cfg.velocityController.iGain, "pos": cfg.positionController.iGain}
    eps, dt = cfg.velocityEpsilon, cfg.dt
    shape = steps[0][1].shape
    last = {"vel": np.full(shape, -1), "pos": np.full(shape, -1)}  # step of the Pid's last call, -1: none since its reset
    mode, tgt, last_pos, at, out = "pos", np.zeros(shape), None, -1, []
    for s, (j, q, qd, _) in enumerate(steps):
        while at < j:  # the Joys between the run before and this one
            at += 1
            seg = script[at]
            if seg[0] != "run":
                if mode != seg[0]:
                    last[seg[0]][:] = -1
                mode, tgt = seg[0], (np.float32(seg[2]) * cmds[seg[1]]).astype(np.float64)
        runs_vel = (np.abs(tgt) > eps) if mode == "vel" else np.zeros(shape, dtype=bool)
        last_pos = np.where(runs_vel, q, last_pos) if mode == "vel" else q
        err = np.where(runs_vel, tgt - qd, (last_pos if mode == "vel" else tgt) - q)
        inc = np.zeros(shape)
        for pid, mask in (("vel", runs_vel), ("pos", ~runs_vel)):
            since = np.where(last[pid] < 0, 0, s - last[pid])
            inc = np.where(mask, gain[pid] * dt * since * np.abs(err), inc)
            last[pid] = np.where(mask, s, last[pid])
        out.append(inc)
    return np.array(out)


@pytest.mark.parametrize("cell,variant", pl.CASES)
def test_branch_coverage_and_the_price_of_a_late_decision(pkg, oracle, clean_env, cell, variant):
    own, cfg, env, pose, cmds, out, steps = base(pkg, oracle, cell, variant)
    eff = np.array([s[3] for s in steps])  # [steps, B, n]
    assert len(steps) == sum(seg[1] for seg in pl.SCRIPTS[variant] if seg[0] == "run")
    cmd_limit = pl.VARIANTS[variant]["cmd_limit"]
    if variant == "integral":
        print(f"branches {cell:12s} {variant:18s} largest |effort| {np.abs(eff).max():.3f} N")
        assert np.abs(eff).max() < 100.0, (cell, np.abs(eff).max())
        free, _ = run(oracle, pl.without(cfg, "cmd_limit"), variant, pose, cmds)  # the command clamp is never met: taking it away changes no bit
        assert all(np.array_equal(x, y) for sa, sb in zip(out, free) for x, y in zip(sa, sb)), cell
        return
    inc = increments(cfg, variant, cmds, steps)
    print(f"price    {cell:12s} {variant:18s} largest anti-windup increment {inc.max():.3e} N", end="")
    assert inc.max() <= 0.5 * TOL["eff"], (cell, variant, inc.max())
    if variant == "command" and not cfg.stages & 2:
        beyond = np.abs(eff) > cmd_limit
        assert beyond.any(), cell
        first = beyond.argmax(axis=0)  # per cable: the first step beyond the clamp
        later_below = np.array([[(np.abs(eff[first[r, i]:, r, i]) < cmd_limit).any() for i in range(eff.shape[2])] for r in range(eff.shape[1])])
        print(f"; largest |effort| {np.abs(eff).max():.4f} N against cmdLimit {cmd_limit}, {beyond.any(axis=0).mean():.2f} of the cables beyond it at some step", end="")
        assert (beyond.any(axis=0) & later_below).any(), cell
        assert np.abs(eff).max() < cmd_limit + 0.5 * TOL["eff"]  # one increment, not more
    print()


FIRST, NOT_STEADY = 1, 8  # CDPR_PLAN_* (include/cdpr.h)


@pytest.mark.parametrize("cell,variant", pl.CASES)
def test_variant_keeps_the_cells_kernels(pkg, monkeypatch, clean_env, cell, variant):
    own, cfg, env, _ = pl.case_config(pkg, cell, variant)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for steps in (1, 10):
        for flags in (0, NOT_STEADY, FIRST | NOT_STEADY):
            assert pkg.plan_kernel(cfg, steps, flags) == pkg.plan_kernel(own, steps, flags), (cell, variant, steps, flags)


# ---- the hold ladder -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", pl.LADDER_EPS)
def test_ladder_values_and_the_two_rules(eps):
    vals = pl.ladder_values(eps)
    first, second = pl.ladder_targets(eps, pl.B, 8)
    for t in (first, second):
        for v in vals:  # every value with both signs (+0 and -0 told apart by the sign bit)
            assert ((t == v) & (np.signbit(t) == np.signbit(v))).any(), (eps, v)
        assert pl.velocity_branch(t, eps).any() and (~pl.velocity_branch(t, eps)).any()
    a, b = pl.velocity_branch(first, eps), pl.velocity_branch(second, eps)
    assert (a & ~b).any() and (~a & b).any()  # cables change branch in both directions at the second Joy
    # the two rules agree on the ladder and on every float32 within 64 ulp of the threshold, both signs
    near = [np.float32(eps)]
    for _ in range(64):
        near = [np.nextafter(near[0], np.float32(-np.inf))] + near + [np.nextafter(near[-1], np.float32(np.inf))]
    probe = np.concatenate([vals, np.array(near, dtype=np.float32), -np.array(near, dtype=np.float32)])
    assert np.array_equal(pl.velocity_branch(probe, eps), pl.velocity_branch_float32(probe, eps)), eps
    e_f = float(np.float32(eps))
    assert {0.001: e_f > eps, 0.004: e_f > eps, 0.01: e_f < eps, 0.0: e_f == eps}[eps]
    if e_f > eps:  # the plain cast gets the value ON the threshold wrong
        assert pl.velocity_branch(np.float32(eps), eps) and not np.abs(np.float32(eps)) > np.float32(eps)
    if eps == 0.0:
        assert pl.velocity_branch(pl.SUBNORMAL, eps) and not pl.velocity_branch(np.float32(-0.0), eps)


@pytest.mark.parametrize("eps", pl.LADDER_EPS)
def test_a_threshold_rounded_up_moves_the_oracle_by_newtons(pkg, oracle, eps):
    """The size of what the GPU ladder test looks for: the oracle with velocityEpsilon = double(float32(eps)) against the oracle
    with eps, on the ladder's sequence."""
    first, second = pl.ladder_targets(eps, pl.B, 8)
    pose = pl.start_poses(pkg.eight_cable_model(), np.random.default_rng(pl.LADDER_SEED))
    eff = []
    for e in (eps, float(np.float32(eps))):
        cfg = pkg.Config(model=pkg.eight_cable_model(), batch=pl.B, stages=3, velocityEpsilon=e)
        ora = oracle.OracleSim(cfg.to_struct(), oracle.DERIV_EXACT)
        ora.set_platform_state(pose7=pose.astype(np.float64))
        ora.update(15)
        out = []
        for joy in (first, second):
            ora.set_velocity_command(joy)
            done = 0
            for k in pl.LADDER_CHECKPOINTS:
                ora.update(k - done)
                done = k
                out.append(ora.joint_states()[2])
        eff.append(np.array(out))
        ora.close()
    d = np.abs(eff[0] - eff[1]).max(axis=(1, 2))
    print(f"ladder eps {eps}: a threshold of float32(eps) moves the oracle's efforts by " + " ".join(f"{x:.1f}" for x in d) + " N at the checkpoints")
    if float(np.float32(eps)) > eps:
        assert d.min() > 1.0
    else:
        assert d.max() == 0.0


# ---- the rollout case ----------------------------------------------------------------------------------------------------------
def rollout_costs(oracle, cfg, pose, cmds, ref=None):
    ora = oracle.OracleSim(cfg.to_struct(), oracle.DERIV_EXACT)
    ora.set_platform_state(pose7=pose.astype(np.float64))
    ora.update(pl.ROLLOUT["warm"])
    if ref is None:
        ref = pl.rollout_ref(ora).astype(np.float64)
    cost = ora.rollout_velocity(cmds, ref)
    ora.close()
    return cost, ref


@pytest.mark.parametrize("handle", ["fast", "general"])
def test_rollout_case_meets_the_command_clamp_and_is_benign(pkg, oracle, handle):
    cfg, pose, cmds = pl.rollout_inputs(pkg, handle)
    assert cmds.shape == (pl.ROLLOUT["B"], pl.ROLLOUT["H"], pl.ROLLOUT["S"], pl.ROLLOUT["n"]) and cmds.dtype == np.float32
    cost, ref = rollout_costs(oracle, cfg, pose, cmds)
    tol = rollout_cost_tol(cost, 1e-6)
    free, _ = rollout_costs(oracle, pl.without(cfg, "cmd_limit"), pose, cmds, ref)
    share = float((np.abs(cost - free) > 10.0 * tol).mean())
    twin = np.nextafter(pose, np.where(np.random.default_rng(pl.ROLLOUT["seed"] + 2).random(pose.shape) < 0.5, -np.inf, np.inf).astype(np.float32))
    cost2, _ = rollout_costs(oracle, cfg, twin, cmds, ref)
    print(f"rollout {handle}: tolerance {tol:.3e}, without cmdLimit {share:.2f} of the samples move by > 10 x that, twin runs differ by {np.abs(cost - cost2).max():.3e}")
    assert np.isfinite(cost).all()
    assert share >= 0.2
    assert np.abs(cost - cost2).max() <= 0.01 * tol
    if handle == "general":  # the ladder values are there, in both branches
        vals = pl.ladder_values(pl.ROLLOUT["eps"])
        assert all((cmds == v).any() for v in vals)
        assert 0.2 < np.isin(cmds, vals).mean() < 0.3
