"""The launch forms behind reset, copy and resample of robots, the CPU side: the oracle-side conditions that
tests/test_gpu_launch_forms_after_robot_ops.py rests on (the script and the forms: tests/launch_forms.py).

  1. benign and history independent, on the nine kinds of per_robot_kinds.ALL: two oracles with the histories (seed, shift) = (1, 0)
     and (2, 1) - other start poses, other commands, every robot in another mode - get the reset recipe with the same mask and poses and
     then the after-script (13 steps, masked velocity Joy + 30, masked position Joy + 25, masked force Joy + 12).  Everything stays
     finite, the reset robots' pose, twist, q, qd and effort are EQUAL (difference 0.0) after every one of the 80 steps while the other
     robots differ, and the effort reaches the clamp (100 N; asserted on the `_long` kinds, measured on all nine): no gentle script.
  2. sensitivity, on n8_fk_td, n8_fk_td_hold and n4: the HALF recipe (pose and twist rows only, the Pids keep their past: what a launch
     form that ignored the reset's call count would resemble) against the full one.  Measured with the inputs below: every reset
     robot's effort differs by at least 0.61 N one step, 1.13 N five and 1.42 N thirteen steps after the reset (TOL eff: 2e-2 N); the
     rollout costs of the reset robots differ by a median of 6.5 / 10.5 / 11.1 times the rollout tolerance at +5 and 37 / 40 / 47 times
     at +13, but only 0.6 to 1.6 times at +1 - which is why the GPU module compares rollouts with the oracle 5 and 13 steps after the
     op.  Asserted: every reset robot's effort differs by at least 10 x TOL eff at +1, +5 and +13; at least half of the reset robots'
     cost rows differ by at least 3 x the rollout tolerance at +5 and at +13.
"""
import numpy as np
import pytest

import launch_forms as lf
import robot_histories as ri
from parity import NAMES, TOL
from per_robot_kinds import ALL, clean_env, config_of  # noqa: F401  (clean_env: autouse here too)

B = ri.B


def test_the_kinds():
    assert len(ALL) == 9 and lf.KINDS == ALL + ["general_one_wave"] and set(lf.GENERAL) <= set(lf.KINDS)
    assert [lf.steps_of_the_last_launch("fused3", k) for k in (37, 13, 30, 25, 12)] == [1, 1, 3, 1, 3]
    assert [lf.steps_of_the_last_launch("rec", k) for k in (37, 13, 30, 25, 12)] == [7, 3, 10, 5, 2]
    assert lf.steps_of_the_last_launch("long", 37) == 37 and lf.steps_of_the_last_launch("one", 37) == 1


@pytest.mark.parametrize("kind", ALL)
def test_the_after_script_is_benign_and_the_reset_robots_forget(pkg, oracle, monkeypatch, kind):
    cfg = config_of(pkg, kind, monkeypatch)
    players = [lf.Player(oracle.OracleSim(cfg.to_struct(), oracle.DERIV_EXACT), "oracle", cfg) for _ in range(2)]
    for p, (seed, shift) in zip(players, ((1, 0), (2, 1))):
        h = ri.history_inputs(cfg.model, seed, shift)
        p.sim.set_platform_state(pose7=h["pose"].astype(np.float64))
        lf.play_history([p], h)
    mask = ri.reset_mask()
    m = mask.astype(bool)
    a = lf.after_inputs(cfg.model, 13)
    for p in players:
        ri.oracle_reset(p.sim, mask, a["pose"])
        p.steps.clear()
    labels = []
    lf.play_after(players, a, lambda label, k: labels.append(label))
    assert len(labels) == 4 and len(players[0].steps) == len(players[1].steps) == 80
    apart, peak = [], 0.0
    for step, (xs, ys) in enumerate(zip(players[0].steps, players[1].steps)):
        for quantity, x, y in zip(NAMES, xs, ys):
            assert np.isfinite(x).all() and np.isfinite(y).all(), (kind, step, quantity)
            assert np.array_equal(x[m], y[m]), f"{kind}, step {step + 1}: {quantity} of the reset robots depends on their history (max difference {np.abs(x[m] - y[m]).max():.3e})"
        apart.append(float(np.abs(xs[0][~m] - ys[0][~m]).max()))
        peak = max(peak, float(np.abs(xs[4]).max()), float(np.abs(ys[4]).max()))
    assert min(apart) > 1e-3, f"{kind}: the two histories do not tell the other robots apart ({min(apart)})"
    print(f"launch forms, {kind}: peak |effort| over the after-script {peak:.3f} N")
    if kind.endswith("_long"):
        assert peak == 100.0, f"{kind}: the after-script does not reach the effort clamp ({peak})"
    for p in players:
        p.close()


@pytest.mark.parametrize("name", list(ri.CONFIGS))
def test_the_script_tells_a_reset_that_forgets_the_controller(pkg, oracle, name):
    n, kw = ri.CONFIGS[name]
    model = ri.model_of(pkg, n)
    cfg = pkg.Config(model=model, batch=B, perRobotCommands=True, **kw)
    general = "velocityEpsilon" in kw
    full, half = (oracle.OracleSim(cfg.to_struct(), oracle.DERIV_EXACT) for _ in range(2))
    h = ri.history_inputs(model, 1)
    mask = ri.reset_mask()
    m = mask.astype(bool)
    a = lf.after_inputs(model, 13)
    for s in (full, half):
        s.set_platform_state(pose7=h["pose"].astype(np.float64))
        ri.play_history([s], h)
    ri.oracle_reset(full, mask, a["pose"])
    lf.half_reset(half, mask, a["pose"])
    roll = lf.rollout_inputs(cfg, a["pose"], 17)
    assert roll["cmds"].shape == (B, 14, lf.SAMPLES, n)
    at = 0
    for steps in (1, 4, 8):
        full.update(steps), half.update(steps)
        at += steps
        per_robot = np.abs(full.joint_states()[2] - half.joint_states()[2]).max(axis=1)
        print(f"launch forms, {name}, +{at}: effort of the reset robots, full against half recipe: min {per_robot[m].min():.3f} N")
        assert per_robot[m].min() >= 10 * TOL["eff"], f"{name}, +{at}: a reset robot's effort does not tell the half recipe ({per_robot[m].min():.3e} N)"
        assert not per_robot[~m].any()  # (the robots outside the mask: the same oracle)
        oc, hc = (s.rollout_velocity(roll["cmds"], roll["ref"].astype(np.float64)) for s in (full, half))
        ratio = np.abs(oc - hc).max(axis=1) / lf.rollout_tolerance(cfg, general, oc)
        print(f"launch forms, {name}, +{at}: rollout cost of the reset robots, full against half recipe: median {np.median(ratio[m]):.1f} x the tolerance")
        if at > 1:
            assert 2 * int((ratio[m] >= 3.0).sum()) >= int(m.sum()), f"{name}, +{at}: fewer than half of the reset robots' cost rows tell the half recipe (median {np.median(ratio[m]):.2f} x tolerance)"
    full.close(), half.close()
