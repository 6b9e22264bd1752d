"""Every launch form behind reset_robots, copy_robots and resample: the kernels that write per-robot controller records for chosen
robots (model_reset, take_over: csrc/cdpr_robot_records.hpp) against every step kernel family that READS those records - not only the
one-step launches the modules of those calls use, but several steps per launch (update(k, spl), update_record, the per-robot schedule
chain), the captured graph of ten fused launches and the MPC rollout.  Forms, script and rollout inputs: tests/launch_forms.py; the
oracle-side conditions (history independence of the recipe, the script's sensitivity to a reset that forgets the controller):
tests/test_launch_form_inputs.py.  Tolerances: TOL and TOL64 of tests/parity.py, the suite's rollout tolerances.

Kinds: per_robot_kinds.ALL and general_one_wave (the one-wave general kernel on 11-sample windows, whose fused launches really are
several steps per launch).  Ops: reset_robots(reset_mask, fresh poses), copy_robots(copy_map), on the general kinds copy_robots(aligned_map)
too.  Every engine plays the 37-step HISTORY in its own form, so the op acts on records the multi-step kernels wrote.

  1  forms against the oracle at the four checkpoints of the after-script (reset: the recipe, copy: the twin from birth); form rec:
     every recorded step against the oracle stepped one step at a time, the record's last image against the getters.
  2  forms against form `one`, to the bit.  Control: every_getter at the end of the history, before any reset or copy kernel has run.
     Where the control is bit equal the form must stay bit equal to `one` at every checkpoint after the op, on every robot, and every
     recorded step must be what `one` published at that step.  NOT_BIT_EQUAL names the (kind, form) whose control is not bit equal:
     those are held to the oracle only (1).
  3  the kernels ran: kernel_name after every segment is plan_kernel(cfg, steps of the segment's last launch); the register-resident
     kinds' several-steps launches name PR> without SINGLE, general_one_wave and general_long the several-steps cdpr_gen_step_kernel.
  4  a reset robot forgets, on the engine itself: two engines with the histories (1, 0) and (2, 1), the same reset, the same
     after-script, in forms one, fused10, long and sched; the reset robots' rows of every_getter are equal to the bit off the general
     path (within TOL on it, exactness printed) at every checkpoint while the other robots differ.  The two histories leave different
     errors in the derivative ring's stale slots.
  5  the MPC rollout right after the op (every getter untouched to the bit; copy: cost of a destination = cost of its source with
     twinned inputs; reset: the two histories' cost rows of the reset robots agree) and 5 and 13 one-step updates later against
     oracle.rollout_velocity; a fused10 segment behind it against the oracle.  And with no op at all: the rollout at the end of the
     history against the oracle, by the mode a robot is in.
  6  resample_device, then a fused10 segment and a rollout: bit equal to an engine that got copy_robots(the downloaded map).

Measured on MI355X (136 cases, 7 s):
  control of 2: bit equal to one-step launches on EVERY kind and form (10 kinds x fused10, fused3, rec, long, sched): NOT_BIT_EQUAL is
     empty, no form is held to the oracle only; behind every op every form stayed bit equal at every checkpoint and recorded step.
  4: the reset robots of the two histories were equal to the bit at every checkpoint on every kind, the general path included.
  worst error against the oracle over the ops and checkpoints - the same for every form of a kind, since the forms are bit equal;
  in brackets the worst over every recorded step of form rec - and the rollout's worst error in units of its tolerance:
     fast_n8            pose 2.3e-07  twist 2.1e-05  q 1.9e-07  qd 1.7e-05  eff 2.9e-03 (3.7e-03)   rollout 0.022
     fast_n4            pose 1.8e-07  twist 8.6e-06  q 1.6e-07  qd 7.6e-06  eff 2.9e-03 (3.7e-03)   rollout 0.011
     fast_n7            pose 2.2e-07  twist 1.0e-05  q 2.1e-07  qd 9.7e-06  eff 2.7e-03 (3.6e-03)   rollout 0.010
     general_n8, general_lean_hot, general_one_wave
                        pose 2.3e-07  twist 2.1e-05  q 2.2e-07  qd 1.6e-05  eff 3.5e-03 (3.7e-03)   rollout 0.022
     general_long       pose 4.9e-07  twist 8.9e-05  q 4.1e-07  qd 9.6e-05  eff 4.5e-03 (6.6e-03)   rollout 0.026
     fp64_n8            pose 7.2e-16  twist 5.1e-14  q 6.7e-16  qd 4.2e-14  eff 9.0e-12 (1.0e-11)   rollout 0.153
     fp64_hold_n8       pose 7.2e-16  twist 6.2e-14  q 6.7e-16  qd 4.3e-14  eff 8.4e-12 (9.6e-12)   rollout 0.169
     fp64_hold_long     pose 3.2e-15  twist 2.1e-13  q 2.7e-15  qd 2.0e-13  eff 2.2e-11 (2.2e-11)   rollout 0.133
  What 5 found: the register-resident per-robot rollout (cdpr_step_kernel<..., ROLLOUT, PR>) took the trajectories of a robot in
  Force mode as open-loop FORCES - the lane's velocity Pid was reset for the Joy, but the force test still read the handle's mode
  byte.  Costs were off by 35 (fast_n4) to 350 (fast_n8) times the tolerance on those robots and by at most 0.021 on the others, right
  after a copy and five steps after a reset alike; the rollout tests before this module had no robot in Force mode on such a handle.
  Fixed in the kernel (the lane's copy of the mode becomes Velocity); every other kernel's code is unchanged.

B = 130: two full wavefronts and a ragged one, stride 192.
"""
import numpy as np
import pytest

import copy_robots as cr
import launch_forms as lf
import parity
import resample_oracle as ro
import robot_histories as ri
from parity import NAMES, TOL, TOL64, equal_rows, every_getter, observed
from launch_forms import Scenario
from per_robot_kinds import LAYOUTS, clean_env  # noqa: F401  (clean_env: autouse here too)

pytestmark = pytest.mark.gpu

B = ri.B
KINDS, GENERAL, FORMS = lf.KINDS, lf.GENERAL, lf.FORMS
FAST = ["fast_n8", "fast_n4", "fast_n7"]
CASES = [(kind, op) for kind in KINDS for op in ["reset", "copy"] + (["copy_aligned"] if kind in GENERAL else [])]
EVERY = slice(None)
# (kind, form) whose control - the end of the history against form `one`, before any op - is not bit equal: held to the oracle only
NOT_BIT_EQUAL = set()
MINIMUM = [(kind, form) for kind in ("fast_n8", "fast_n4", "fast_n7", "fp64_n8", "fp64_hold_n8", "fp64_hold_long") for form in ("fused10", "rec", "long")]
assert not NOT_BIT_EQUAL & set(MINIMUM)


def against_the_oracle(eng, ora, cfg, where):
    parity.against_the_oracle(eng, ora, cfg.precision == 64, where, printed="copy_robots")  # (as tests/test_gpu_copy_robots.py)


def tol_of(cfg):
    return TOL64 if cfg.precision == 64 else TOL


def errors(got, want, rows=EVERY):
    return {name: float(np.abs(g[rows] - w[rows]).max()) for name, g, w in zip(NAMES, got, want)}


def within(worst, tol, where):
    print(f"launch forms, {where}: " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for name in NAMES:
        assert np.isfinite(worst[name]) and worst[name] <= tol[name], f"{where}: {name} differs from the oracle by {worst[name]:.3e} (tolerance {tol[name]:.1e})"


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,op", CASES)
def test_forms_against_the_oracle(pkg, oracle, monkeypatch, kind, op):
    sc = Scenario(pkg, oracle, monkeypatch, kind, op, FORMS, 301)
    cfg, tol = sc.cfg, tol_of(sc.cfg)
    want = observed(sc.ora.sim, cfg.precision == 64)
    for p in sc.players:  # (the twin from birth holds the plain history on every robot that is no destination)
        within(errors(observed(p.sim, cfg.precision == 64), want, EVERY if op == "reset" else ~sc.touched), tol, f"{kind}, {op}, {p.form}, the end of the history")
    sc.apply()
    worst = {p.form: dict.fromkeys(NAMES, 0.0) for p in sc.players}

    def check(label, k):
        want = observed(sc.ora.sim, cfg.precision == 64)
        for p in sc.players:
            got = observed(p.sim, cfg.precision == 64)
            for name, v in errors(got, want).items():
                worst[p.form][name] = max(worst[p.form][name], v)
            against_the_oracle(p.sim, sc.ora.sim, cfg, f"{kind}, {op}, {p.form}, {label}")
            if p.form == "rec":
                for key, x in zip(("pose", "twist", "position", "velocity", "effort"), got):
                    assert np.array_equal(p.record[key][-1], x), f"{kind}, {op}, {label}: the record's last step is not the published one ({key})"

    sc.play_after(check)
    rec = next(p for p in sc.players if p.form == "rec")
    assert len(rec.steps) == len(sc.ora.steps) == 80
    rec_worst = dict.fromkeys(NAMES, 0.0)
    for got, want in zip(rec.steps, sc.ora.steps):
        for name, v in errors(got, want).items():
            rec_worst[name] = max(rec_worst[name], v)
    for form, w in worst.items():
        print(f"launch forms WORST {kind} {op} {form}: " + "  ".join(f"{k} {v:.2e}" for k, v in w.items()))
    within(rec_worst, tol, f"WORST {kind} {op} rec, every recorded step")
    sc.close()


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,op", CASES)
def test_forms_against_one_step_launches_to_the_bit(pkg, monkeypatch, kind, op):
    sc = Scenario(pkg, None, monkeypatch, kind, op, FORMS, 311)
    cfg = sc.cfg
    one, others = sc.players[0], sc.players[1:]
    assert one.form == "one"
    base = every_getter(one.sim, cfg, pkg)
    control = {p.form: equal_rows(every_getter(p.sim, cfg, pkg), base, EVERY, EVERY) for p in others}
    print(f"launch forms CONTROL {kind} {op}: " + "  ".join(f"{form} {'equal' if same else 'NOT EQUAL'}" for form, same in control.items()))
    known = {form for form in control if (kind, form) in NOT_BIT_EQUAL}
    surprises = [form for form, same in control.items() if not same and form not in known]
    assert not surprises, f"{kind}: the control (end of the history, no op yet) is not bit equal to one-step launches in the forms {surprises}"
    sc.apply()
    parted = []
    right_after = every_getter(one.sim, cfg, pkg)
    for p in others:
        if control[p.form] and not equal_rows(every_getter(p.sim, cfg, pkg), right_after, EVERY, EVERY):
            parted.append((p.form, f"right after the {op}"))

    def check(label, k):
        base = every_getter(one.sim, cfg, pkg)
        for p in others:
            if not control[p.form]:
                continue
            got = every_getter(p.sim, cfg, pkg)
            if not equal_rows(got, base, EVERY, EVERY):
                rows = "touched and untouched" if not equal_rows(got, base, ~sc.touched, ~sc.touched) else "touched only"
                parted.append((p.form, label, rows))

    sc.play_after(check)
    rec = next(p for p in others if p.form == "rec")
    assert len(rec.steps) == len(one.steps) == 80
    if control["rec"]:
        for j, (got, want) in enumerate(zip(rec.steps, one.steps)):
            if not all(np.array_equal(x, y) for x, y in zip(got, want)):
                parted.append(("rec", f"recorded step {j + 1} after the {op}", "touched and untouched" if not equal_rows(got, want, ~sc.touched, ~sc.touched) else "touched only"))
                break
    print(f"launch forms BITS {kind} {op}: " + (f"parted {parted}" if parted else "every form with an equal control stayed equal to one-step launches"))
    assert not parted, f"{kind}, {op}: forms whose control was bit equal to one-step launches parted from them: {parted}"
    sc.close()


def test_the_minimum_of_the_control():
    """what the control must cover at least: no (kind, form) of MINIMUM may be excused"""
    assert not NOT_BIT_EQUAL & set(MINIMUM) and len(MINIMUM) == 18


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_the_kernels_ran(pkg, monkeypatch, kind):
    sc = Scenario(pkg, None, monkeypatch, kind, "reset", FORMS, 321)
    cfg = sc.cfg
    sc.apply()
    sc.play_after(lambda label, k: None)
    for p in sc.players:
        assert len(p.launches) == 5
        for last, name in p.launches:
            assert name == pkg.plan_kernel(cfg, last), (kind, p.form, last, name)
        several = [name for last, name in p.launches if last > 1]
        assert (p.form == "one") == (not several), (kind, p.form)
        for name in several:
            if kind in FAST:
                assert "cdpr_step_kernel<" in name and name.endswith("PR>") and "SINGLE" not in name, (kind, p.form, name)
            if kind in ("general_one_wave", "general_long"):
                assert "cdpr_gen_step_kernel<8," in name and "SINGLE" not in name and "ROLLOUT" not in name, (kind, p.form, name)
            if cfg.precision == 64:
                assert "cdpr_step_kernel_f64<8, PR" in name, (kind, p.form, name)
    sc.close()


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["one", "fused10", "long", "sched"])
@pytest.mark.parametrize("kind", KINDS)
def test_a_reset_robot_forgets(pkg, monkeypatch, kind, form):
    pair = [Scenario(pkg, None, monkeypatch, kind, "reset", [form], seed, shift) for seed, shift in ((1, 0), (2, 1))]
    cfg, m = pair[0].cfg, pair[0].touched
    tol = tol_of(cfg)
    (x,), (y,) = pair[0].players, pair[1].players
    assert not equal_rows(every_getter(x.sim, cfg, pkg), every_getter(y.sim, cfg, pkg), m, m)  # (before the reset they differ)
    for sc in pair:
        sc.apply()
    exact, apart = [], []

    def check(label):
        gx, gy = every_getter(x.sim, cfg, pkg), every_getter(y.sim, cfg, pkg)
        exact.append(equal_rows(gx, gy, m, m))
        if kind not in GENERAL:
            assert exact[-1], f"{kind}, {form}, {label}: a reset robot remembers its history"
        within(errors(observed(x.sim, cfg.precision == 64), observed(y.sim, cfg.precision == 64), m), tol, f"{kind}, {form}, {label}, the reset robots of two histories")
        apart.append(float(np.abs(gx[0][~m] - gy[0][~m]).max()))

    check("right after the reset")
    for label, joy, key, k in lf.SEGMENTS:  # (both engines, segment by segment)
        for p in (x, y):
            p.run(k) if joy is None else p.joy(joy, pair[0].a[key], pair[0].a[key + "_mask"], k)
        check(label)
    print(f"launch forms FORGETS {kind} {form}: the reset robots of the two histories equal to the bit at the checkpoints: {exact}")
    assert min(apart) > 1e-3, f"{kind}, {form}: the two histories do not tell the other robots apart ({apart})"
    for sc in pair:
        sc.close()


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,op", CASES)
def test_rollout_behind_the_op(pkg, oracle, monkeypatch, kind, op):
    sc = Scenario(pkg, oracle, monkeypatch, kind, op, ["fused10"], 1)
    cfg, m, general = sc.cfg, sc.touched, kind in GENERAL
    other = Scenario(pkg, None, monkeypatch, kind, op, ["fused10"], 2, 1) if op == "reset" else None
    eng, ora = sc.players[0].sim, sc.ora.sim
    roll = lf.rollout_inputs(cfg, sc.a["pose"], 331)
    if op != "reset":
        roll = cr.twin_rows(roll, sc.source)
    cmds, ref = roll["cmds"], roll["ref"]
    H = cmds.shape[1]
    assert H == (35 if kind.endswith("_long") else 14) and cmds.shape[2] == lf.SAMPLES
    sc.apply()
    if other:
        other.apply()

    def rollout(e, where):
        before = every_getter(e, cfg, pkg)
        steps = e.step_count
        cost = e.rollout_velocity(cmds, ref)
        assert e.kernel_name == pkg.plan_kernel(cfg, H, flags=pkg._abi.PLAN_ROLLOUT), (kind, e.kernel_name)
        assert cost.shape == (B, lf.SAMPLES) and np.isfinite(cost).all(), where
        assert e.step_count == steps and equal_rows(every_getter(e, cfg, pkg), before, EVERY, EVERY), f"{where}: the rollout changed what a getter returns"
        return cost

    def against(cost, where):
        oc = ora.rollout_velocity(cmds, ref.astype(np.float64))
        err, bound = float(np.abs(cost - oc).max()), lf.rollout_tolerance(cfg, general, oc)
        print(f"launch forms ROLLOUT {where}: max |cost - oracle| {err:.3e} = {err / bound:.3f} x the tolerance")
        assert err <= bound, f"{where}: the rollout's costs differ from the oracle's by {err:.3e} (tolerance {bound:.3e})"
        return oc

    # right after the op
    where = f"{kind}, {op}, right after"
    cost = rollout(eng, where)
    oc = ora.rollout_velocity(cmds, ref.astype(np.float64))  # (reset: the scale of the tolerance only - the recipe is latched by the next update)
    bound = lf.rollout_tolerance(cfg, general, oc)
    if op == "reset":
        twin_cost = rollout(other.players[0].sim, where + ", the other history")
        diff = float(np.abs(cost[m] - twin_cost[m]).max())
        print(f"launch forms ROLLOUT {where}: the reset robots' cost rows of two histories differ by {diff:.3e}")
        assert diff <= (bound if general else 0.0), f"{where}: the rollout of a reset robot remembers the robot's history ({diff:.3e})"
        assert not np.array_equal(cost[~m], twin_cost[~m])
    else:
        against(cost, where)
        src = sc.source[m]
        diff = float(np.abs(cost[m] - cost[src]).max())
        print(f"launch forms ROLLOUT {where}: cost of a destination and of its source differ by {diff:.3e}")
        assert diff <= (bound if general else 0.0), f"{where}: the rollout of a destination is not its source's ({diff:.3e})"
    # 5 and 13 one-step updates later
    for steps, at in ((5, 5), (8, 13)):
        for _ in range(steps):
            eng.update(1), ora.update(1)
        against(rollout(eng, f"{kind}, {op}, +{at}"), f"{kind}, {op}, +{at}")
    # the rollout left the records alone
    eng.update(20, 10), ora.update(20)
    against_the_oracle(eng, ora, cfg, f"{kind}, {op}, a fused10 segment behind the rollouts")
    sc.close()
    if other:
        other.close()


@pytest.mark.parametrize("kind", KINDS)
def test_a_rollout_enters_velocity_mode_from_every_mode(pkg, oracle, monkeypatch, kind):
    """No op at all: the rollout at the end of the history, by the mode a robot is in (index mod 3: Position, Velocity, Force).  What 5
    found on the register-resident kinds, by its cause: the parent's kernel was off by 313 (fast_n8) and 34 (fast_n4) tolerances on the
    robots in Force mode and by at most 0.021 on the others."""
    sc = Scenario(pkg, oracle, monkeypatch, kind, "reset", ["fused10"], 1)
    cfg, eng, ora = sc.cfg, sc.players[0].sim, sc.ora.sim
    roll = lf.rollout_inputs(cfg, sc.a["pose"], 331)
    gc, oc = eng.rollout_velocity(roll["cmds"], roll["ref"]), ora.rollout_velocity(roll["cmds"], roll["ref"].astype(np.float64))
    bound = lf.rollout_tolerance(cfg, kind in GENERAL, oc)
    worst = {name: float(np.abs(gc - oc)[sc.h["group"] == g].max()) for g, name in enumerate(("Position", "Velocity", "Force"))}
    print(f"launch forms ROLLOUT {kind}, by mode: " + "  ".join(f"{k} {v / bound:.3f} x the tolerance" for k, v in worst.items()))
    for name, v in worst.items():
        assert v <= bound, f"{kind}: the rollout of the robots in {name} mode differs from the oracle's by {v:.3e} (tolerance {bound:.3e})"
    sc.close()


# ---- 6 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", LAYOUTS)
def test_resample_then_fused_launches_and_a_rollout(pkg, monkeypatch, kind):
    """the inputs of test_gpu_resample.test_fused"""
    sc = Scenario(pkg, None, monkeypatch, kind, "reset", ["fused10", "fused10"], 341)
    cfg, P = sc.cfg, 65
    eng, twin = (p.sim for p in sc.players)
    w = ro.pattern("heavy_tail", P, 2, seed=10)
    w[3], w[70] = np.nan, -1.0
    words = np.array([123456789, 4000000000], np.uint32)
    source, _, status = eng.resample(w, words, P)  # resample_device: the map and the copy on it, back to back
    assert status[0] > 20 and status[1] == 0 and cr.validate_map(source) is None
    twin.copy_robots(source)
    assert equal_rows(every_getter(eng, cfg, pkg), every_getter(twin, cfg, pkg), EVERY, EVERY), kind
    for e in (eng, twin):
        e.update(30, 10)
    assert eng.kernel_name == pkg.plan_kernel(cfg, 10)
    assert equal_rows(every_getter(eng, cfg, pkg), every_getter(twin, cfg, pkg), EVERY, EVERY), f"{kind}: resample_device and copy_robots(its map) part in fused launches"
    roll = lf.rollout_inputs(cfg, sc.a["pose"], 342)
    costs = [e.rollout_velocity(roll["cmds"], roll["ref"]) for e in (eng, twin)]
    assert np.isfinite(costs[0]).all() and np.array_equal(costs[0], costs[1]), f"{kind}: resample_device and copy_robots(its map) part in the rollout"
    dest = cr.destinations_of(source)
    if kind not in GENERAL:  # (a destination still is its source: same commands since)
        got = every_getter(eng, cfg, pkg)
        assert equal_rows(got, got, dest, source[dest]), kind
    sc.close()
