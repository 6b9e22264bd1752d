"""The Pid's clamps and the hold threshold in every kernel family, against the oracle.

The other GPU modules meet the oracle where the controller is linear: under the shipped limits (iLimit 100, cmdLimit 100, effort
limit 100) and their commands |iTerm| stays below 1 N, and the one test that saturates (test_saturation_and_anti_windup) does so
on the fast path with cmdLimit = effort limit, where SetForce cuts off what the anti-windup leaves beyond the clamp.  A wrong sign
on iMin, a wrong 1 / iGain or a back-calculation written to the wrong lane passes all of them.  Here the limits come from
tests/pid_limits.py, and tests/test_pid_limit_inputs.py establishes on the oracle alone that each limit bites (taking it away
moves the efforts by more than 10 x the tolerance on >= 20 % of the robots at two checkpoints or more), that the inputs are benign
(the oracle's own sensitivity to one float32 rounding of the start pose is 100 x below the tolerance) and that a decision taken a
step apart costs at most half the effort tolerance.

  a. the matrix: one case per cell of workspace_poses.CELLS and variant (`command`, `integral`; `command_low_effort` on seven
     cells), 130 robots, the variant's script with the oracle after every run at TOL (TOL64 on precision = 64 cells), on one-step
     launches and on fused launches; kernel_name = plan_kernel.
  b. launch forms: on the step, gen_split and f64_split cells under `command`, one-step launches, fused launches and the
     trajectory record give the same bits.
  c. the hold ladder: targets on, one float32 below and one float32 above float32(velocityEpsilon) (at epsilon = 0: +-0, the
     smallest subnormal, the smallest normal), on six fp32 general handles and two fp64 controls, the oracle 1, 2, 5, 12 and 20
     steps after each of two Joys.  A branch taken differently from the oracle moves efforts by tens of newtons.
  d. the MPC rollout under `command` on a fast, a general and an fp64 handle: costs against oracle.rollout_velocity at
     1e-6 + 2e-4 max |cost|, the engine's state bit-identical before and after.
  e. coverage (every family of workspace_poses.FAMILIES ran) and the report of the worst errors (-s).

Measured on MI355X (this module's run inside the whole GPU suite; test_zz_report_measured_agreement prints every row with -s):
  a. worst over the fp32 cells, one-step and fused launches (pose, twist, q, qd, effort):
       command             4.9e-7  2.3e-5  4.6e-7  2.4e-5  4.4e-3 N
       command_low_effort  5.4e-7  2.2e-5  6.0e-7  1.7e-5  3.4e-3 N
       integral            4.8e-7  2.7e-5  3.7e-7  2.8e-5  3.9e-3 N
     worst over the precision = 64 cells:
       command             1.7e-15  6.9e-14  1.8e-15  6.9e-14  1.2e-11 N
       command_low_effort  1.7e-15  4.7e-14  1.6e-15  4.4e-14  1.0e-11 N
       integral            8.3e-16  5.8e-14  1.0e-15  6.6e-14  8.9e-12 N
     (the efforts stay under the largest anti-windup increment of the inputs, 8.1e-3 N: no clamp decision showed a step apart.)
  c. ladder: fp32 handles pose 1.9e-7, twist 1.4e-5, q 2.4e-7, qd 1.4e-5, effort 4.4e-3 N; fp64 controls 2.6e-16, 3.9e-14,
     3.3e-16, 3.6e-14, 9.4e-12 N.  The subnormal targets at epsilon = 0 take the velocity Pid on every handle, as in the oracle.
  d. rollout costs: fast 6.7e-8 (tolerance 1.7e-6), general 8.3e-8 (1.7e-6), fp64 1.2e-10 (1.7e-6).
No case was outside TOL / TOL64.  One defect was found, at the hold threshold: the host handed the fp32 general kernels
(float)velocityEpsilon, which rounds up for 0.001 and 0.004, so a target equal to float32(epsilon) held position where the reference
runs the velocity Pid.  With that library the ladder fails at epsilon 0.001 and 0.004 on all six fp32 handles (12 cases) and passes
at 0.01 and 0, and on both fp64 controls at every epsilon; general_ctl now passes the largest float32 not above epsilon.
"""
import numpy as np
import pytest

import parity
import pid_limits as pl
import workspace_poses as wp
from parity import TOL, TOL64, observed, state_of

pytestmark = pytest.mark.gpu

WORST = {}
RAN = {}  # cell -> kernel names its launches ran on
clean_env = parity.clean_env_fixture()


def note(where, name, err):
    WORST[(where, name)] = max(WORST.get((where, name), 0.0), float(err))


def start(pkg, oracle, cfg, pose, engines=1):
    return parity.sims_at(pkg, oracle, cfg, pose, engines, through_f32=False)  # (the oracle starts at the doubles)


def against_the_oracle(eng, ora, f64, where, report, failures):
    """every quantity outside its tolerance is a line of `failures`, with the robot and the column"""
    tol = TOL64 if f64 else TOL
    got, want = observed(eng, f64), observed(ora)
    for name, (err, r, i) in parity.worst_errors(got, want, where, f64=f64).items():
        note(report, name, err)
        if err > tol[name]:
            g, o = got[parity.NAMES.index(name)], want[parity.NAMES.index(name)]
            failures.append(f"{where}: {name} differs from the oracle by {err:.3e} (tolerance {tol[name]:.1e}; robot {r}, column {i}: {g[r, i]!r} against {o[r, i]!r})")


# ---- a. the matrix -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell,variant", pl.CASES)
def test_clamps_against_the_oracle(pkg, oracle, monkeypatch, cell, variant):
    own, cfg, env, pose, cmds = pl.case_inputs(pkg, cell, variant)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    f64 = cfg.precision == 64
    (a, b), ora = start(pkg, oracle, cfg, pose, 2)  # a: one step per launch; b: fused (10 per launch)
    ran = RAN.setdefault(cell, set())
    failures = []
    script = pl.SCRIPTS[variant]
    for j, k in pl.play(variant, cmds, (a, b, ora)):
        a.update(k)
        b.update(k, 10)
        ora.update(k)
        ran.update((a.kernel_name, b.kernel_name))
        where = f"{cell}, {variant}, run {j} ({k} steps after {script[j - 1][:2] if j else 'Load'})"
        kind = f"{variant}, fp64" if f64 else variant
        against_the_oracle(a, ora, f64, where, kind, failures)
        against_the_oracle(b, ora, f64, where + ", fused launches", kind, failures)
    assert a.kernel_name == pkg.plan_kernel(cfg, 1) == pkg.plan_kernel(own, 1), (cell, variant)
    assert not failures, "\n".join(failures)
    for e in (a, b):
        e.close()
    ora.close()


# ---- b. launch forms -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", ["step", "gen_split", "f64_split"])
def test_launch_forms_give_the_same_bits_under_the_command_clamp(pkg, oracle, monkeypatch, cell):
    own, cfg, env, pose, cmds = pl.case_inputs(pkg, cell, "command")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    f64 = cfg.precision == 64
    (a, b, c), ora = start(pkg, oracle, cfg, pose, 3)
    for j, k in pl.play("command", cmds, (a, b, c)):
        a.update(k)
        b.update(k, 10)
        rec = c.update_record(k, 10)
        sa = state_of(a, f64)
        for e, form in ((b, "fused"), (c, "recorded")):
            for x, y in zip(sa, state_of(e, f64)):
                assert np.array_equal(x, y), f"{cell}, run {j}: {form} launches differ from one-step launches"
        for i, key in enumerate(("position", "velocity", "effort", "pose", "twist")):
            assert np.array_equal(rec[key][-1], sa[2 + i]), f"{cell}, run {j}: the record's last step is not the published one ({key})"
    for e in (a, b, c):
        e.close()
    ora.close()


# ---- c. the hold ladder --------------------------------------------------------------------------------------------------------
# handle: (cables, Config keywords, environment switches)
LADDER_HANDLES = {
    "gen_step":      (8, dict(stages=3), {"CDPR_GEN_SPLIT": "0"}),
    "gen_split":     (8, dict(stages=3), {}),
    "gen_lean":      (8, dict(stages=3), {"CDPR_GEN_SPLIT": "0", "CDPR_GEN_LEAN": "1"}),
    "one_wave":      (8, dict(stages=3), {"CDPR_GEN_SPLIT": "0", "CDPR_GEN_LEAN": "0"}),
    "per_robot":     (8, dict(stages=3, perRobotCommands=True), {}),
    "cube":          (4, dict(stages=0), {}),
    "f64":           (8, dict(stages=3, precision=64), {}),
    "f64_per_robot": (8, dict(stages=3, precision=64, perRobotCommands=True), {}),
}


@pytest.mark.parametrize("eps", pl.LADDER_EPS)
@pytest.mark.parametrize("handle", list(LADDER_HANDLES))
def test_hold_threshold_ladder(pkg, oracle, monkeypatch, handle, eps):
    n, kw, env = LADDER_HANDLES[handle]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg = pkg.Config(model=wp.cell_model(pkg, n), batch=pl.B, velocityEpsilon=eps, **kw)
    f64 = cfg.precision == 64
    name = pkg.plan_kernel(cfg, 1)
    assert ("f64" in name and "HOLD" in name) if f64 else "gen" in name, name  # the hold branch is live on this handle
    pose = pl.start_poses(cfg.model, np.random.default_rng(pl.LADDER_SEED))
    (eng,), ora = start(pkg, oracle, cfg, pose)
    eng.update(15), ora.update(15)
    failures = []
    for which, joy in zip(("first", "second"), pl.ladder_targets(eps, pl.B, n)):
        eng.set_velocity_command(joy), ora.set_velocity_command(joy)
        done = 0
        for k in pl.LADDER_CHECKPOINTS:
            eng.update(k - done), ora.update(k - done)
            done = k
            against_the_oracle(eng, ora, f64, f"{handle}, eps {eps}, {k} steps after the {which} Joy", "ladder, fp64" if f64 else "ladder", failures)
    if failures:  # name the values of the ladder on which the efforts differ
        vel = pl.velocity_branch(joy, eps)
        bad = np.abs(observed(eng, f64)[4] - ora.joint_states()[2]) > (TOL64 if f64 else TOL)["eff"]
        failures.append(f"targets of the cables that differ now: {sorted(set(float(v) for v in joy[bad]))} (velocity Pid expected: {sorted(set(bool(v) for v in vel[bad]))})")
    assert eng.kernel_name == name
    assert not failures, "\n".join(failures)
    eng.close()
    ora.close()


# ---- d. the rollout ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("handle", list(pl.ROLLOUT_HANDLES))
def test_rollout_under_the_command_clamp(pkg, oracle, handle):
    cfg, pose, cmds = pl.rollout_inputs(pkg, handle)
    f64 = cfg.precision == 64
    (eng,), ora = start(pkg, oracle, cfg, pose)
    eng.update(pl.ROLLOUT["warm"]), ora.update(pl.ROLLOUT["warm"])
    ref = pl.rollout_ref(ora)
    before = state_of(eng, f64)
    gc = eng.rollout_velocity(cmds, ref)
    oc = ora.rollout_velocity(cmds, ref.astype(np.float64))
    err, tol = float(np.abs(gc - oc).max()), parity.rollout_cost_tol(oc, 1e-6)
    note(f"rollout, {handle}", "cost / tolerance", err / tol)
    print(f"rollout under the command clamp, {handle} handle: costs differ by {err:.3e} (tolerance {tol:.3e})")
    assert gc.shape == (pl.ROLLOUT["B"], pl.ROLLOUT["S"]) and np.isfinite(gc).all()
    assert err < tol, (handle, err, tol)
    for x, y in zip(before, state_of(eng, f64)):
        assert np.array_equal(x, y), f"{handle}: the rollout changed the engine's state"
    failures = []
    eng.update(5), ora.update(5)  # and the engine carries on as if nothing had happened
    against_the_oracle(eng, ora, f64, f"{handle}: after the rollout", f"rollout, {handle}", failures)
    assert not failures, "\n".join(failures)
    eng.close()
    ora.close()


# ---- e. coverage and report ----------------------------------------------------------------------------------------------------
def test_zy_every_family_ran(pkg):
    """The launches of the matrix ran on every family of workspace_poses.FAMILIES (a routing change, or a limit that re-routes
    a handle, cannot hollow the module out)."""
    missing = [fam for fam, (cell, pred) in wp.FAMILIES.items() if not any(pred(k) for k in RAN.get(cell, ()))]
    assert not missing, (f"families that did not run IN THIS PROCESS: {missing}.  This test reads what test_clamps_against_the_oracle recorded: run "
                         f"the whole module in one process (no -k, no single node id, no distributing plugin); only then does a missing family "
                         f"mean a routing change.  Ran: { {c: sorted(v) for c, v in RAN.items()} }")


def test_zz_report_measured_agreement():
    """Largest error seen per quantity and variant in this module's run (printed with -s)."""
    for (where, name), err in sorted(WORST.items()):
        print(f"pid limits agreement: {where:28s} {name:18s} {err:.3e}")
