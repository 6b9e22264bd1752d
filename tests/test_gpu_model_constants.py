"""Every kernel family on a model that is not the unit cube.  Sets, reasons and the tolerance: tests/model_constants.py; that the sets
are benign and that every varied constant has teeth on the oracle alone: tests/test_model_constant_inputs.py.

The other GPU matrices (workspace, Pid limits, padded stride, late clock, launch forms, quaternion stages) run on mass 1, inertia
diag(1, 1, 1), joint_damping 1, gravity (0, 0, -9.8), dt 1e-3 and a spawn pose with R = I.  There the world step's R Ib^-1 (R^T tau -
w_b x Ib w_b) is tau whatever R and whichever entry of Ib a kernel reads.  Under M, H and S (full tensors, other masses, dampings,
gravity with x and y parts, dt 5e-4 and 2e-3, a moved and turned spawn pose) it is not.

  a  the matrix: every cell of workspace_poses.CELLS under each set through workspace_poses.closed_loop_cell - the body of
     tests/test_gpu_workspace.py's matrix, every property of it - at model_constants.tolerance (TOL / TOL64, effort x max(1, 1e-3 / dt)).
  b  the steady role-split kernel, whose controller wave takes the rotation matrix from the estimator wave (CDPR_STEADY_SHARED_ROT),
     on the `split` cell's config under each set, 65 and 64 robots from quat_stage_poses.start_state, 25 one-step launches in Velocity
     mode with a new command every 10: the default handle, a CDPR_SPLIT_STEADY=0 handle and a CDPR_ONESTEP=1 handle bit equal on all
     five read-outs after every step, the default handle within tolerance of the oracle, last_variant crossing into the steady
     instantiation where the window filled.
  c  the MPC rollout under S on fast_n8, general_lean_hot and fp64_n8 of tests/per_robot_kinds.py against the oracle's
     (launch_forms.rollout_inputs, rollout_tolerance; model_constants.rollout_case: a history of 37 steps in three modes, poses from box
     W).  The cost is a plain sum of squared distances over the horizon on both sides (no dt in it), so the check stands at
     dt = 2e-3; the oracle at the shipped dt is 4 000 tolerances away.
  d  cdpr_reset and the first publish under S: a fresh handle and a handle after cdpr_reset sit at the moved home pose to the bit
     of Config.model.home_pose() in the handle's precision, and publish joint positions within TOL["q"] of 0 (TOL64 on precision = 64).
  e  coverage (every family of workspace_poses.FAMILIES, and the steady variant, under each set) and the report (-s).

Measured on MI355X (this module's run inside the whole GPU suite: 79 cases in 6 s, the slowest 0.34 s; test_zz_report_measured_agreement
prints every row with -s).  Worst error against the oracle per set, over the eighteen fp32 cells and over the three precision = 64 cells:
  M  fp32  pose 8.9e-7   twist 9.2e-6   q 3.3e-7   qd 1.0e-5   effort 3.2e-3 N (pair_stream)  FK estimate 2.2e-6  tension 3.0e-3 N
     fp64  pose 1.1e-15  twist 1.8e-14  q 4.4e-16  qd 1.6e-14  effort 6.2e-12 N
  H  fp32  pose 6.1e-7   twist 2.6e-5   q 3.5e-7   qd 2.6e-5   effort 1.2e-2 N (n12)          FK estimate 2.6e-6  tension 1.2e-2 N
     fp64  pose 8.9e-16  twist 5.1e-14  q 6.7e-16  qd 4.8e-14  effort 1.5e-11 N
  S  fp32  pose 9.8e-7   twist 7.0e-6   q 5.2e-7   qd 1.0e-5   effort 1.9e-3 N (n12)          FK estimate 2.1e-6  tension 1.9e-3 N
     fp64  pose 1.0e-15  twist 1.5e-14  q 6.7e-16  qd 1.4e-14  effort 3.6e-12 N
  (precision = 64: FK estimate 3.0e-8 and tension 3.8e-6 N, both read out as float32.)  At dt = 5e-4 the fp32 effort is 1.2e-2 N: inside
  the 4e-2 N that parity.py's scaling argument allows and inside the unscaled 2e-2 N.
  No flag of the tension distribution differs in any cell; at most one robot of 130 lies within 5e-3 N of a bound in the Force
  segment (M lowreg, M gen_step, H gen_lean, S joint_stop).
  b  steady role-split under M / H / S: pose 1.8e-7, twist 6.0e-7, q 1.7e-7, qd 5.7e-7, effort 1.0e-3 N; bit equal to the generic and to
     the one-wave kernel on every step of every case.
  c  rollout costs: 0.011 (fast_n8), 0.016 (general_lean_hot) and 0.12 (fp64_n8) of the tolerance.
  d  q = 0 exactly at the first publish on all three kinds, fresh and behind cdpr_reset.
Nothing was outside the tolerances and no kernel defect was found.

Teeth, on scratch builds that were not committed (the older GPU tests: 1 371 that run and 109 that skip themselves):
  1  integrate_velocity (cdpr_step_kernel.hpp) with R where R^T belongs and back - right for an isotropic tensor: 60 of this module's 79
     cases fail (every fp32 cell of a but the three `lumped` ones, whose 6 x 6 world step does not call that function; all six of b;
     the three coverage tests), 19 pass (the nine precision = 64 cells, the three lumped cells, c - a sum of squared position errors
     over 14 steps sees little of the rotation, tests/test_model_constant_inputs.py prints how little -, d and the report).  Of the
     older GPU tests 34 fail: 33 cases of test_randomised_model_and_controller_parameters (the kernels AUTO picks, one-step launches)
     and test_loaded_models_run_on_the_hip_path; the 1 337 others, every matrix among them, pass.
  2  the matrix transposed on the way back to the world frame alone: the same 60 of 79, but 613 of the older tests fail too, since
     R^T R^T tau is wrong on any tensor once R != I.  That defect does not speak to the gap; 1 does.
"""
from dataclasses import replace

import numpy as np
import pytest

import launch_forms as lf
import model_constants as mc
import parity
import per_robot_kinds as prk
import robot_histories as ri
import workspace_poses as wp
from parity import NAMES, TOL, TOL64, assert_within, observed, worst_errors
from quat_stage_poses import KAPPA_MAX, TURNING, start_state

pytestmark = pytest.mark.gpu

clean_env = parity.clean_env_fixture("CDPR_SPLIT_STEADY", "CDPR_NO_GRAPH")

WORST = {}
RAN = {}  # "set cell" -> kernel names its launches ran on; "set steady" -> the steady instantiation of section b
STEADY = "steady"
CASES = [(name, cell) for name in mc.SETS for cell in wp.CELLS]


def note(where, name, err):
    WORST[(where, name)] = max(WORST.get((where, name), 0.0), float(err))


# ---- a. the matrix -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cell", CASES, ids=[f"{s} {c}" for s, c in CASES])
def test_closed_loop_cell_under_the_set(pkg, oracle, monkeypatch, name, cell):
    cfg, env, seed = mc.cell_config(pkg, cell, name)
    assert cfg.batch == 130 and sum(k for _, k in wp.SCRIPT) == 110
    wp.closed_loop_cell(pkg, oracle, monkeypatch, cfg, env, seed, mc.tolerance(cfg), RAN, WORST, f"{name} {cell}")


# ---- b. the steady role-split kernel and its handed-over matrix ------------------------------------------------------------------
STEPS, REFRESH = 25, 10
SPLIT, ONE_WAVE = "cdpr_split_kernel<8, false>", "cdpr_step_kernel<"


def make_engine(pkg, monkeypatch, cfg, pose, twist, **env):
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        eng = pkg.Engine(cfg, 0)  # (the overrides are read when the handle is created)
    eng.set_platform_state(pose7=pose, twist6=twist)
    return eng


@pytest.mark.parametrize("batch", [65, 64])
@pytest.mark.parametrize("name", list(mc.SETS))
def test_steady_role_split_against_generic_one_wave_and_oracle(pkg, oracle, monkeypatch, name, batch):
    cfg, env, _ = mc.cell_config(pkg, "split", name, batch)
    assert not env and cfg.stages == 3 and cfg.n_cables == 8
    tol = mc.tolerance(cfg)
    pose, twist, kappa = start_state(pkg, 8, batch)
    assert kappa <= KAPPA_MAX, kappa
    default = make_engine(pkg, monkeypatch, cfg, pose, twist)
    generic = make_engine(pkg, monkeypatch, cfg, pose, twist, CDPR_SPLIT_STEADY="0")
    one_wave = make_engine(pkg, monkeypatch, cfg, pose, twist, CDPR_ONESTEP="1")
    ora = oracle.OracleSim(cfg.to_struct(), oracle.DERIV_EXACT)
    ora.set_platform_state(pose7=pose.astype(np.float64), twist6=twist.astype(np.float64))
    sims = [default, generic, one_wave, ora]
    vel = np.random.default_rng(4100 + batch).uniform(-0.03, 0.03, (3, batch, 8)).astype(np.float32)
    variants = []
    for k in range(STEPS):
        if k % REFRESH == 0:
            for s in sims:
                s.set_velocity_command(vel[k // REFRESH])
        for s in sims:
            s.update(1)
        if k == 0:  # the turning robot has made its turn: every simulator goes on from the default handle's rates with that one at zero
            t = default.raw_state()[1].copy()
            t[TURNING] = 0.0
            for s in sims:
                s.set_platform_state(twist6=t)
        got = default.observables()
        for other, what in ((generic, "the generic role-split kernel"), (one_wave, "the one-wave kernel")):
            diff = [key for key, x, y in zip(("q", "qd", "eff", "pose", "twist"), got, other.observables()) if not np.array_equal(x, y)]
            assert not diff, f"{name}, step {k}: {diff} differ between the default handle and {what}"
        assert default.kernel_name == generic.kernel_name == SPLIT and one_wave.kernel_name.startswith(ONE_WAVE), (default.kernel_name, one_wave.kernel_name)
        assert generic.last_variant == 0
        variants.append(default.last_variant)
        worst = worst_errors(observed(default), observed(ora), f"{name}, step {k}")
        for key in NAMES:
            note(f"{name} {STEADY}", key, worst[key][0])
        if any(worst[key][0] > tol[key] for key in NAMES):
            print(f"{name}, step {k}: " + "  ".join(f"{key} {v[0]:.2e} (robot {v[1]})" for key, v in worst.items()))
        assert_within(worst, tol, f"{name}, b{batch}, step {k}")
    nbuf = cfg.velocityController.dBufferLength
    assert variants == [0] * (nbuf + 1) + [1] * (STEPS - nbuf - 1), variants  # the launches crossed into the steady kernel where the window filled
    RAN.setdefault(f"{name} {STEADY}", set()).add(f"{default.kernel_name} (steady)")
    for other in (generic, one_wave):
        for x, y in zip(list(default.raw_state()) + list(default.fk_state()) + list(default.td_state()), list(other.raw_state()) + list(other.fk_state()) + list(other.td_state())):
            assert np.array_equal(x, y)
    rate = float(np.abs(default.raw_state()[1][:, 3:]).max())
    print(f"{name} b{batch}: steady role-split, worst against the oracle: " + "  ".join(f"{key} {WORST[(f'{name} {STEADY}', key)]:.2e}" for key in NAMES) + f"; |w| up to {rate:.2f} rad/s at the end")
    for s in sims:
        s.close()


# ---- c. the MPC rollout under S -------------------------------------------------------------------------------------------------
KINDS = mc.ROLLOUT_KINDS  # register-resident, general path, precision = 64


@pytest.mark.parametrize("kind", KINDS)
def test_rollout_under_S(pkg, oracle, monkeypatch, kind):
    cfg, h, pose, roll = mc.rollout_case(pkg, kind, monkeypatch)
    assert cfg.dt == 2e-3
    (eng,), ora = parity.sims_at(pkg, oracle, cfg, pose)
    ri.play_history([eng, ora], h)
    prk.named(eng, kind)
    horizon = roll["cmds"].shape[1]
    before = prk.state_of(eng, cfg)
    got = eng.rollout_velocity(roll["cmds"], roll["ref"])
    assert eng.kernel_name == pkg.plan_kernel(cfg, horizon, flags=pkg._abi.PLAN_ROLLOUT), eng.kernel_name
    want = ora.rollout_velocity(roll["cmds"], roll["ref"].astype(np.float64))
    assert got.shape == want.shape == (lf.B, lf.SAMPLES) and np.isfinite(got).all()
    err, bound = float(np.abs(got - want).max()), lf.rollout_tolerance(cfg, kind in lf.GENERAL, want)
    note(f"S rollout {kind}", "cost / tolerance", err / bound)
    print(f"rollout under S, {kind} ({eng.kernel_name}, {horizon} steps): max |cost - oracle| {err:.3e} = {err / bound:.3f} x the tolerance; costs up to {np.abs(want).max():.3e}")
    assert err <= bound, f"{kind}: the costs differ from the oracle's by {err:.3e} (tolerance {bound:.3e})"
    for x, y in zip(before, prk.state_of(eng, cfg)):
        assert np.array_equal(x, y), f"{kind}: the rollout changed what a getter returns"
    # dt is in the rollout's own integration: the oracle at the shipped dt is far outside the tolerance
    ora2 = parity.oracle_at(oracle, replace(cfg, dt=mc.DEFAULTS["dt"]), pose)
    ri.play_history([ora2], h)
    assert np.abs(ora2.rollout_velocity(roll["cmds"], roll["ref"].astype(np.float64)) - want).max() > 20 * bound
    eng.close(), ora.close(), ora2.close()


# ---- d. cdpr_reset and the first publish under S --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_home_pose_after_create_and_after_reset_under_S(pkg, oracle, monkeypatch, kind):
    cfg = mc.apply(prk.config_of(pkg, kind, monkeypatch), "S")
    f64 = cfg.precision == 64
    B = cfg.batch
    home64 = np.tile(np.asarray(cfg.model.home_pose(), dtype=np.float64), (B, 1))
    home = home64 if f64 else home64.astype(np.float32)
    assert np.abs(home64[0] - wp.cell_model(pkg, 8).home_pose()).max() > 0.02  # (the moved home)
    tolq = (TOL64 if f64 else TOL)["q"]
    used, fresh = pkg.Engine(cfg, 0), pkg.Engine(cfg, 0)
    ora = oracle.OracleSim(cfg.to_struct(), oracle.DERIV_EXACT)
    h = ri.history_inputs(cfg.model, 613)
    # the used handle leaves home first: a history from other poses, then cdpr_reset
    used.set_platform_state_f64(pose7=h["pose"].astype(np.float64)) if f64 else used.set_platform_state(pose7=h["pose"])
    ri.play_history([used], h)
    assert not np.array_equal((used.raw_state_f64() if f64 else used.raw_state())[0], home)
    used.reset()
    for eng, what in ((fresh, "a fresh handle"), (used, "a handle after cdpr_reset")):
        p, t = eng.raw_state_f64() if f64 else eng.raw_state()
        assert p.dtype == home.dtype and np.array_equal(p, home), f"{kind}: {what} is not at the home pose to the bit"
        assert not t.any(), f"{kind}: {what} is not at rest"
        assert eng.step_count == 0
    for sim in (fresh, used, ora):
        sim.update(1)
    want = observed(ora)
    assert np.array_equal(want[0], home64) and np.abs(want[2]).max() < 1e-15  # (the oracle publishes the state at t_0: the home pose, q = 0)
    for eng, what in ((fresh, "a fresh handle"), (used, "a handle after cdpr_reset")):
        got = observed(eng, f64)
        assert np.array_equal(got[0], home), f"{kind}: the first publish of {what} is not the home pose to the bit"
        q = float(np.abs(got[2]).max())
        note(f"S first publish {kind}", "q", q)
        print(f"first publish under S, {kind}, {what}: |q| up to {q:.3e}")
        assert q <= tolq, f"{kind}: {what} publishes joint positions {q:.3e} from 0 at the home pose (tolerance {tolq:.1e})"
        assert_within(worst_errors(got, want, f"{kind}, {what}, first publish", f64=f64), mc.tolerance(cfg), f"{kind}, {what}, first publish")
    for x, y in zip(prk.state_of(used, cfg), prk.state_of(fresh, cfg)):
        assert np.array_equal(x, y), f"{kind}: one step behind cdpr_reset differs from one step on a fresh handle"
    for sim in (fresh, used, ora):
        sim.update(12)
    for x, y in zip(prk.state_of(used, cfg), prk.state_of(fresh, cfg)):
        assert np.array_equal(x, y), f"{kind}: 13 steps behind cdpr_reset differ from 13 steps on a fresh handle"
    assert_within(worst_errors(observed(fresh, f64), observed(ora), f"{kind}, 13 steps from home", f64=f64), mc.tolerance(cfg), f"{kind}, 13 steps from home")
    assert prk.HANDLES[kind][3][0] in fresh.kernel_name and fresh.kernel_name == used.kernel_name, (kind, fresh.kernel_name, used.kernel_name)
    fresh.close(), used.close(), ora.close()


# ---- e. coverage and report -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mc.SETS))
def test_zy_every_family_ran(pkg, name):
    """As test_zy_every_family_ran of tests/test_gpu_workspace.py, under each set, with the steady instantiation of section b as a
    family of its own."""
    missing = [fam for fam, (cell, pred) in wp.FAMILIES.items() if not any(pred(k) for k in RAN.get(f"{name} {cell}", ()))]
    if not RAN.get(f"{name} {STEADY}"):
        missing.append("cdpr_split_kernel, steady instantiation (section b)")
    assert not missing, (f"families that did not run under set {name} IN THIS PROCESS: {missing}.  This test reads what sections a and b recorded: run the "
                         f"whole module in one process (no -k, no single node id, no distributing plugin); only then does a missing family mean a "
                         f"routing change.  Ran: { {c: sorted(v) for c, v in RAN.items() if c.startswith(name + ' ')} }")
    cfg = mc.cell_config(pkg, "lumped", name)[0]
    assert cfg.model.leg_inertia > 0 and mc.cell_config(pkg, "joint_stop", name)[0].model.travel_stop > 0 and mc.cell_config(pkg, "per_robot", name)[0].perRobotCommands
    assert cfg.model.mass == mc.SETS[name]["model"]["mass"] and tuple(cfg.model.inertia) == mc.SETS[name]["model"]["inertia"] and cfg.dt == mc.SETS[name]["config"]["dt"]
    print(f"model constants, set {name}: all {len(wp.FAMILIES)} families and the steady instantiation ran")


def test_zz_report_measured_agreement(pkg):
    """Largest error seen per set, cell and quantity in this module's run, and per set over the fp32 and the precision = 64 cells
    (printed with -s)."""
    for (where, key), err in sorted(WORST.items()):
        print(f"model constants agreement: {where:24s} {key:36s} {err:.3e}")
    for name in mc.SETS:
        for f64 in (False, True):
            cells = [c for c in wp.CELLS if (wp.CELLS[c][1].get("precision") == 64) == f64]
            row = {key: max([WORST.get((f"{name} {c}", key), 0.0) for c in cells]) for key in NAMES + ("fk estimate", "tension")}
            at = max(cells, key=lambda c: WORST.get((f"{name} {c}", "eff"), 0.0))
            print(f"model constants summary: set {name}, {'precision = 64' if f64 else 'fp32'} cells: " + "  ".join(f"{k} {v:.1e}" for k, v in row.items()) + f"  (worst effort: {at})")
