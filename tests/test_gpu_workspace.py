"""Every kernel family across the workspace, and IK against the reference's own geometry away from R = I.

The other GPU modules start their robots within +-0.05 m and +-0.1 rad of the spawn pose (R ~ I, cond(J^T J) ~ 1.2e3): a wrong
sign on an off-diagonal rotation term, a quaternion update that is only right for small angles or a Cholesky that loses its pivot
at cond 3e4 stays under their tolerances.  Here the poses come from tests/workspace_poses.py: box W (+-0.15 m, z 0.15 .. 0.45,
tilt +-0.3 rad, yaw +-pi), box E (+-0.20 m, z 0.10 .. 0.50, tilt +-0.4 rad, yaw +-pi), and the special poses (yaw exactly pi with
w = 0, yaw +-pi / 2, the largest tilt about x and about y alone, the corners of W's position box, each once more with the
quaternion negated).  tests/test_workspace_inputs.py establishes on the oracle alone that these inputs are benign (the oracle's own
sensitivity to one float32 rounding of the start pose is 100x below TOL; FK converges from near seeds; <= 1 % of the robots sit
within 5e-3 N of a tension bound).

  a. cdpr_solve_ik on the cube model against tests/golden/geometry_workspace.json (gen_cdpr.py:101-125 evaluated with the
     reference's transformations.py at 77 poses): L0 - L and the Jacobian at 2e-7, the tolerance of test_solve_ik_matches_oracle
     (the absolute figure holds, so the restatement as 2 ulp of L is not needed); q from a pose and from its negated quaternion
     bit for bit.
  b. the one-shot solvers over E at eight and twelve cables, 500 robots: IK against oracle.ik, FK from near seeds (8 iterations,
     fkTolerance 1e-6), TD against oracle.td_wrench at 5e-3 N with flags equal except within 5e-3 N of a bound.  The balance
     -J^T t = w of unflagged robots is formed with the oracle's Jacobian and asserted at 2e-3 N, the bound of
     test_solve_td_matches_oracle_and_flags_infeasible.
  c. the closed-loop matrix over W: one cell per kernel family of the selection table (workspace_poses.CELLS), 130 robots (two
     workgroups and a ragged third), the script hold 5 / velocity 30 / position 30 / force 20 / velocity 25, the oracle after every
     segment at TOL (TOL64 on precision = 64 handles), one-step = fused = recorded launches bit for bit, kernel_name = plan_kernel,
     FK iteration counts and estimates, TD tensions and flags, (q, -q) twins bit-identical with negated published quaternions.
  d. the headline launch (65 536 x 8, FK + TD, cdpr_split_kernel) from W: three 128-robot slices against the oracle, duplicate
     halves, a permuted batch, unit quaternions, the FK estimate against the true pose.
  e. coverage (every family of the list ran) and the report of the worst errors (-s).

Measured on MI355X (this module's run inside the whole GPU suite; test_zz_report_measured_agreement prints every row with -s):
  a. IK against the fixture: q 8.7e-8, Jacobian 1.4e-7.
  b. over E: solve_ik q 1.0e-7, qd 7.0e-8, J 1.6e-7; solve_fk estimate 3.1e-6 (n = 8) and 1.4e-6 (n = 12) outside the exit class,
     2.6e-6 and 1.41e-5 inside it, residual 9.5e-7, iteration counts within 1; solve_td tension 2.2e-4 N, balance (kernel's Jacobian) 3.5e-5 N, no flag
     differs (0 and 1 robots of 500 within 5e-3 N of a bound).
  c. worst over the eighteen fp32 cells: pose 5.7e-7, twist 1.7e-5, q 5.1e-7, qd 2.0e-5, effort 3.9e-3 N (the step cell; 2.3e-3 N
     near the spawn pose: L grows from 0.49 m to 0.95 m and its rounding with it), FK estimate 3.3e-6 (pair cell), tension
     3.9e-3 N, no flag differs in any cell; worst over the three precision = 64 cells: pose 1.0e-15, twist 3.1e-14, q 7.8e-16,
     qd 3.3e-14, effort 6.4e-12 N, FK estimate 3.0e-8 and tension 3.8e-6 N (both read out as float32).
  d. 65 536 x 8 over W: | |quat| - 1 | 1.2e-7, FK estimate against the true position 1.7e-7 (quaternion 2.7e-6, asserted at 5e-6), residual 1.5e-7.
No cell was outside TOL / TOL64 and no kernel defect was found.  With one rotation term made wrong on a scratch build (w y taken as
|w| y in quat_to_rot, cdpr_step_kernel.hpp: right for every quaternion with w >= 0) 27 of this module's 31 tests fail - (a), (b),
every fp32 cell of (c), (d) - while 502 of the 503 older GPU tests pass (the one that fails is the million-step run of
test_pid_call_counter_never_saturates, in which the platform turns over and w passes through 0).
"""
import json
import os

import numpy as np
import pytest

import workspace_poses as wp
from parity import FULL_SIZE_SLICES, TOL, TOL64, check_slice, clean_env_fixture

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
WORST = {}
RAN = {}  # cell -> kernel names its launches ran on


def note(where, name, err):
    WORST[(where, name)] = max(WORST.get((where, name), 0.0), float(err))


clean_env = clean_env_fixture()


def quat_diff(g, o):
    """|g - o| per component with the quaternion (last four columns) compared up to sign."""
    d = np.abs(g - o)
    d[:, 3:] = np.minimum(d[:, 3:], np.abs(g[:, 3:] + o[:, 3:]))
    return d


# ---- a. IK against the reference fixture ---------------------------------------------------------------------------------------
def test_solve_ik_matches_the_reference_geometry_across_the_workspace(pkg):
    """L0 - L and the Jacobian rows [u, (R b) x u] of geometry_workspace.json at 2e-7, on the fp32 handle, the pose given as the
    reference's quaternion rounded to float32; the same poses with the quaternion negated give the same q, qdot and Jacobian bit
    for bit."""
    geo = json.load(open(os.path.join(GOLD, "geometry_workspace.json")))
    poses = geo["poses"]
    B = len(poses)
    cfg = pkg.Config(model=pkg.cube_model(), batch=B)
    l0 = cfg.model.reference_lengths()
    pose = np.array([p["xyz"] + p["quaternion_xyzw"] for p in poses]).astype(np.float32)
    twist = np.random.default_rng(5).uniform(-0.3, 0.3, (B, 6)).astype(np.float32)
    eng = pkg.Engine(cfg, 0)
    q, qd, jac = eng.solve_ik(pose, twist)
    want_q = np.array([[l0[i] - c["L"] for i, c in enumerate(p["cables"])] for p in poses])
    want_j = np.array([[c["jacobian_row"] for c in p["cables"]] for p in poses])
    length = np.array([[c["L"] for c in p["cables"]] for p in poses])
    err_q, err_j = np.abs(q - want_q), np.abs(jac - want_j)
    note("ik fixture", "q", err_q.max()), note("ik fixture", "jac", err_j.max())
    note("ik fixture", "q / ulp(L)", (err_q / np.spacing(length.astype(np.float32))).max())
    print(f"IK vs fixture: q {err_q.max():.3e} ({(err_q / np.spacing(length.astype(np.float32))).max():.2f} ulp of L), J {err_j.max():.3e}")
    assert err_q.max() < 2e-7 and err_j.max() < 2e-7
    neg = pose.copy()
    neg[:, 3:] = -neg[:, 3:]
    q2, qd2, jac2 = eng.solve_ik(neg, twist)
    assert np.array_equal(q, q2) and np.array_equal(qd, qd2) and np.array_equal(jac, jac2)
    eng.close()


# ---- b. the one-shot solvers over E --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 12])
def test_solve_ik_over_the_edge_box(pkg, oracle, n):
    cfg, inp, ref = wp.solver_reference(pkg, oracle, n)
    eng = pkg.Engine(cfg, 0)
    q, qd, jac = eng.solve_ik(inp["pose"], inp["twist"])
    sl = slice(0, None, 7)
    for name, g, o in (("q", q, ref["q"]), ("qd", qd, ref["qd"]), ("jac", jac, ref["jac"])):
        err = float(np.abs(g[sl] - o[sl]).max())
        note(f"solve_ik n={n}", name, err)
        print(f"solve_ik n = {n}: {name} {err:.3e}")
    for name, g, o in (("q", q, ref["q"]), ("qd", qd, ref["qd"]), ("jac", jac, ref["jac"])):
        assert np.abs(g[sl] - o[sl]).max() < 2e-7, (n, name)
    eng.close()


@pytest.mark.parametrize("n", [8, 12])
def test_solve_fk_from_near_seeds_over_the_edge_box(pkg, oracle, n):
    """8 iterations, fkTolerance 1e-6, seeds within +-0.03 m / +-0.1 rad of the pose (half of them with the quaternion negated):
    robots the oracle does not converge on are left out (<= 0.5 %, else the test fails); iteration counts within 1 of the
    oracle's, the estimate within 5e-6 (the quaternion up to sign).

    One pose class cannot meet 5e-6 in float32: robots whose residual passes within 2e-7 m (3 ulp of a cable length) of fkTolerance
    at some iteration of the ORACLE (workspace_poses.fk_exit_class: 19 robots of 500 at n = 8, 23 at n = 12).  Float32 and float64
    may leave the loop one iteration apart there; the solver that leaves early keeps a residual of up to 1e-6 m, which is
    1e-6 / sigma_min(J) ~ 1e-4 rad of orientation at worst (sigma_min(J) >= 0.008 over these batches).  Shown without the kernel:
    workspace_poses.fk_float32 - orc_fk's arithmetic in numpy float32 - differs from the oracle by 6.9e-6 (n = 8) and 1.40e-5
    (n = 12) on that class and by < 5e-6 outside it (tests/test_workspace_inputs.py::test_float32_fk_exit_class prints both).  The
    class is therefore held to 2 x the emulation's worst distance from the oracle there, every other robot to 5e-6."""
    cfg, inp, ref = wp.solver_reference(pkg, oracle, n)
    ok = ref["res"] < ref["fk_tolerance"]
    assert (~ok).mean() <= 0.005
    eng = pkg.Engine(cfg, 0)
    est, res, it = eng.solve_fk(ref["lengths32"], inp["seed"])
    d_it = np.abs(it[ok] - ref["it"][ok]).max()
    d_est = quat_diff(est.astype(np.float64), ref["est"]).max(axis=1)
    # the exit class (see the docstring): told apart and bounded by the float32 emulation of the ORACLE's arithmetic alone
    e_est, _, e_it = wp.fk_float32(cfg.to_struct(), ref["lengths32"], inp["seed"])
    exit_class = ok & wp.fk_exit_class(ref)
    plain = ok & ~exit_class
    tol_class = max(5e-6, 2.0 * float(quat_diff(e_est.astype(np.float64), ref["est"]).max(axis=1)[exit_class].max()))
    note(f"solve_fk n={n}", "estimate", d_est[plain].max()), note(f"solve_fk n={n}", "residual", res[ok].max())
    note(f"solve_fk n={n}", "estimate, exit class", d_est[exit_class].max() if exit_class.any() else 0.0)
    print(f"solve_fk n = {n}: iterations differ by up to {d_it}, estimate {d_est[plain].max():.3e}, residual {res[ok].max():.3e}; "
          f"exit class ({exit_class.sum()} robots): {d_est[exit_class].max() if exit_class.any() else 0.0:.3e} (tolerance {tol_class:.3e})")
    assert np.isfinite(est).all()
    assert exit_class.mean() <= 0.05
    off = np.flatnonzero(plain & (d_est >= 5e-6))
    assert d_it <= 1 and not off.size, f"robots {off}: estimate off by {d_est[off]}, oracle residuals {ref['res_seq'][off]}, iterations {it[off]} / {ref['it'][off]}"
    assert d_est[exit_class].max() <= tol_class
    eng.close()


@pytest.mark.parametrize("n", [8, 12])
def test_solve_td_over_the_edge_box(pkg, oracle, n):
    """Tensions at 5e-3 N on every robot (the clamp is continuous); flags equal except on robots whose oracle-side unclamped
    tension is within 5e-3 N of a bound (<= 1 % of the batch, else the test fails); -J^T t = w on unflagged robots, with the
    ORACLE's Jacobian, at the 2e-3 N of test_solve_td_matches_oracle_and_flags_infeasible; both flag values occur."""
    cfg, inp, ref = wp.solver_reference(pkg, oracle, n)
    near = wp.near_bound(ref["unclamped"], ref["f_min"], ref["f_max"], 5e-3)
    assert near.mean() <= 0.01
    assert 0 < int(ref["flag"].sum()) < wp.SOLVER_B
    eng = pkg.Engine(cfg, 0)
    t, flag = eng.solve_td(inp["pose"], inp["wrench"])
    err = float(np.abs(t - ref["t"]).max())
    free = ref["flag"] == 0
    balance = float(np.abs(np.einsum("bna,bn->ba", -ref["jac"], t.astype(np.float64)) - inp["wrench"])[free].max())
    note(f"solve_td n={n}", "tension", err), note(f"solve_td n={n}", "balance", balance)
    print(f"solve_td n = {n}: tension {err:.3e}, balance {balance:.3e}, flags differ on {(flag != ref['flag']).sum()} robots, near a bound {near.sum()}")
    assert err < 5e-3
    assert np.array_equal(flag[~near], ref["flag"][~near])
    assert balance < 2e-3
    assert (flag != 0).any() and (flag == 0).any() and t.min() >= ref["f_min"] and t.max() <= ref["f_max"]
    eng.close()


# ---- c. the closed-loop matrix over W ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", list(wp.CELLS))
def test_closed_loop_cell_over_the_wide_box(pkg, oracle, monkeypatch, cell):
    """The cell body is workspace_poses.closed_loop_cell (shared with tests/test_gpu_model_constants.py)."""
    cfg, env, seed = wp.cell_config(pkg, cell)
    wp.closed_loop_cell(pkg, oracle, monkeypatch, cfg, env, seed, TOL64 if cfg.precision == 64 else TOL, RAN, WORST, cell)


# ---- d. the headline launch from W ---------------------------------------------------------------------------------------------
def test_full_size_launch_over_the_wide_box(pkg, oracle):
    """test_full_size_properties_config3's shape (65 536 x 8, FK + TD, 20 steps, a velocity Joy, 200 steps) with poses from W."""
    B = 65536
    rng = np.random.default_rng(9301)
    cfg = pkg.Config(model=pkg.eight_cable_model(), batch=B, stages=3)
    assert pkg.plan_kernel(cfg, 1) == "cdpr_split_kernel<8, false>"
    pose = wp.box_poses(cfg.model, B, rng, "W").astype(np.float32)
    pose[B // 2 - 26: B // 2] = wp.special_poses(cfg.model).astype(np.float32)
    pose[B // 2:] = pose[: B // 2]  # second half duplicates the first
    cmd = rng.uniform(-0.05, 0.05, (B, 8)).astype(np.float32)
    cmd[B // 2:] = cmd[: B // 2]
    eng = pkg.Engine(cfg, 0)
    eng.set_platform_state(pose7=pose)
    eng.update(20)
    eng.set_velocity_command(cmd)
    eng.update(200)
    assert eng.kernel_name == "cdpr_split_kernel<8, false>"
    p, t = eng.platform_state()
    q, qd, eff = eng.joint_states()
    assert np.isfinite(p).all() and np.isfinite(eff).all()
    unit = float(np.abs(np.linalg.norm(p[:, 3:], axis=1) - 1.0).max())
    fk_pose, res, it = eng.fk_state()
    d = quat_diff(fk_pose.astype(np.float64), p.astype(np.float64))
    note("full size", "unit quaternion", unit), note("full size", "fk position", d[:, :3].max()), note("full size", "fk quaternion", d[:, 3:].max()), note("full size", "fk residual", res.max())
    print(f"full size over W: |quat| - 1 {unit:.3e}, FK estimate vs true position {d[:, :3].max():.3e}, quaternion {d[:, 3:].max():.3e}, residual {res.max():.3e}")
    assert unit < 1e-6
    assert np.array_equal(p[: B // 2], p[B // 2:]) and np.array_equal(eff[: B // 2], eff[B // 2:])
    # the estimate against the true pose, as test_full_size_properties_config3 (residual 1e-6, position 5e-6), and its rotation half:
    # the quaternion up to sign at the same 5e-6 (the one-shot solver's figure in (b); the estimator runs 4 full iterations here)
    assert np.all(it == 4) and res.max() < 1e-6
    assert d[:, :3].max() < 5e-6 and d[:, 3:].max() < 5e-6
    ten, flag = eng.td_state()
    assert ten.min() >= 5.0 and ten.max() <= 100.0
    for sl in FULL_SIZE_SLICES + (slice(B // 2 - 128, B // 2),):
        check_slice(pkg, oracle, dict(model=cfg.model, stages=3), sl, pose, [(20, None), (200, cmd)], (p, t, q, qd, eff))
    perm = rng.permutation(4096)
    e2 = pkg.Engine(pkg.Config(model=pkg.eight_cable_model(), batch=4096, stages=3), 0)
    e2.set_platform_state(pose7=pose[:4096][perm])
    e2.update(20)
    e2.set_velocity_command(cmd[:4096][perm])
    e2.update(200)
    assert np.array_equal(e2.platform_state()[0], p[:4096][perm])
    eng.close(), e2.close()


# ---- e. coverage and report ----------------------------------------------------------------------------------------------------
def test_zy_every_family_ran(pkg):
    """The launches of the closed-loop matrix ran on every family of the list (a routing change cannot hollow the module out), and
    the optional-physics cells carry the options they are named for."""
    missing = [fam for fam, (cell, pred) in wp.FAMILIES.items() if not any(pred(k) for k in RAN.get(cell, ()))]
    assert not missing, (f"families that did not run IN THIS PROCESS: {missing}.  This test reads what test_closed_loop_cell_over_the_wide_box "
                         f"recorded: run the whole module in one process (no -k, no single node id, no distributing plugin); only then "
                         f"does a missing family mean a routing change.  Ran: { {c: sorted(v) for c, v in RAN.items()} }")
    assert wp.cell_config(pkg, "lumped")[0].model.leg_inertia > 0 and wp.cell_config(pkg, "joint_stop")[0].model.travel_stop > 0
    assert wp.cell_config(pkg, "per_robot")[0].perRobotCommands


def test_zz_report_measured_agreement():
    """Largest error seen per quantity and cell in this module's run (printed with -s)."""
    for (where, name), err in sorted(WORST.items()):
        print(f"workspace agreement: {where:16s} {name:36s} {err:.3e}")
