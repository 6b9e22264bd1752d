"""The conditions tests/test_gpu_workspace.py relies on, re-established on the fp64 oracle alone (no GPU), with the seeds, boxes
and batches of tests/workspace_poses.py that the GPU module uses - so that a change of seed or box cannot quietly invalidate them.

  sensitivity  every closed-loop cell, run twice from poses one float32 rounding apart: effort within 2e-4 N, twist within 2e-6,
               everything finite.  The inputs are benign: the tolerances of the GPU comparison (TOL: effort 2e-2 N, twist 2e-4)
               are 100x above the oracle's own sensitivity to the rounding of its start pose.
  FK           from seeds near the pose (the tracking regime the step kernels run the estimator in) the oracle converges on all
               but <= 0.5 % of the robots within fkMaxIterations; one-shot FK seeded from the spawn pose does not (79 % over E).
  TD           the robots whose unclamped tension lies within 5e-3 N of a bound - where the infeasibility flag may go either way
               under float32 rounding - are <= 1 % of the batch; the unclamped tensions are recomputed here in float64 numpy
               (pseudo-inverse) and their clamp equals oracle.td_wrench to 1e-9 N; both flag values occur.
"""
import numpy as np
import pytest

import workspace_poses as wp
from parity import clean_env_fixture

clean_env = clean_env_fixture()


@pytest.mark.parametrize("cell", list(wp.CELLS))
def test_oracle_sensitivity_to_one_rounding_of_the_start_pose(pkg, oracle, clean_env, cell):
    cfg, _, seed = wp.cell_config(pkg, cell)
    B, n = cfg.batch, cfg.n_cables
    rng = np.random.default_rng(seed)
    pose = wp.start_poses(cfg.model, B, rng)
    cmds = wp.script_commands(rng, B, n)
    twin = np.nextafter(pose, np.where(np.random.default_rng(seed + 1).random(pose.shape) < 0.5, -np.inf, np.inf).astype(np.float32))
    assert twin.dtype == np.float32 and (twin != pose).all()
    a, targets, limits, force = wp.oracle_script(oracle, cfg, pose.astype(np.float64), cmds)
    b, _, _, _ = wp.oracle_script(oracle, cfg, twin.astype(np.float64), cmds, targets)
    worst = dict.fromkeys(("pose", "twist", "q", "qd", "eff"), 0.0)
    for sa, sb in zip(a, b):
        for name, x, y in zip(worst, sa, sb):
            assert np.isfinite(x).all() and np.isfinite(y).all(), (cell, name)
            worst[name] = max(worst[name], float(np.abs(x - y).max()))
    print(f"sensitivity {cell:12s} " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst["eff"] <= 2e-4 and worst["twist"] <= 2e-6, (cell, worst)
    # the joint-stop cell: its stops stay out of play (a stop is a threshold float32 and float64 may cross a step apart:
    # test_travel_stop_against_the_oracle covers contact); the cell is about the kinematics of that instantiation
    assert all((m == 0).all() for m in limits), cell
    if force is not None:
        # Force mode with the tension distribution on: the commanded forces are known, so the unclamped tensions follow from the
        # oracle's Jacobian at its estimate; their clamp is what the oracle applied, and few robots sit within 5e-3 N of a bound
        st = cfg.to_struct()
        lo, hi = float(st.td_f_min), float(st.td_f_max)
        at, ot, of = force
        jac = np.array([oracle.ik(st, p)[3] for p in at])
        unc = wp.unclamped_tensions(jac, -np.einsum("bna,bn->ba", jac, cmds["force"].astype(np.float64)), lo, hi)
        assert np.abs(np.clip(unc, lo, hi) - ot).max() < 1e-9, cell
        assert wp.near_bound(unc, lo, hi, 5e-3).mean() <= 0.01 and (of != 0).any(), cell


def test_twin_rows_are_negated_quaternions(pkg):
    m = pkg.eight_cable_model()
    pose = wp.start_poses(m, 130, np.random.default_rng(1))
    rows, twins = wp.twin_rows(130)
    assert len(rows) == wp.N_TWINS + wp.N_SPECIAL and len(set(rows) | set(twins)) == 2 * len(rows)
    assert np.array_equal(pose[rows, :3], pose[twins, :3]) and np.array_equal(pose[rows, 3:], -pose[twins, 3:])
    assert np.abs(np.linalg.norm(pose[:, 3:], axis=1) - 1.0).max() < 2e-7
    w = wp.BOXES["W"]
    assert np.abs(pose[:, :2]).max() <= w["dxy"] + 1e-7 and pose[:, 2].min() >= w["zlo"] - 1e-7 and pose[:, 2].max() <= w["zhi"] + 1e-7


@pytest.mark.parametrize("n", [8, 12])
def test_oracle_fk_converges_from_near_seeds(pkg, oracle, n):
    cfg, inp, ref = wp.solver_reference(pkg, oracle, n)
    assert cfg.fkMaxIterations == 8 and ref["fk_tolerance"] == 1e-6
    failed = ref["res"] >= ref["fk_tolerance"]
    print(f"FK n = {n}: not converged {failed.mean():.4f}, iterations up to {ref['it'][~failed].max()}")
    assert failed.mean() <= 0.005
    ok = ~failed
    assert np.abs(ref["est"][ok, :3] - inp["pose"][ok, :3]).max() < 5e-6
    assert np.abs(np.abs((ref["est"][ok, 3:] * inp["pose"][ok, 3:]).sum(axis=1)) - 1.0).max() < 1e-6
    assert ((ref["est"][ok, 3:] * inp["pose"][ok, 3:]).sum(axis=1) < 0).any()  # (negated seeds stay negated)


@pytest.mark.parametrize("n", [8, 12])
def test_float32_fk_exit_class(pkg, oracle, n):
    """What float32 arithmetic can meet in one-shot FK with a tolerance-controlled exit, shown on the oracle's own arithmetic in
    numpy float32 (workspace_poses.fk_float32), no kernel involved.  The exit class (workspace_poses.fk_exit_class) is defined on
    the fp64 oracle alone: robots whose residual passes within 2e-7 m (3 ulp of a cable length) of fkTolerance at some iteration.
    Outside it the float32 emulation takes the oracle's number of iterations and agrees with it within 5e-6; inside it the two may
    leave one iteration apart, the one that left early keeps a residual of up to 1e-6 m, and the estimates differ by up to
    1e-6 / sigma_min(J) in orientation (6.9e-6 at n = 8 and 1.40e-5 at n = 12 when this was written; printed with -s).
    tests/test_gpu_workspace.py holds the kernel to 2 x this emulation's worst distance on that class and to 5e-6 elsewhere."""
    cfg, inp, ref = wp.solver_reference(pkg, oracle, n)
    est, res, it = wp.fk_float32(cfg.to_struct(), ref["lengths32"], inp["seed"])
    d = np.abs(est - ref["est"])
    d[:, 3:] = np.minimum(d[:, 3:], np.abs(est[:, 3:] + ref["est"][:, 3:]))
    d = d.max(axis=1)
    exit_class = wp.fk_exit_class(ref)
    flipped = it != ref["it"]
    print(f"float32 FK n = {n}: outside the exit class {d[~exit_class].max():.3e}, inside ({exit_class.sum()} robots, {flipped.sum()} leave "
          f"an iteration apart) {d[exit_class].max():.3e}")
    assert np.abs(it - ref["it"]).max() <= 1 and res.max() < 1e-6
    assert flipped.any() and not flipped[~exit_class].any()
    assert exit_class.mean() <= 0.05
    assert d[~exit_class].max() < 5e-6
    sigma_min = min(np.linalg.svd(ref["jac"][r], compute_uv=False)[-1] for r in np.flatnonzero(flipped))
    assert d[exit_class].max() <= 1e-6 / sigma_min


@pytest.mark.parametrize("n", [8, 12])
def test_oracle_td_margin_to_the_bounds(pkg, oracle, n):
    cfg, inp, ref = wp.solver_reference(pkg, oracle, n)
    lo, hi = ref["f_min"], ref["f_max"]
    assert np.abs(np.clip(ref["unclamped"], lo, hi) - ref["t"]).max() <= 1e-9
    flag = ((ref["unclamped"] < lo) | (ref["unclamped"] > hi)).any(axis=1)
    near = wp.near_bound(ref["unclamped"], lo, hi, 5e-3)
    assert np.array_equal(flag[~near], ref["flag"][~near] != 0)
    print(f"TD n = {n}: flagged {flag.mean():.3f}, within 5e-3 N of a bound {near.mean():.4f}")
    assert near.mean() <= 0.01
    assert 0 < ref["flag"].sum() < len(flag)  # both branches
    # unflagged robots balance the wrench
    w = np.einsum("bna,bn->ba", -ref["jac"], ref["t"])
    assert np.abs(w - inp["wrench"])[ref["flag"] == 0].max() < 1e-9
