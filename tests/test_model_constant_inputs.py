"""The conditions tests/test_gpu_model_constants.py relies on, established on the fp64 oracle alone (no GPU) for every set of
tests/model_constants.py x every cell of workspace_poses.CELLS, with the cell's own seed, poses and commands.

  benign  two oracle runs from start poses one float32 rounding apart (the construction of tests/test_workspace_inputs.py):
          everything finite, effort within 4e-4 N (1 / 50 of TOL["eff"]), twist within 2e-6 (the workspace module's bound).
  teeth   each varied constant in turn back at its shipped value, the rest of the set kept (model_constants.teeth: mass; the whole
          inertia; its off-diagonals alone 0; the isotropic tensor of the same trace; damping; gravity's x and y 0; dt where the set
          changes it): the oracle's observables over the script move by at least 20 x the tolerance of the GPU comparison
          (model_constants.tolerance on parity.TOL, for the precision = 64 cells as well: the stricter reading) in at least one of
          pose, twist, q, qd, eff.  A kernel that ignores or misuses the constant then cannot pass the GPU comparison.  The home pose
          of S: reference_lengths() differs from the shipped model's by more than 20 x TOL["q"] on some cable.
  TD      cells with the tension distribution: at most 1 % of the robots within 5e-3 N of a tension bound in the Force segment,
          the clamp of the unclamped tensions (float64 numpy) is what the oracle applied, both flag values occur; the joint-stop
          cell reaches no stop.
Each case prints its sensitivities and its teeth ratios (-s).
"""
from dataclasses import replace

import numpy as np
import pytest

import launch_forms as lf
import model_constants as mc
import parity
import robot_histories as ri
import workspace_poses as wp
from parity import NAMES, TOL, clean_env_fixture

clean_env = clean_env_fixture()

MARGIN = 20.0  # x the tolerance a shipped constant must move some observable by
_runs = {}


def base_run(pkg, oracle, name, cell):
    """The set's own run of the cell's script on the oracle, from the poses and commands workspace_poses.closed_loop_cell draws for that
    Config: computed once, shared by the tests of the case, left unchanged."""
    if (name, cell) not in _runs:
        cfg, _, seed = mc.cell_config(pkg, cell, name)
        rng = np.random.default_rng(seed)
        pose = wp.start_poses(cfg.model, cfg.batch, rng)
        cmds = wp.script_commands(rng, cfg.batch, cfg.n_cables)
        _runs[(name, cell)] = (cfg, seed, pose, cmds) + wp.oracle_script(oracle, cfg, pose.astype(np.float64), cmds)
    return _runs[(name, cell)]


def moved(a, b):
    """{quantity: largest |a - b| over the segments}"""
    out = dict.fromkeys(NAMES, 0.0)
    for sa, sb in zip(a, b):
        for key, x, y in zip(NAMES, sa, sb):
            assert np.isfinite(x).all() and np.isfinite(y).all(), key
            out[key] = max(out[key], float(np.abs(x - y).max()))
    return out


CASES = [(name, cell) for name in mc.SETS for cell in wp.CELLS]


@pytest.mark.parametrize("name,cell", CASES, ids=[f"{s} {c}" for s, c in CASES])
def test_benign_under_the_set(pkg, oracle, clean_env, name, cell):
    cfg, seed, pose, cmds, a, targets, limits, force = base_run(pkg, oracle, name, cell)
    twin = np.nextafter(pose, np.where(np.random.default_rng(seed + 1).random(pose.shape) < 0.5, -np.inf, np.inf).astype(np.float32))
    assert twin.dtype == np.float32 and (twin != pose).all()
    b, _, _, _ = wp.oracle_script(oracle, cfg, twin.astype(np.float64), cmds, targets)
    worst = moved(a, b)
    rate = max(float(np.abs(s[1][:, 3:]).max()) for s in a)
    on_limit = max(float((np.abs(s[4]) >= cfg.model.effort_limit).mean()) for s in a)
    print(f"sensitivity {name} {cell:12s} " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f"  |w| up to {rate:.2f} rad/s, efforts on the limit {on_limit:.3f}")
    assert worst["eff"] <= 4e-4 and worst["twist"] <= 2e-6, (name, cell, worst)


@pytest.mark.parametrize("name,cell", CASES, ids=[f"{s} {c}" for s, c in CASES])
def test_every_constant_has_teeth(pkg, oracle, clean_env, name, cell):
    cfg, seed, pose, cmds, a, targets, _, _ = base_run(pkg, oracle, name, cell)
    tol = mc.tolerance(replace(cfg, precision=32))  # (the fp32 bound on the precision = 64 cells as well: the stricter reading)
    weak = []
    for what, model_kw, config_kw in mc.teeth(name):
        other = mc.apply(wp.cell_config(pkg, cell)[0], name, model_kw, config_kw)
        b, _, _, _ = wp.oracle_script(oracle, other, pose.astype(np.float64), cmds, targets)
        ratio = {k: v / tol[k] for k, v in moved(a, b).items()}
        best = max(ratio, key=ratio.get)
        print(f"teeth {name} {cell:12s} {what:38s} {best} moves by {ratio[best]:9.1f} x its tolerance")
        if ratio[best] < MARGIN:
            weak.append((what, ratio))
    assert not weak, (name, cell, weak)


@pytest.mark.parametrize("name,cell", CASES, ids=[f"{s} {c}" for s, c in CASES])
def test_tension_distribution_and_joint_stop_under_the_set(pkg, oracle, clean_env, name, cell):
    cfg, seed, pose, cmds, a, targets, limits, force = base_run(pkg, oracle, name, cell)
    assert all((m == 0).all() for m in limits), (name, cell)
    assert (force is not None) == bool(cfg.stages & 2)
    if force is not None:
        st = cfg.to_struct()
        lo, hi = float(st.td_f_min), float(st.td_f_max)
        at, ot, of = force
        jac = wp.oracle_jacobians(oracle, st, at)
        unc = wp.unclamped_tensions(jac, -np.einsum("bna,bn->ba", jac, cmds["force"].astype(np.float64)), lo, hi)
        near = wp.near_bound(unc, lo, hi, 5e-3)
        print(f"TD {name} {cell:12s} within 5e-3 N of a bound {near.mean():.4f}, flagged {(of != 0).mean():.3f}")
        assert np.abs(np.clip(unc, lo, hi) - ot).max() < 1e-9, (name, cell)
        assert near.mean() <= 0.01, (name, cell, float(near.mean()))
        assert (of != 0).any() and (of == 0).any(), (name, cell)


@pytest.mark.parametrize("kind", mc.ROLLOUT_KINDS)
def test_rollout_costs_under_S_have_teeth(pkg, oracle, monkeypatch, kind):
    """The inputs of the GPU module's rollout case on the oracle alone: the costs are finite, one float32 rounding of the start poses
    moves them by less than 1 / 50 of launch_forms.rollout_tolerance on the fp32 kinds, and each of mass, the whole inertia, damping,
    gravity's x and y and dt back at its shipped value moves them by at least 20 x that tolerance - a rollout instantiation that
    folds one of them fails the GPU comparison.  The off-diagonals of the inertia alone move the fp32 costs by less (7 x, printed):
    a sum of squared POSITION errors over 14 steps sees little of the rotation; the matrix of tests/test_gpu_model_constants.py,
    not the rollout, holds the rotation to account."""
    def costs(model_kw=None, config_kw=None, pose=None):
        cfg, h, start, roll = mc.rollout_case(pkg, kind, monkeypatch, model_kw, config_kw)
        ora = parity.oracle_at(oracle, cfg, start if pose is None else pose)
        ri.play_history([ora], h)
        out = ora.rollout_velocity(roll["cmds"], roll["ref"].astype(np.float64))
        ora.close()
        return cfg, start, out

    cfg, pose, want = costs()
    assert cfg.dt == 2e-3 and np.isfinite(want).all()
    bound = lf.rollout_tolerance(cfg, kind in lf.GENERAL, want)
    twin = np.nextafter(pose, np.where(np.random.default_rng(7).random(pose.shape) < 0.5, -np.inf, np.inf).astype(np.float32))
    sens = float(np.abs(costs(pose=twin)[2] - want).max()) / bound
    ratios = {what: float(np.abs(costs(model_kw, config_kw)[2] - want).max()) / bound for what, model_kw, config_kw in mc.teeth("S")}
    print(f"rollout under S, {kind}: costs up to {np.abs(want).max():.3e}, tolerance {bound:.2e}, one rounding of the start poses {sens:.4f} x, " + ", ".join(f"{k} {v:.1f} x" for k, v in ratios.items()))
    assert cfg.precision == 64 or sens <= 0.02, sens
    weak = {k: v for k, v in ratios.items() if v < MARGIN and not k.startswith("inertia, ")}
    assert not weak and len(ratios) == 7, weak


def test_the_home_pose_of_S_moves_the_reference_lengths(pkg):
    for n in sorted({v[0] for v in wp.CELLS.values()}):
        shipped = wp.cell_model(pkg, n)
        moved_home = mc.apply(pkg.Config(model=shipped), "S").model
        d = np.abs(moved_home.reference_lengths() - shipped.reference_lengths())
        print(f"home pose of S, n = {n}: reference lengths move by up to {d.max():.3e} m = {d.max() / TOL['q']:.0f} x TOL[q]")
        assert d.max() > MARGIN * TOL["q"], (n, d)
    assert np.array_equal(mc.apply(pkg.Config(model=wp.cell_model(pkg, 8)), "M").model.home_pose(), wp.cell_model(pkg, 8).home_pose())


def test_the_sets_and_the_tolerance(pkg):
    """Every set leaves each varied constant off its shipped value (dt and the home pose where the table says so), its tensor is
    positive definite and anisotropic; the tolerance widens the effort alone, by 1e-3 / dt, and only upwards."""
    for name, s in mc.SETS.items():
        cfg = mc.apply(pkg.Config(model=pkg.eight_cable_model()), name)
        m = cfg.model
        assert m.mass != mc.DEFAULTS["mass"] and m.joint_damping != mc.DEFAULTS["joint_damping"] and cfg.gravity[0] != 0.0 and cfg.gravity[1] != 0.0
        xx, yy, zz, xy, xz, yz = m.inertia
        ev = np.linalg.eigvalsh(np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]]))
        assert ev.min() > 0.05 and np.diff(ev).min() > 0.02 and min(abs(xy), abs(xz), abs(yz)) > 0.0 and len({abs(xy), abs(xz), abs(yz)}) == 3
        tol = mc.tolerance(cfg)
        assert tol == dict(TOL, eff=TOL["eff"] * max(1.0, 1e-3 / cfg.dt))
        tol64 = mc.tolerance(mc.apply(pkg.Config(model=pkg.eight_cable_model(), precision=64), name))
        assert tol64 == dict(mc.TOL64, eff=mc.TOL64["eff"] * max(1.0, 1e-3 / cfg.dt))
    assert mc.tolerance(mc.apply(pkg.Config(), "H"))["eff"] == 2 * TOL["eff"] and mc.tolerance(mc.apply(pkg.Config(), "S"))["eff"] == TOL["eff"]
    assert mc.SETS["S"]["model"]["home_position"] != mc.DEFAULTS["home_position"] and mc.SETS["M"]["config"]["dt"] == mc.DEFAULTS["dt"]
