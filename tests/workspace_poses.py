"""Poses across the workspace, and the closed-loop script run from them: shared by tests/test_workspace_inputs.py (CPU: the
oracle-side conditions the GPU tests rely on) and tests/test_gpu_workspace.py (GPU), so that both see the same seeds, boxes and
batches.  A plain module: no fixtures, no pytest hooks.

Boxes (the frame is a 0.6 m cube, the spawn pose is its centre with R = I):
  x, y uniform in +-dxy, z uniform in [zlo, zhi], orientation Rz(yaw) exp(rotvec) with each rotvec component uniform in +-dr and
  yaw uniform in +-yaw.
    W (wide): dxy 0.15, z 0.15 .. 0.45, dr 0.3, yaw pi
    E (edge): dxy 0.20, z 0.10 .. 0.50, dr 0.4, yaw pi
"""
import numpy as np
from scipy.spatial.transform import Rotation

BOXES = {
    "W": dict(dxy=0.15, zlo=0.15, zhi=0.45, dr=0.3, yaw=np.pi),
    "E": dict(dxy=0.20, zlo=0.10, zhi=0.50, dr=0.4, yaw=np.pi),
}


def box_poses(model, B, rng, box):
    """B poses (x y z, quaternion x y z w; float64) drawn from box "W" or "E".  `model` is taken for symmetry with
    special_poses and parity.perturbed_poses: the boxes are stated in frame coordinates."""
    b = BOXES[box]
    pose = np.empty((B, 7))
    pose[:, :2] = rng.uniform(-b["dxy"], b["dxy"], (B, 2))
    pose[:, 2] = rng.uniform(b["zlo"], b["zhi"], B)
    yaw = Rotation.from_euler("z", rng.uniform(-b["yaw"], b["yaw"], B))
    pose[:, 3:] = (yaw * Rotation.from_rotvec(rng.uniform(-b["dr"], b["dr"], (B, 3)))).as_quat()
    return pose


SPECIAL_RPY = ((0.0, 0.0, np.pi), (0.0, 0.0, 0.5 * np.pi), (0.0, 0.0, -0.5 * np.pi))  # + the two tilts, see special_rpy_xyz


def special_rpy_xyz(model, tilt=BOXES["W"]["dr"]):
    """The special poses as (roll, pitch, yaw) and position, 13 of them: yaw pi and +-pi / 2 at the spawn position, the largest
    tilt about x alone and about y alone, the eight corners of W's position box with R = I."""
    home = [float(v) for v in model.home_position]
    w = BOXES["W"]
    out = [(rpy, home) for rpy in SPECIAL_RPY + ((tilt, 0.0, 0.0), (0.0, tilt, 0.0))]
    for x in (-w["dxy"], w["dxy"]):
        for y in (-w["dxy"], w["dxy"]):
            for z in (w["zlo"], w["zhi"]):
                out.append(((0.0, 0.0, 0.0), [x, y, z]))
    return out


def special_poses(model, tilt=BOXES["W"]["dr"]):
    """26 poses: the 13 of special_rpy_xyz with quaternions written out in closed form (yaw exactly pi is (0, 0, 1, 0): w = 0, no
    rounding of cos(pi / 2)), then the same 13 with the quaternion negated (the same rotation; row k + 13 is the twin of row k)."""
    h = np.sqrt(0.5)
    quats = [(0.0, 0.0, 1.0, 0.0), (0.0, 0.0, h, h), (0.0, 0.0, -h, h),
             (np.sin(0.5 * tilt), 0.0, 0.0, np.cos(0.5 * tilt)), (0.0, np.sin(0.5 * tilt), 0.0, np.cos(0.5 * tilt))] + [(0.0, 0.0, 0.0, 1.0)] * 8
    pose = np.array([list(xyz) + list(q) for (_, xyz), q in zip(special_rpy_xyz(model, tilt), quats)])
    twin = pose.copy()
    twin[:, 3:] = -twin[:, 3:]
    return np.concatenate([pose, twin])


N_SPECIAL = 13
N_TWINS = 20  # box poses repeated with the quaternion negated in start_poses


def start_poses(model, B, rng, box="W"):
    """The batch a closed-loop cell starts from, rounded to float32: B - 26 - N_TWINS poses from the box, N_TWINS of them once
    more with the quaternion negated, then special_poses.  twin_rows() names the (q, -q) pairs."""
    nbox = B - 2 * N_SPECIAL - N_TWINS
    assert nbox >= N_TWINS
    p = box_poses(model, nbox, rng, box)
    neg = p[:N_TWINS].copy()
    neg[:, 3:] = -neg[:, 3:]
    return np.concatenate([p, neg, special_poses(model)]).astype(np.float32)


def twin_rows(B):
    """(rows, rows of their twins): start_poses(...)[twins] is start_poses(...)[rows] with the quaternion negated."""
    nbox = B - 2 * N_SPECIAL - N_TWINS
    rows = np.concatenate([np.arange(N_TWINS), nbox + N_TWINS + np.arange(N_SPECIAL)])
    twins = np.concatenate([nbox + np.arange(N_TWINS), nbox + N_TWINS + N_SPECIAL + np.arange(N_SPECIAL)])
    return rows, twins


def near_seeds(pose, rng, dp=0.03, dr=0.1):
    """Estimator seeds within +-dp and +-dr (rotation vector, world frame) of the poses, every second one with the quaternion
    negated: the tracking regime the step kernels run FK in (the estimate of the step before)."""
    seed = np.array(pose, dtype=np.float64)
    B = seed.shape[0]
    seed[:, :3] += rng.uniform(-dp, dp, (B, 3))
    seed[:, 3:] = (Rotation.from_rotvec(rng.uniform(-dr, dr, (B, 3))) * Rotation.from_quat(seed[:, 3:])).as_quat()
    seed[1::2, 3:] = -seed[1::2, 3:]
    return seed


# ---- the closed-loop script ---------------------------------------------------------------------------------------------------
# hold 5, velocity 30, position 30 (targets = the oracle's current q + offset), force 20, velocity 25
SCRIPT = (("hold", 5), ("velocity", 30), ("position", 30), ("force", 20), ("velocity", 25))
SETTER = {"velocity": "set_velocity_command", "position": "set_position_command", "force": "set_force_command"}


def script_commands(rng, B, n):
    """Per-robot commands of the script, float32: two velocity Joys (+-0.03 m/s), position offsets (+-0.004 m), forces (2 .. 6 N).
    The -q twins of start_poses hear what their robots hear."""
    v, v2 = (rng.uniform(-0.03, 0.03, (B, n)).astype(np.float32) for _ in range(2))
    off = rng.uniform(-0.004, 0.004, (B, n)).astype(np.float32)
    f = rng.uniform(2.0, 6.0, (B, n)).astype(np.float32)
    rows, twins = twin_rows(B)
    for arr in (v, v2, off, f):
        arr[twins] = arr[rows]
    return {"velocity": [v, v2], "position": off, "force": f}


def segment_command(kind, cmds, ora, used):
    """The command of one segment (None for "hold").  Position targets are the oracle's current joint positions plus the offset,
    rounded to float32: the one array goes to every simulator."""
    if kind == "hold":
        return None
    if kind == "velocity":
        used["velocity"] = used.get("velocity", -1) + 1
        return cmds["velocity"][used["velocity"]]
    if kind == "position":
        return (ora.joint_states()[0] + cmds["position"]).astype(np.float32)
    return cmds["force"]


def unclamped_tensions(jac, wrench, f_min, f_max):
    """The tension distribution before its clamp, in float64 numpy: T = Tm 1 + A^+ (w - A Tm 1) with A = -J^T and Tm the middle of
    [f_min, f_max] (least-norm solution by the pseudo-inverse; jac[B, n, 6], wrench[B, 6])."""
    tm = 0.5 * (f_min + f_max)
    out = np.empty(jac.shape[:2])
    for r in range(jac.shape[0]):
        a = -jac[r].T
        out[r] = tm + np.linalg.pinv(a) @ (wrench[r] - a @ np.full(jac.shape[1], tm))
    return out


def near_bound(t, f_min, f_max, margin):
    """Robots with some tension within `margin` of a bound of the clamp (a flag there may go either way under rounding)."""
    return ((np.abs(t - f_min) < margin) | (np.abs(t - f_max) < margin)).any(axis=1)


def oracle_script(oracle, cfg, pose, cmds, targets=None):
    """The script on the oracle alone from `pose` (tests/test_workspace_inputs.py, tests/test_model_constant_inputs.py); returns the
    observables after every segment, the position targets used, the travel-limit masks and, with the tension distribution on, (the
    pose it saw, its tensions, its flags) of the Force segment.  `targets`: position targets of an earlier run (twin runs share
    their commands)."""
    ora = oracle.OracleSim(cfg.to_struct(), oracle.DERIV_EXACT)
    ora.set_platform_state(pose7=pose)
    used, out, tg, limits, force = {}, [], None, [], None
    for kind, k in SCRIPT:
        cmd = segment_command(kind, cmds, ora, used)
        if kind == "position":
            cmd = tg = cmd if targets is None else targets
        if cmd is not None:
            getattr(ora, SETTER[kind])(cmd)
        ora.update(k)
        out.append(ora.platform_state() + ora.joint_states())
        limits.append(ora.limit_state())
        if kind == "force" and cfg.stages & 2:  # the pose the tension distribution saw, its tensions and flags
            force = (ora.fk_state()[0] if cfg.stages & 1 else ora.platform_state()[0],) + ora.td_state()
    ora.close()
    return out, tg, limits, force


# ---- the cells of the closed-loop matrix (tests/test_gpu_workspace.py, section c) ---------------------------------------------
# name: (cables, Config keywords beyond model / batch, environment switches, batch, seed).  Models: 4 = cube_model, 8 =
# eight_cable_model, 12 = twelve_cable_model, else the first n anchors of twelve_cable_model (as tests/test_gpu_cable_counts.py).
LUMPED = dict(passive_damping=0.01, leg_inertia=0.004, cable_axial_mass=0.001, anchor_point_mass=0.002, anchor_inertia=0.001)
CELLS = {
    "step":        (8, dict(stages=3, mapping="robot"), {"CDPR_ONESTEP": "1"}, 130, 9101),
    "step_n6":     (6, dict(stages=0, mapping="robot"), {}, 130, 9102),
    "lowreg":      (8, dict(stages=3, mapping="robot"), {"CDPR_LOWREG": "1"}, 130, 9103),
    "onestep":     (8, dict(stages=3, mapping="robot"), {"CDPR_SPLIT": "0"}, 130, 9104),
    "split":       (8, dict(stages=3), {}, 130, 9105),
    "pair":        (8, dict(stages=3, mapping="pair"), {}, 130, 9106),
    "pair_stream": (4, dict(stages=0), {}, 130, 9107),
    "cable":       (8, dict(stages=3, mapping="cable"), {}, 130, 9108),
    "gen_step":    (8, dict(stages=3, velocityEpsilon=0.004), {"CDPR_GEN_SPLIT": "0"}, 130, 9109),
    "gen_split":   (8, dict(stages=3, velocityEpsilon=0.004), {}, 130, 9110),
    "gen_lean":    (8, dict(stages=3, velocityEpsilon=0.004), {"CDPR_GEN_SPLIT": "0", "CDPR_GEN_LEAN": "1"}, 130, 9111),
    "f64_step":    (8, dict(stages=1, precision=64), {}, 130, 9112),
    "f64_split":   (8, dict(stages=3, precision=64), {}, 130, 9113),
    "per_robot":   (8, dict(stages=3, perRobotCommands=True), {}, 130, 9114),
    "lumped":      (8, dict(stages=3, model_kw=LUMPED), {}, 130, 9115),
    "joint_stop":  (8, dict(stages=3, model_kw=dict(travel_lower=-0.6, travel_upper=0.6, travel_stop=2)), {}, 130, 9116),
    "n9":          (9, dict(stages=3), {}, 130, 9117),
    "n10":         (10, dict(stages=0), {}, 130, 9118),
    "n11":         (11, dict(stages=3), {}, 130, 9119),
    "n12":         (12, dict(stages=3), {}, 130, 9120),
    "n12_f64":     (12, dict(stages=3, precision=64), {}, 130, 9121),
}


# kernel family or handle kind -> (cell, predicate on a kernel name).  The lumped legs and the joint stop are two options of ONE
# kernel (the PHYS instantiations): their cells differ in the configuration, which the test_zy_every_family_ran of tests/test_gpu_workspace.py and tests/test_gpu_pid_limits.py check, not in the name.
# The joint-stop cell runs the stop's sweeps every step with limits no joint reaches (test_workspace_inputs asserts it): a stop is a
# threshold float32 and float64 may cross a step apart, so contact stays with test_travel_stop_against_the_oracle.
FAMILIES = {
    "cdpr_step_kernel (plain)": ("step", lambda k: k == "cdpr_step_kernel<8, true, true, SINGLE>"),
    "cdpr_step_kernel (several steps)": ("step", lambda k: k == "cdpr_step_kernel<8, true, true>"),
    "cdpr_step_kernel (low-register)": ("lowreg", lambda k: k.startswith("cdpr_step_kernel<8,") and "LOWREG" in k),
    "cdpr_onestep_kernel": ("onestep", lambda k: k.startswith("cdpr_onestep_kernel<8,")),
    "cdpr_split_kernel": ("split", lambda k: k == "cdpr_split_kernel<8, false>"),
    "cdpr_step_kernel_pair": ("pair", lambda k: k.startswith("cdpr_step_kernel_pair<8, true, true")),
    "cdpr_pair_stream_kernel": ("pair_stream", lambda k: k.startswith("cdpr_pair_stream_kernel<")),
    "lane-per-cable": ("cable", lambda k: k.startswith("cdpr_step_kernel_cable<8,")),
    "cdpr_gen_step_kernel": ("gen_step", lambda k: k.startswith("cdpr_gen_step_kernel<8,")),
    "cdpr_gen_split_kernel": ("gen_split", lambda k: k.startswith("cdpr_gen_split_kernel<8>")),
    "cdpr_gen_lean_kernel": ("gen_lean", lambda k: k.startswith("cdpr_gen_lean_kernel<8>")),
    "cdpr_step_kernel_f64": ("f64_step", lambda k: k.startswith("cdpr_step_kernel_f64<8")),
    "cdpr_split_kernel_f64": ("f64_split", lambda k: k.startswith("cdpr_split_kernel_f64<8")),
    "per-robot handle (role-split)": ("per_robot", lambda k: k == "cdpr_split_kernel<8, true>"),
    "per-robot handle (several steps)": ("per_robot", lambda k: k.startswith("cdpr_step_kernel<8,") and k.endswith(", PR>")),
    "lumped-leg physics": ("lumped", lambda k: k.startswith("cdpr_step_kernel<8,") and "PHYS" in k),
    "joint stop (the same PHYS kernel, travel_stop sweeps on)": ("joint_stop", lambda k: k.startswith("cdpr_step_kernel<8,") and "PHYS" in k),
    "nine cables": ("n9", lambda k: k.startswith("cdpr_step_kernel<9,")),
    "ten cables": ("n10", lambda k: k.startswith("cdpr_step_kernel<10,")),
    "eleven cables": ("n11", lambda k: k.startswith("cdpr_step_kernel<11,")),
    "twelve cables": ("n12", lambda k: k.startswith("cdpr_step_kernel<12,")),
    "twelve cables, precision = 64": ("n12_f64", lambda k: k.startswith("cdpr_step_kernel_f64<12")),
}


def cell_model(pkg, n, **model_kw):
    from dataclasses import replace

    if n == 4:
        m = pkg.cube_model()
    elif n == 8:
        m = pkg.eight_cable_model()
    else:
        m = pkg.twelve_cable_model()
        if n != 12:
            m = replace(m, frame_anchors=m.frame_anchors[:n], platform_anchors=m.platform_anchors[:n])
    return replace(m, **model_kw) if model_kw else m


def cell_config(pkg, name, batch=None):
    """(Config, environment switches, seed) of a cell."""
    n, kw, env, B, seed = CELLS[name]
    kw = dict(kw)
    mapping = kw.pop("mapping", None)
    if mapping:
        kw["mapping"] = {"robot": pkg._abi.MAP_LANE_PER_ROBOT, "pair": pkg._abi.MAP_LANE_PAIR, "cable": pkg._abi.MAP_LANE_PER_CABLE}[mapping]
    model = cell_model(pkg, n, **kw.pop("model_kw", {}))
    return pkg.Config(model=model, batch=batch or B, **kw), env, seed


# ---- the body of a closed-loop cell (tests/test_gpu_workspace.py, section c; tests/test_gpu_model_constants.py, section a) ------
FIRST, NOT_STEADY = 1, 8  # CDPR_PLAN_* (include/cdpr.h)


def oracle_jacobians(oracle, s, poses):
    return np.array([oracle.ik(s, p)[3] for p in poses])


def closed_loop_cell(pkg, oracle, monkeypatch, cfg, env, seed, tol, ran, worst, label):
    """The script on three engines (one step per launch, fused, recorded) and the oracle from start_poses, under the environment
    switches `env`: the oracle after every segment at `tol` (a dictionary over parity.NAMES), one-step = fused = recorded bit for
    bit, kernel_name = plan_kernel, FK iteration counts and estimates, TD tensions and flags with the near-bound rule, the
    Force-mode tension reconstruction, (q, -q) twins.  ran[label] collects the kernel names, worst[(label, quantity)] the largest
    error seen.  pytest rewrites asserts only in test modules, so every assert here carries its message."""
    from parity import TOL, observed, state_of, worst_errors

    def note(name, err):
        worst[(label, name)] = max(worst.get((label, name), 0.0), float(err))

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    B, n, f64, stages = cfg.batch, cfg.n_cables, cfg.precision == 64, cfg.stages
    s = cfg.to_struct()
    rng = np.random.default_rng(seed)
    pose = start_poses(cfg.model, B, rng)
    cmds = script_commands(rng, B, n)
    rows, twins = twin_rows(B)
    pkg.plan_kernel(cfg, 1)
    # a: one step per launch; b: fused (10 per launch); c: the trajectory record
    engs = [pkg.Engine(cfg, 0) for _ in range(3)]
    a, b, c = engs
    ora = oracle.OracleSim(cfg.to_struct(), oracle.DERIV_EXACT)
    for e in engs:
        e.set_platform_state_f64(pose7=pose.astype(np.float64)) if f64 else e.set_platform_state(pose7=pose)
    ora.set_platform_state(pose7=pose.astype(np.float64))
    names = ran.setdefault(label, set())
    used = {}
    failures = []
    for kind, k in SCRIPT:
        where = f"{label}, {kind}"
        cmd = segment_command(kind, cmds, ora, used)
        if cmd is not None:
            for sim in (a, b, c, ora):
                getattr(sim, SETTER[kind])(cmd)
        a.update(k)
        b.update(k, 10)
        rec = c.update_record(k, 10)
        ora.update(k)
        # what ran = what was planned (as test_cable_count_matrix)
        flags = (FIRST | NOT_STEADY) if kind == "hold" else NOT_STEADY if kind == "force" else 0
        last = k - 10 * ((k - 1) // 10)
        assert a.kernel_name == pkg.plan_kernel(cfg, 1), (where, a.kernel_name)
        planned = pkg.plan_kernel(cfg, last, flags)
        if kind == "hold" and pkg.plan_kernel(cfg, 10).startswith(("cdpr_gen_split", "cdpr_gen_lean")):
            planned = pkg.plan_kernel(cfg, 1, NOT_STEADY)  # (these handles run a fused update as one-step launches: the last one does not start at world step 0)
        assert b.kernel_name == planned == c.kernel_name, (where, b.kernel_name, planned, c.kernel_name)
        names.update((a.kernel_name, b.kernel_name))
        # the oracle
        got = observed(a, f64)
        for name, (err, robot, _) in worst_errors(got, observed(ora), where, f64=f64).items():
            note(name, err)
            if err > tol[name]:
                failures.append(f"{where}: {name} differs from the oracle by {err:.3e} (tolerance {tol[name]:.1e}, robot {robot})")
        # launch forms
        sa = state_of(a, f64)
        for e, form in ((b, "fused"), (c, "recorded")):
            for x, y in zip(sa, state_of(e, f64)):
                assert np.array_equal(x, y), f"{where}: {form} launches differ from one-step launches"
        for j, key in enumerate(("position", "velocity", "effort", "pose", "twist")):
            assert np.array_equal(rec[key][-1], sa[2 + j]), f"{where}: the record's last step is not the published one ({key})"
        # a robot and its twin started from the negated quaternion
        gp, gt, gq, gqd, ge = got
        for name, x in (("q", gq), ("qd", gqd), ("effort", ge), ("twist", gt), ("position", gp[:, :3])):
            assert np.array_equal(x[rows], x[twins]), f"{where}: {name} of a robot and of its -q twin differ"
        assert np.array_equal(gp[rows, 3:], -gp[twins, 3:]), f"{where}: published quaternions of twins are not exact negatives"
        if stages & 1:
            fp, fr, fi = a.fk_state()
            op, orr, oi = ora.fk_state()
            err = float(np.abs(fp - op).max())
            note("fk estimate", err)
            assert np.array_equal(fi, oi), f"{where}: FK iteration counts"
            if err > 1e-5:
                failures.append(f"{where}: FK estimate differs from the oracle's by {err:.3e} (robot {int(np.abs(fp - op).max(axis=1).argmax())})")
        if stages & 2:
            tt, tf = a.td_state()
            ot, of = ora.td_state()
            err = float(np.abs(tt - ot).max())
            note("tension", err)
            if err > TOL["eff"]:
                failures.append(f"{where}: tensions differ by {err:.3e}")
            lo, hi = float(s.td_f_min), float(s.td_f_max)
            near = near_bound(ot, lo, hi, 2e-2)  # (a clamped value sits on its bound)
            differ = tf != of
            note("flags differ (share)", differ.mean())
            assert not differ[~near].any(), f"{where}: infeasibility flags differ away from the bounds"
            assert differ.mean() <= 0.01, f"{where}: flags differ on {differ.sum()} robots"
            if kind == "force":
                # the commanded forces are known: the unclamped tensions follow from the oracle's Jacobian at its estimate
                at = ora.fk_state()[0] if stages & 1 else ora.platform_state()[0]
                jac = oracle_jacobians(oracle, s, at)
                wd = -np.einsum("bna,bn->ba", jac, cmd.astype(np.float64))
                unc = unclamped_tensions(jac, wd, lo, hi)
                assert np.abs(np.clip(unc, lo, hi) - ot).max() < 1e-9, where
                near5 = near_bound(unc, lo, hi, 5e-3)
                note("near a bound in force mode (share)", near5.mean())
                assert near5.mean() <= 0.01, (where, float(near5.mean()))
                assert np.array_equal(tf[~near5], of[~near5]), f"{where}: flags differ on robots farther than 5e-3 N from a bound"
                assert (of != 0).any(), where
    assert not failures, "\n".join(failures)
    for e in engs:
        e.close()
    ora.close()


# ---- the one-shot solvers over E (tests/test_gpu_workspace.py, section b) ------------------------------------------------------
SOLVER_B = 500
SOLVER_SEEDS = {8: 9208, 12: 9212}
_SOLVER_CACHE = {}


def solver_inputs(pkg, n):
    """Config (FK with 8 iterations and fkTolerance 1e-6) and float32 inputs of the one-shot solvers: SOLVER_B poses in E, twists,
    estimator seeds near the poses, the wrench to balance (the platform's weight plus noise, as test_solve_td_matches_oracle...)."""
    B = SOLVER_B
    model = cell_model(pkg, n)
    cfg = pkg.Config(model=model, batch=B, stages=3, fkMaxIterations=8, fkTolerance=1e-6)
    rng = np.random.default_rng(SOLVER_SEEDS[n])
    pose = box_poses(model, B, rng, "E").astype(np.float32)
    twist = rng.uniform(-0.3, 0.3, (B, 6)).astype(np.float32)
    seed = near_seeds(pose, rng).astype(np.float32)
    wrench = (np.tile([0, 0, 9.8, 0, 0, 0], (B, 1)) + rng.uniform(-0.5, 0.5, (B, 6)) * [1, 1, 1, 0.02, 0.02, 0.02]).astype(np.float32)
    return cfg, dict(pose=pose, twist=twist, seed=seed, wrench=wrench)


FK_EXIT_MARGIN = 2e-7  # 3 ulp of a cable length in [0.5, 1) m: what a float32 evaluation of max |L* - L| may be off by


def fk_exit_class(ref):
    """Robots on which the oracle's FK tests a residual within FK_EXIT_MARGIN of fkTolerance at some iteration: float32 and float64
    may leave the loop one iteration apart there, and the one that leaves early keeps a residual of up to fkTolerance."""
    return (np.abs(ref["res_seq"] - ref["fk_tolerance"]) <= FK_EXIT_MARGIN).any(axis=1)


def solver_reference(pkg, oracle, n):
    """The oracle's answers on solver_inputs, computed once per session and shared (callers must not write into them): IK (q, qd,
    L, J), the encoder lengths rounded to float32 (what both FK solvers are given), FK from the near seeds (estimate, residual,
    iterations), TD (tensions, flag) and the unclamped tensions in float64 numpy from the oracle's Jacobian."""
    if n not in _SOLVER_CACHE:
        cfg, inp = solver_inputs(pkg, n)
        s = cfg.to_struct()
        B = SOLVER_B
        ref = dict(q=np.empty((B, n)), qd=np.empty((B, n)), L=np.empty((B, n)), jac=np.empty((B, n, 6)), est=np.empty((B, 7)), res=np.empty(B),
                   it=np.empty(B, dtype=np.int32), t=np.empty((B, n)), flag=np.empty(B, dtype=np.int32))
        for r in range(B):
            p64 = inp["pose"][r].astype(np.float64)
            ref["q"][r], ref["qd"][r], ref["L"][r], ref["jac"][r] = oracle.ik(s, p64, inp["twist"][r].astype(np.float64))
        ref["lengths32"] = ref["L"].astype(np.float32)
        for r in range(B):
            ref["est"][r], ref["res"][r], ref["it"][r] = oracle.fk(s, ref["lengths32"][r].astype(np.float64), inp["seed"][r].astype(np.float64))
            ref["t"][r], ref["flag"][r] = oracle.td_wrench(s, inp["pose"][r].astype(np.float64), inp["wrench"][r].astype(np.float64))
        # the residual the oracle's FK tests against fkTolerance before each iteration (column k: after k iterations)
        ref["res_seq"] = np.empty((B, cfg.fkMaxIterations + 1))
        for k in range(cfg.fkMaxIterations + 1):
            sk = pkg.Config(model=cfg.model, batch=1, stages=3, fkMaxIterations=max(k, 1), fkTolerance=0.0 if k else 1e9).to_struct()
            for r in range(B):
                ref["res_seq"][r, k] = oracle.fk(sk, ref["lengths32"][r].astype(np.float64), inp["seed"][r].astype(np.float64))[1]
        ref["unclamped"] = unclamped_tensions(ref["jac"], inp["wrench"].astype(np.float64), float(s.td_f_min), float(s.td_f_max))
        ref["f_min"], ref["f_max"], ref["fk_tolerance"] = float(s.td_f_min), float(s.td_f_max), float(s.fk_tolerance)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _SOLVER_CACHE[n] = (cfg, inp, ref)
    return _SOLVER_CACHE[n]


# ---- the oracle's FK in float32 numpy (an emulation of the ORACLE's arithmetic, not of any kernel) ------------------------------
def fk_float32(cfg_struct, lengths, seed):
    """orc_fk (oracle/cdpr_oracle.c: IK, J^T J + lambda I, 6 x 6 Cholesky, q <- exp(theta / 2) (x) q, the tolerance-controlled exit)
    restated with every operation in numpy float32, batched.  Returns (estimate[B, 7], residual[B], iterations[B]).  Used to
    tell what float32 arithmetic can and cannot meet; never compared with a kernel as a reference."""
    f = np.float32
    n = int(cfg_struct.n_cables)
    a = np.array([[cfg_struct.frame_anchor[i][k] for k in range(3)] for i in range(n)], dtype=f)
    b = np.array([[cfg_struct.platform_anchor[i][k] for k in range(3)] for i in range(n)], dtype=f)
    lam, tol, iters = f(cfg_struct.fk_lambda), f(cfg_struct.fk_tolerance), int(cfg_struct.fk_max_iterations)
    pose = np.array(seed, dtype=f)
    want = np.array(lengths, dtype=f)
    B = pose.shape[0]

    def ik(p):
        x, y, z, w = (p[:, 3 + k] for k in range(4))
        one, two = f(1), f(2)
        r = np.stack([one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w),
                      two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w),
                      two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)], axis=1).reshape(B, 3, 3)
        rb = (r[:, None, :, 0] * b[None, :, 0, None] + r[:, None, :, 1] * b[None, :, 1, None]) + r[:, None, :, 2] * b[None, :, 2, None]
        l = (p[:, None, :3] + rb) - a[None]
        length = np.sqrt((l[..., 0] * l[..., 0] + l[..., 1] * l[..., 1]) + l[..., 2] * l[..., 2])
        u = l / length[..., None]
        return length, np.concatenate([u, np.cross(rb, u).astype(f)], axis=2)

    done = np.zeros(B, dtype=bool)
    count = np.zeros(B, dtype=np.int32)
    for _ in range(iters):
        length, jac = ik(pose)
        r = want - length
        done |= np.abs(r).max(axis=1) < tol
        if done.all():
            break
        m = np.zeros((B, 6, 6), dtype=f)
        g = np.zeros((B, 6), dtype=f)
        for i in range(n):  # sums in cable order, as normal_eq
            m += jac[:, i, :, None] * jac[:, i, None, :]
            g += jac[:, i, :] * r[:, i, None]
        m[:, range(6), range(6)] += lam
        for j in range(6):  # chol6_solve
            d = m[:, j, j].copy()
            for k in range(j):
                d -= m[:, j, k] * m[:, j, k]
            d = np.sqrt(d)
            m[:, j, j] = d
            for i in range(j + 1, 6):
                s = m[:, i, j].copy()
                for k in range(j):
                    s -= m[:, i, k] * m[:, j, k]
                m[:, i, j] = s / d
        for i in range(6):
            s = g[:, i].copy()
            for k in range(i):
                s -= m[:, i, k] * g[:, k]
            g[:, i] = s / m[:, i, i]
        for i in range(5, -1, -1):
            s = g[:, i].copy()
            for k in range(i + 1, 6):
                s -= m[:, k, i] * g[:, k]
            g[:, i] = s / m[:, i, i]
        th = g[:, 3:]
        a2 = (th[:, 0] * th[:, 0] + th[:, 1] * th[:, 1]) + th[:, 2] * th[:, 2]
        an = np.sqrt(a2)
        with np.errstate(invalid="ignore", divide="ignore"):
            kk = np.where(an < f(1e-8), f(0.5) - a2 / f(48.0), np.sin(f(0.5) * an) / an).astype(f)
        c = np.cos(f(0.5) * an)
        d0, d1, d2 = kk * th[:, 0], kk * th[:, 1], kk * th[:, 2]
        x, y, z, w = (pose[:, 3 + k] for k in range(4))
        nw = c * w - d0 * x - d1 * y - d2 * z
        nx = c * x + w * d0 + d1 * z - d2 * y
        ny = c * y + w * d1 + d2 * x - d0 * z
        nz = c * z + w * d2 + d0 * y - d1 * x
        nn = np.sqrt(((nx * nx + ny * ny) + nz * nz) + nw * nw)
        new = pose.copy()
        new[:, :3] = pose[:, :3] + g[:, :3]
        new[:, 3:] = np.stack([nx / nn, ny / nn, nz / nn, nw / nn], axis=1)
        pose = np.where(done[:, None], pose, new)
        count += ~done
    length, _ = ik(pose)
    assert pose.dtype == f and length.dtype == f
    return pose, np.abs(want - length).max(axis=1), count
