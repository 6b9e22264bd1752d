"""Done rules (cdpr_evaluate_done, cdpr_reset_done_device): the predicate in numpy and the scenarios shared by
tests/test_done_rule_inputs.py (CPU: the conditions on the reference and on the oracle that the GPU tests rely on) and
tests/test_gpu_done.py (GPU), so that both see the same seeds, rules and batches.  A plain module: no fixtures, no pytest hooks.

The verdict is specified as a pure function of what the getters return (include/cdpr.h); `done_reference` is that function, in
float32 or float64 to match the handle.  numpy has no fma, the kernels use it: the metrics of tilt, speed and rate may differ from the
kernels' in the last bits, so every scenario keeps those metrics away from their thresholds and the tests assert that they do
(`metric_margins`).  The workspace, FK-residual, flag and timeout tests involve no arithmetic and are exact, on the bound included.
"""
import numpy as np
from scipy.spatial.transform import Rotation

import robot_histories as ri
from parity import perturbed_poses

B = ri.B
NONFINITE, WORKSPACE, TILT, SPEED, RATE, FK_RESIDUAL, INFEASIBLE, TRAVEL, TIMEOUT = (1 << k for k in range(9))
COUNTS = 16
BIT_NAMES = ("nonfinite", "workspace", "tilt", "speed", "rate", "fk_residual", "infeasible", "travel", "timeout")


def metrics(pose, twist, dtype):
    """R33, v . v and w . w of every robot in `dtype` (the operation order of the header's formulas)."""
    p, t = np.asarray(pose).astype(dtype), np.asarray(twist).astype(dtype)
    with np.errstate(all="ignore"):
        tilt = p[:, 3] * p[:, 3] + p[:, 4] * p[:, 4]
        qq = p[:, 6] * p[:, 6] + (p[:, 5] * p[:, 5] + tilt)
        r33 = dtype(1) - (dtype(2) * tilt) / qq
        vv = t[:, 2] * t[:, 2] + (t[:, 1] * t[:, 1] + t[:, 0] * t[:, 0])
        ww = t[:, 5] * t[:, 5] + (t[:, 4] * t[:, 4] + t[:, 3] * t[:, 3])
    return r33, vv, ww


def done_reference(rule, pose, twist, fk_residual, infeasible, limit_mask, start, step_count, f64):
    """(mask uint8[B], reason uint32[B], counts uint32[16]) of `rule` (a DoneRule) on the getters' outputs: pose / twist from
    raw_state[_f64], fk_residual from fk_state, infeasible from td_state, limit_mask from limit_state (None where the handle has no
    such stage: zeros), start from episode_start, step_count.  The rule's thresholds are float32 values, promoted when f64."""
    T = np.float64 if f64 else np.float32
    p, t = np.asarray(pose).astype(T), np.asarray(twist).astype(T)
    n = p.shape[0]
    f32 = lambda v: np.asarray(v, dtype=np.float32).astype(T)  # noqa: E731
    lo, hi = f32(rule.pos_lo), f32(rule.pos_hi)
    res = np.zeros(n, T) if fk_residual is None else np.asarray(fk_residual).astype(T)
    inf = np.zeros(n, bool) if infeasible is None else np.asarray(infeasible) != 0
    lim = np.zeros(n, bool) if limit_mask is None else np.asarray(limit_mask) != 0
    r33, vv, ww = metrics(p, t, T)
    age = (np.uint32(int(step_count) & 0xFFFFFFFF) - np.asarray(start, dtype=np.uint32)).astype(np.uint32)
    with np.errstate(all="ignore"):
        cond = [
            ~(np.isfinite(p).all(axis=1) & np.isfinite(t).all(axis=1)),
            ((p[:, :3] < lo) | (p[:, :3] > hi)).any(axis=1),
            r33 < f32(rule.min_up),
            vv > f32(rule.max_speed) * f32(rule.max_speed),
            ww > f32(rule.max_rate) * f32(rule.max_rate),
            res > f32(rule.max_fk_residual),
            inf,
            lim,
            age >= np.uint32(rule.max_steps),
        ]
    reason = np.zeros(n, np.uint32)
    for k, c in enumerate(cond):
        if (int(rule.enable) >> k) & 1:
            reason |= np.where(c, np.uint32(1 << k), np.uint32(0)).astype(np.uint32)
    counts = np.zeros(COUNTS, np.uint32)
    counts[0] = int((reason != 0).sum())
    for k in range(COUNTS - 1):
        counts[1 + k] = int(((reason >> np.uint32(k)) & np.uint32(1)).sum())
    return (reason != 0).astype(np.uint8), reason, counts


def metric_margins(rule, pose, twist):
    """Relative distance of the tilt, speed and rate metric of every robot from its threshold, in float64: |metric - threshold| /
    |threshold| (NaN / inf metrics: inf - nothing rounds there).  The static tests assert that none is within 1e-5."""
    r33, vv, ww = metrics(pose, twist, np.float64)
    out = {}
    for name, m, thr in (("tilt", r33, float(np.float32(rule.min_up))), ("speed", vv, float(np.float32(rule.max_speed)) ** 2), ("rate", ww, float(np.float32(rule.max_rate)) ** 2)):
        with np.errstate(all="ignore"):
            d = np.abs(m - thr) / abs(thr)
        out[name] = np.where(np.isfinite(d), d, np.inf)
    return out


# ---- the static scenario (item 1 of tests/test_gpu_done.py) ----------------------------------------------------------------------
HALF = 0.05      # half width of the workspace box around the home position
MIN_UP = 0.955   # ~ cos(0.3 rad)
MAX_SPEED, MAX_RATE = 0.5, 1.0
ON_LO, ON_HI, BELOW_LO, ABOVE_HI = (3, 4, 5), (6, 7, 8), (9, 10, 11), (12, 13, 14)  # robot k sits on / past the bound of axis k % 3
TILTED, UPRIGHT_SCALED = (20, 21, 22, 66, 128), (23, 24, 25)
FAST, SPINNING, FAST_AND_OUT = (30, 31, 32, 67), (40, 41, 42, 127), (50, 51, 52)
NAN_POSITION, INF_TWIST, NEG_INF_POSITION, NAN_QUATERNION = 63, 64, 65, 129
NONFINITE_ROBOTS = (NAN_POSITION, INF_TWIST, NEG_INF_POSITION, NAN_QUATERNION)


def static_scenario(pkg, model, f64):
    """(rule, pose, twist): B robots placed so that every one of NONFINITE, WORKSPACE, TILT, SPEED, RATE fires for some and stays
    clear for others; pose and twist in the handle's precision (float32 / float64).  Robots ON_LO / ON_HI sit exactly on the
    box (inside), BELOW_LO / ABOVE_HI one value of the handle's precision past it; TILTED are rotated by 0.5 rad about x (or y),
    some with a quaternion that is not normalised; UPRIGHT_SCALED carry a small tilt and a quaternion of length 1.7."""
    T = np.float64 if f64 else np.float32
    rng = np.random.default_rng(101)
    home = np.asarray(model.home_pose(), dtype=np.float64)
    lo32, hi32 = (home[:3] - HALF).astype(np.float32), (home[:3] + HALF).astype(np.float32)
    rule = pkg.DoneRule(enable=NONFINITE | WORKSPACE | TILT | SPEED | RATE, pos_lo=tuple(float(v) for v in lo32), pos_hi=tuple(float(v) for v in hi32),
                        min_up=MIN_UP, max_speed=MAX_SPEED, max_rate=MAX_RATE)
    pose = perturbed_poses(model, B, rng, 0.8 * HALF, 0.1).astype(T)
    twist = rng.uniform(-0.1, 0.1, (B, 6)).astype(T)
    lo, hi = lo32.astype(T), hi32.astype(T)
    for group, bound, toward in ((ON_LO, lo, None), (ON_HI, hi, None), (BELOW_LO, lo, -np.inf), (ABOVE_HI, hi, np.inf)):
        for k in group:
            c = k % 3
            pose[k, c] = bound[c] if toward is None else np.nextafter(bound[c], T(toward))
    for j, k in enumerate(TILTED):
        axis = [0.5, 0.0, 0.0] if j % 2 == 0 else [0.0, -0.5, 0.0]
        pose[k, 3:] = (Rotation.from_rotvec(axis).as_quat() * (1.0 if j < 3 else 0.6)).astype(T)
    for k in UPRIGHT_SCALED:
        pose[k, 3:] = (pose[k, 3:].astype(np.float64) * 1.7).astype(T)
    for k in FAST + FAST_AND_OUT:
        twist[k, :3] = (np.array([0.5, -0.4, 0.3]) * (1.0 + 0.1 * (k % 4))).astype(T)  # |v| >= 0.707
    for k in FAST_AND_OUT:
        pose[k, k % 3] = T(home[k % 3] + 1.5 * HALF)
    for k in SPINNING:
        twist[k, 3:] = (np.array([-1.0, 1.2, 0.9]) * (1.0 + 0.1 * (k % 4))).astype(T)  # |w| >= 1.8
    pose[NAN_POSITION, 1] = np.nan
    twist[INF_TWIST, 0] = np.inf
    pose[NEG_INF_POSITION, 2] = -np.inf
    pose[NAN_QUATERNION, 6] = np.nan
    return rule, pose, twist


# ---- the closed loop (item 7) ------------------------------------------------------------------------------------------------------
LOOP_STEPS, LOOP_EVERY = 40, 5
LOOP_HALF = 0.015        # workspace box: home +- 15 mm
LOOP_MIN_UP = 0.99       # respawn tilts: rotvec components within +-0.03 rad (R33 >= 0.9991) or one of 0.2 rad (R33 = 0.980)
LOOP_MAX_SPEED = 0.5     # far above anything the commands reach: the bit is enabled and must stay clear
LOOP_MAX_STEPS = 15      # a robot that has not been reset for 15 steps times out
LOOP_ENABLE = NONFINITE | WORKSPACE | TILT | SPEED | TIMEOUT
LOOP_SEED = 2027


def loop_rule(pkg, model):
    home = np.asarray(model.home_pose(), dtype=np.float64)
    return pkg.DoneRule(enable=LOOP_ENABLE, pos_lo=tuple(float(v) for v in (home[:3] - LOOP_HALF).astype(np.float32)),
                        pos_hi=tuple(float(v) for v in (home[:3] + LOOP_HALF).astype(np.float32)), min_up=LOOP_MIN_UP, max_speed=LOOP_MAX_SPEED, max_steps=LOOP_MAX_STEPS)


def loop_poses(model, rng):
    """Start / respawn poses (float32): well inside the box and upright, except one robot in eight pushed 19 mm out along one axis
    and one in eight tilted by 0.2 rad about x or y."""
    pose = perturbed_poses(model, B, rng, 0.008, 0.03)
    home = np.asarray(model.home_pose(), dtype=np.float64)
    pick = rng.integers(0, 8, B)
    for k in np.nonzero(pick == 0)[0]:
        c = int(rng.integers(0, 3))
        pose[k, c] = home[c] + (0.019 if rng.random() < 0.5 else -0.019)
    for k in np.nonzero(pick == 1)[0]:
        axis = np.zeros(3)
        axis[int(rng.integers(0, 2))] = 0.2 if rng.random() < 0.5 else -0.2
        pose[k, 3:] = Rotation.from_rotvec(axis).as_quat()
    return pose.astype(np.float32)


def loop_inputs(model):
    """Everything the closed loop draws, in the order it is used: the history commands (robots in Position / Velocity / Force mode by
    index mod 3, as the reset tests have them), the start poses, one batch of respawn poses per evaluation point."""
    rng = np.random.default_rng(LOOP_SEED)
    h = ri.history_inputs(model, LOOP_SEED + 1)
    h["pose"] = loop_poses(model, rng)
    return h, [loop_poses(model, rng) for _ in range(LOOP_STEPS // LOOP_EVERY)]


def loop_margins(rule, pose, twist, tol):
    """The distance of every oracle robot's metric from its threshold in units of the parity tolerance of that quantity (`tol`: TOL
    or TOL64 of tests/parity.py): position components against the faces of the box at tol["pose"];
    R33 at 4 tol["pose"] (|dR33/dq| <= 4 |q| on quaternions of length ~1, and the quaternion is compared at the pose tolerance); |v|
    against max_speed at sqrt(3) tol["twist"].  An engine within tolerance of the oracle takes the oracle's decisions where every
    entry is above 1; the tests ask for 100."""
    p, t = np.asarray(pose, dtype=np.float64), np.asarray(twist, dtype=np.float64)
    lo, hi = np.asarray(rule.pos_lo, dtype=np.float32).astype(np.float64), np.asarray(rule.pos_hi, dtype=np.float32).astype(np.float64)
    r33, vv, _ = metrics(p, t, np.float64)
    return {
        "workspace": float(np.minimum(np.abs(p[:, :3] - lo), np.abs(p[:, :3] - hi)).min() / tol["pose"]),
        "tilt": float(np.abs(r33 - float(np.float32(rule.min_up))).min() / (4.0 * tol["pose"])),
        "speed": float(np.abs(np.sqrt(vv) - float(np.float32(rule.max_speed))).min() / (np.sqrt(3.0) * tol["twist"])),
    }


def run_loop(sims, ora, rule, h, respawn, reset_engine=None, check=None):
    """The closed loop on the oracle `ora` and, in lock step, on the engines `sims`: the history's three masked commands, then
    LOOP_STEPS steps; after every LOOP_EVERY steps the oracle's verdict (done_reference on its own getters, start clock kept here)
    drives ri.oracle_reset with that evaluation point's respawn poses, and reset_engine(j, poses) does what it does on the engines.
    check(j, mask, reason, counts, margins-input) is called at every evaluation point BEFORE the resets.  Returns the oracle-side
    (mask, reason, counts) per evaluation point."""
    start = np.zeros(B, np.uint32)
    for s in list(sims) + [ora]:
        assert s.set_position_command(h["p"], mask=(h["group"] == 0).astype(np.uint8)) == 0
        assert s.set_velocity_command(h["v"], mask=(h["group"] == 1).astype(np.uint8)) == 0
        assert s.set_force_command(h["f"], mask=(h["group"] == 2).astype(np.uint8)) == 0
    verdicts = []
    for j in range(LOOP_STEPS // LOOP_EVERY):
        for s in list(sims) + [ora]:
            s.update(LOOP_EVERY)
        p, t = ora.raw_state()
        mask, reason, counts = done_reference(rule, p, t, None, None, None, start, ora.step_count, True)
        verdicts.append((mask, reason, counts))
        if check is not None:
            check(j, mask, reason, counts, p, t)
        if reset_engine is not None:
            reset_engine(j, respawn[j])
        ri.oracle_reset(ora, mask, respawn[j])
        start[mask.astype(bool)] = np.uint32(ora.step_count)
    return verdicts
