"""What the parity tests share: the tolerances, the read-out of a simulator, the comparison with the oracle, the making of engines and
oracles at given start poses, the inputs several modules draw, the rollout cost bound and the list of routing overrides.  No module
imports a test_*.py module; what two of them need lives here or in a helper module beside this one (tests/test_support.py holds the
rule and shows that the comparison below can fail).

TOL.  Everything on the GPU is fp32 unless cdpr_config_t.precision = 64; tolerances are absolute, stated per quantity:
  pose 1e-5 (m / quaternion units), twist 2e-4 (m/s, rad/s), joint position 1e-5 m, joint velocity 2e-4 m/s,
  effort 2e-2 N (the effort range is +-100 N; the position Pid's D gain of 80 N s/m amplifies fp32 rounding of
  the 1 ms window: measured worst case on MI355X 2.2e-3 N).
Measured on MI355X at the sizes of tests/test_gpu_parity.py: pose <= 7e-7, twist <= 1.5e-5, effort <= 2.3e-3.

TOL64.  precision = 64 (cdpr_step_kernel_f64.hpp): both sides compute in double; they differ in the order of the sums and in the
derivative's formulation (closed-form end-point weights here, a least-squares fit in centred time there), so the agreement is that of
two double implementations.  Measured on MI355X over tests/test_gpu_fp64.py: pose 8.3e-16, twist 5.1e-14, joint position 6.7e-16,
joint velocity 3.9e-14, effort 1.2e-11 N (the position Pid's D gain times 1/dt = 8e4 N s/m amplifies the last bits of the 1 ms
window); config 1 over 3 000 steps: pose 1.7e-16, effort 7.3e-14.  Tolerances: two orders above that.

pytest rewrites asserts only in test modules, so every assert here carries its message.
"""
from dataclasses import replace

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

NAMES = ("pose", "twist", "q", "qd", "eff")
TOL = {"pose": 1e-5, "twist": 2e-4, "q": 1e-5, "qd": 2e-4, "eff": 2e-2}
TOL64 = {"pose": 1e-13, "twist": 5e-12, "q": 1e-13, "qd": 5e-12, "eff": 1e-9}
WORST64 = {}  # worst error per quantity over every compare64 of the session (tests/test_gpu_fp64.py prints it)

# 128-robot slices of a 65 536-robot run that the oracle replays: workgroups 0-1, 9-10 and 1022-1023 of the split kernel;
# under the role-swap mask 0x9 (StepArgs::split_swap) each pair holds one swapped and one un-swapped workgroup
# (popcount(block & 9): 0, 1 | 2, 1 | 1, 2), and the last pair sits at the far end of the grid
FULL_SIZE_SLICES = (slice(0, 128), slice(576, 704), slice(65408, 65536))

# every CDPR_* name cdpr_select.hpp reads through env("...") (tests/test_support.py compares the list with the file), and
# CDPR_STRIDE_PAD, which cdpr_create reads (the forced row-stride pad of tests/padded_stride.py: set around a create only), and
# CDPR_STEP_ORIGIN, which cdpr_create reads as well (the clock origin of tests/late_clock.py: set around a create only)
ROUTING_OVERRIDES = ("CDPR_MAPPING", "CDPR_LOWREG", "CDPR_CHUNK", "CDPR_PERSIST", "CDPR_ONESTEP", "CDPR_SPLIT", "CDPR_PAIR_STREAM", "CDPR_GEN_SPLIT",
                     "CDPR_GEN_LEAN", "CDPR_GEN_HOT", "CDPR_STRIDE_PAD", "CDPR_STEP_ORIGIN")


# ---- hermeticity ---------------------------------------------------------------------------------------------------------------
def clear_overrides(monkeypatch, more=()):
    for k in ROUTING_OVERRIDES + tuple(more):
        monkeypatch.delenv(k, raising=False)


def clean_env_fixture(*more):
    """The fixture that clears ROUTING_OVERRIDES and `more`: autouse in every module that holds it under a name."""
    @pytest.fixture(autouse=True)
    def clean_env(monkeypatch):
        clear_overrides(monkeypatch, more)

    return clean_env


# ---- read-out ------------------------------------------------------------------------------------------------------------------
def observed(sim, f64=False):
    """(pose, twist, q, qd, effort) of the last published step, in NAMES order: observables_f64 of an engine where f64, else - and
    always for an oracle - platform_state + joint_states."""
    if f64 and hasattr(sim, "observables_f64"):
        q, qd, e, p, t = sim.observables_f64()
        return p, t, q, qd, e
    return tuple(sim.platform_state()) + tuple(sim.joint_states())


def state_of(eng, f64, joint_states=False):
    """What two engines are compared on bit for bit: raw_state and observables (the doubles of a precision = 64 handle);
    joint_states: the separate float getter of an fp32 handle as well."""
    if f64:
        return eng.raw_state_f64() + eng.observables_f64()
    return eng.raw_state() + (eng.joint_states() if joint_states else ()) + eng.observables()


def every_getter(eng, cfg, pkg):
    """state_of, the episode clock and the FK, TD, limit and pid-debug read-outs the handle's stages have"""
    out = list(state_of(eng, cfg.precision == 64, joint_states=True)) + [eng.episode_start(), eng.limit_state()]
    if cfg.precision == 64:
        out += list(eng.raw_state()) + list(eng.joint_states())  # (the float getters of the double rows)
    if cfg.stages & pkg._abi.STAGE_FK:
        out += list(eng.fk_state())
    if cfg.stages & pkg._abi.STAGE_TD:
        out += list(eng.td_state())
    if cfg.stages & pkg._abi.STAGE_PID_DEBUG:
        out.append(eng.pid_debug())
    return out


def equal_rows(xs, ys, rows_x, rows_y):
    return all(np.array_equal(x[rows_x], y[rows_y]) for x, y in zip(xs, ys))


# ---- the comparison ------------------------------------------------------------------------------------------------------------
def worst_errors(got, want, where, f64=False, rows=None):
    """The core: `got` and `want` are five arrays in NAMES order, `want` of the robots `rows` (a slice) of `got` where given.  Every
    quantity read is finite, and float64 where f64.  Returns {name: (worst absolute error, robot, column)}."""
    out = {}
    for name, g, o in zip(NAMES, got, want):
        g = np.asarray(g) if rows is None else np.asarray(g)[rows]
        assert not f64 or g.dtype == np.float64, f"{where}: {name} is {g.dtype}, not float64"
        assert np.isfinite(g).all(), f"{where}: {name} is not finite"
        d = np.abs(g - o)
        r, c = np.unravel_index(d.argmax(), d.shape)
        out[name] = (float(d.max()), int(r) + (0 if rows is None else rows.start or 0), int(c))
    return out


def assert_within(worst, tol, where):
    for name in NAMES:
        err = worst[name][0]
        assert err <= tol[name], f"{where}: {name} differs from the oracle by {err:.3e} (tolerance {tol[name]:.1e})"


def compare(eng, ora, tol=TOL, where=""):
    """The float getters of an engine against the oracle."""
    assert_within(worst_errors(observed(eng), observed(ora), where), tol, where)


def compare64(eng, ora, where, tol=TOL64):
    """observables_f64 of a precision = 64 engine against the oracle; returns {name: worst error}."""
    worst = worst_errors(observed(eng, True), observed(ora), where, f64=True)
    assert_within(worst, tol, where)
    for name, (err, _, _) in worst.items():
        WORST64[name] = max(WORST64.get(name, 0.0), err)
    return {name: err for name, (err, _, _) in worst.items()}


def against_the_oracle(eng, ora, f64, where, printed=None):
    """compare64 at TOL64 where f64, else compare at TOL; printed: the call's name, for a line of the worst errors (-s).
    Returns {name: (worst error, robot, column)}."""
    worst = worst_errors(observed(eng, f64), observed(ora), where, f64=f64)
    if printed:
        print(f"{printed}, {where}: " + "  ".join(f"{k} {v[0]:.2e}" for k, v in worst.items()))
    assert_within(worst, TOL64 if f64 else TOL, where)
    return worst


def check_slice(pkg, oracle, cfg_kwargs, sl, pose, script, got, tol=TOL):
    """Replay `script` ([(nsteps, command or None)]; a command is an array = jointVelocities, or ("pos", array) =
    jointPositions) on the oracle for robots `sl` and compare with `got` = (pose, twist, q, qd, effort) of the full GPU run.
    Robots are independent, so a slice of the batch is its own problem."""
    n = sl.stop - sl.start
    ora = oracle.OracleSim(pkg.Config(batch=n, **cfg_kwargs).to_struct(), oracle.DERIV_EXACT)
    ora.set_platform_state(pose7=pose[sl].astype(np.float64))
    for nsteps, cmd in script:
        if isinstance(cmd, tuple):
            ora.set_position_command(cmd[1][sl])
        elif cmd is not None:
            ora.set_velocity_command(cmd[sl])
        ora.update(nsteps)
    where = f"robots {sl.start} .. {sl.stop - 1}"
    assert_within(worst_errors(got, observed(ora), where, rows=sl), tol, where)


def run_script(eng, ora, script, tol=TOL, label=""):
    for kind, val in script:
        for sim in (eng, ora):
            if kind == "vel":
                sim.set_velocity_command(val)
            elif kind == "pos":
                sim.set_position_command(val)
            else:
                sim.update(val)
        if kind == "run":
            compare(eng, ora, tol=tol, where=f"{label} after run {val}")


def rollout_cost_tol(reference_cost, floor):
    """The bound on |cost - reference cost| of an MPC rollout: floor + 2e-4 max |reference cost| (floor 1e-6; 1e-9 on the general path)."""
    return floor + 2e-4 * float(np.abs(reference_cost).max())


# ---- simulators at given start poses -------------------------------------------------------------------------------------------
def sims_at(pkg, oracle, cfg, pose=None, count=1, twist=None, with_oracle=True, through_f32=True, f64=None):
    """`count` engines and, unless with_oracle is false, an oracle, at the same start state: ([engines], oracle or None).
    An engine takes it through set_platform_state_f64 where f64 (default: cfg.precision == 64), else as float32.  through_f32: the
    doubles of the oracle and of an f64 engine are the float32 values (what an fp32 engine holds); false: the doubles as given."""
    f64 = cfg.precision == 64 if f64 is None else f64
    engs = [pkg.Engine(cfg, 0) for _ in range(count)]
    ora = oracle.OracleSim(cfg.to_struct(), oracle.DERIV_EXACT) if with_oracle else None
    if pose is not None or twist is not None:
        p32, t32 = (None if x is None else np.asarray(x, dtype=np.float32) for x in (pose, twist))
        p64, t64 = (None if x is None else np.asarray(y if through_f32 else x, dtype=np.float64) for x, y in ((pose, p32), (twist, t32)))
        for e in engs:
            e.set_platform_state_f64(pose7=p64, twist6=t64) if f64 else e.set_platform_state(pose7=p32, twist6=t32)
        if ora is not None:
            ora.set_platform_state(pose7=p64, twist6=t64)
    return engs, ora


def pair(pkg, oracle, cfg, pose=None, twist=None):
    """One engine on the float setters and its oracle at the float32 values."""
    (eng,), ora = sims_at(pkg, oracle, cfg, pose, twist=twist, f64=False)
    return eng, ora


def pair64(pkg, oracle, cfg, pose=None):
    """One precision = 64 engine and its oracle at the doubles as given."""
    (eng,), ora = sims_at(pkg, oracle, cfg, pose, through_f32=False, f64=True)
    return eng, ora


def engines(pkg, cfg, pose, count):
    return sims_at(pkg, None, cfg, pose, count, with_oracle=False)[0]


def oracle_at(oracle, cfg, pose):
    return sims_at(None, oracle, cfg, pose, 0)[1]


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def perturbed_poses(model, B, rng, dp=0.05, dr=0.1):
    pose = np.tile(model.home_pose(), (B, 1))
    pose[:, :3] += rng.uniform(-dp, dp, (B, 3))
    pose[:, 3:] = Rotation.from_rotvec(rng.uniform(-dr, dr, (B, 3))).as_quat()
    return pose


def sliced_twelve(pkg, n):
    """The first n cables of twelve_cable_model."""
    m = pkg.twelve_cable_model()
    return m if n == 12 else replace(m, frame_anchors=m.frame_anchors[:n], platform_anchors=m.platform_anchors[:n])


def static_forces(cfg, B, rng, spread=0.5):
    """Forces around what holds the platform: 3.9657 N per cable on the shipped cube, mid tension on 8 cables."""
    base = 3.965671444 if cfg.n_cables == 4 else 7.0
    return (base + rng.uniform(-spread, spread, (B, cfg.n_cables))).astype(np.float32)


def hold_commands(rng, B, n, eps, share=0.35):
    """Velocity Joys with a good share of the cables at or below epsilon (hold branch) and the rest clearly above."""
    cmd = rng.uniform(-0.04, 0.04, (B, n)).astype(np.float32)
    cmd[np.abs(cmd) <= 2 * eps] = np.float32(3 * eps)
    low = rng.random((B, n)) < share
    cmd[low] = (rng.uniform(-1.0, 1.0, int(low.sum())) * eps).astype(np.float32)
    return cmd
