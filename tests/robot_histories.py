"""The inputs the tests of the calls over chosen robots share (reset_robots, copy_robots, the done rules, the environment view, resample,
the launch forms): batch, models, a 37-step history with robots in three modes, what follows it, and the oracle-side reset recipe.

The oracle has no masked reset and needs none.  On OracleSim a reset of mask m is `oracle_reset` below: raw_state read back, the rows of
m overwritten with the new pose and twist (float32 values as doubles), set_platform_state with the result, then
set_velocity_command(0, mask=m) and set_position_command(0, mask=m).  Both latch at the next update, velocity first, then position
(PLG.cpp:206-219): whatever mode a robot was in, it ends in Position mode with target 0 and the Pid of each mode entered reset
(JFC.cpp:101-103, 113-115); a velocity Pid that was not reset - the robot was in Velocity mode already - is reset before it can run again.
The one thing the recipe cannot set is mLastPosition; Position mode overwrites it every step, so in comparisons with the oracle a velocity
Joy below velocityEpsilon reaches a reset robot only after at least one update.  tests/test_reset_robots_inputs.py establishes on the
oracle alone that the recipe leaves nothing of a robot's history behind.
"""
import numpy as np

from parity import perturbed_poses, sliced_twelve

B = 130      # two full wavefronts and a ragged one (stride 192)
EPS = 0.002  # velocityEpsilon of the handles with the hold branch
HISTORY = 37  # steps before the reset: more than any nbuf of the shipped windows (windows full, call counts saturated, hot rows entered)

CONFIGS = {  # (cables, Config arguments)
    "n8_fk_td": (8, dict(stages=3)),
    "n8_fk_td_hold": (8, dict(stages=3, velocityEpsilon=EPS)),
    "n4": (4, dict(stages=0)),
}


def model_of(pkg, n):
    if n == 4:
        return pkg.cube_model()
    if n == 8:
        return pkg.eight_cable_model()
    return sliced_twelve(pkg, n)


def reset_mask(batch=B):
    """every fourth robot plus the corners of the wavefronts"""
    m = np.zeros(batch, dtype=np.uint8)
    m[::4] = 1
    m[[0, 63, 64, batch - 1]] = 1
    return m


def oracle_reset(ora, mask, pose7=None, twist6=None, home=None):
    """The recipe: what cdpr_reset_robots(mask, pose7, twist6) is on the oracle.  pose7 None: `home` (the model's home pose)."""
    m = np.asarray(mask).astype(bool)
    p, t = ora.raw_state()
    p[m] = np.asarray(home, dtype=np.float64) if pose7 is None else np.asarray(pose7, dtype=np.float32).astype(np.float64)[m]
    t[m] = 0.0 if twist6 is None else np.asarray(twist6, dtype=np.float32).astype(np.float64)[m]
    ora.set_platform_state(pose7=p, twist6=t)
    zero = np.zeros(ora.n, dtype=np.float32)
    for name in ("set_velocity_command", "set_position_command"):
        rc = getattr(ora, name)(zero, mask=m.astype(np.uint8))
        assert rc == 0, f"oracle_reset: {name} returned {rc}"


def forces(n, rng, batch=B):
    """around what holds the platform (parity.static_forces, tests/test_gpu_cable_counts.py)"""
    if n == 4:
        return (3.965671444 + rng.uniform(-0.5, 0.5, (batch, n))).astype(np.float32)
    if n == 8:
        return (7.0 + rng.uniform(-0.5, 0.5, (batch, n))).astype(np.float32)
    return rng.uniform(2.0, 6.0, (batch, n)).astype(np.float32)


def history_inputs(model, seed, shift=0, batch=B):
    """Start poses and the three commands of a history; robots by (index + shift) mod 3: Position, Velocity, Force mode."""
    rng = np.random.default_rng(seed)
    n = model.n_cables
    return dict(pose=perturbed_poses(model, batch, rng, 0.02, 0.05).astype(np.float32), group=(np.arange(batch) + shift) % 3,
                v=rng.uniform(-0.03, 0.03, (batch, n)).astype(np.float32), p=rng.uniform(-0.004, 0.004, (batch, n)).astype(np.float32), f=forces(n, rng, batch))


def after_inputs(model, seed, batch=B):
    """What follows the history: the reset poses, a velocity Joy whose even cables sit below EPS (they hold position where the hold branch
    is live) for the even robots, a position Joy for two robots of three."""
    rng = np.random.default_rng(seed)
    n = model.n_cables
    v = rng.uniform(-0.03, 0.03, (batch, n)).astype(np.float32)
    v[np.abs(v) <= 2 * EPS] = np.float32(3 * EPS)
    v[:, ::2] = np.float32(0.5 * EPS)
    return dict(pose=perturbed_poses(model, batch, rng, 0.02, 0.05).astype(np.float32), v=v, v_mask=(np.arange(batch) % 2 == 0).astype(np.uint8),
                p=rng.uniform(-0.004, 0.004, (batch, n)).astype(np.float32), p_mask=(np.arange(batch) % 3 != 1).astype(np.uint8))


def _sent(rc, what):
    assert rc == 0, f"{what} returned {rc}"


def play_history(sims, h, steps=HISTORY):
    for s in sims:
        _sent(s.set_position_command(h["p"], mask=(h["group"] == 0).astype(np.uint8)), "play_history: set_position_command")
        _sent(s.set_velocity_command(h["v"], mask=(h["group"] == 1).astype(np.uint8)), "play_history: set_velocity_command")
        _sent(s.set_force_command(h["f"], mask=(h["group"] == 2).astype(np.uint8)), "play_history: set_force_command")
        s.update(steps)


def play_after(sims, a, check):
    """The script behind a reset: 1 step, 6 more, the masked velocity Joy + 30 steps, the masked position Joy + 25 steps; check(label)
    after each."""
    for s in sims:
        s.update(1)
    check("1 step after the reset")
    for s in sims:
        s.update(6)
    check("7 steps after the reset")
    for s in sims:
        _sent(s.set_velocity_command(a["v"], mask=a["v_mask"]), "play_after: set_velocity_command")
        s.update(30)
    check("30 steps after the masked velocity Joy")
    for s in sims:
        _sent(s.set_position_command(a["p"], mask=a["p_mask"]), "play_after: set_position_command")
        s.update(25)
    check("25 steps after the masked position Joy")
