"""Inputs that drive the Pid's clamps and the hold threshold: shared by tests/test_pid_limit_inputs.py (CPU: the oracle-side
conditions the GPU tests rely on) and tests/test_gpu_pid_limits.py (GPU), so that both see the same seeds, limits and commands.
A plain module: no fixtures, no pytest hooks.

Pid::update (Pid.cpp:122-191) clamps the integral term (143-152: iTerm to +-iLimit, mIerr recomputed from it) and the command
(175-186: cmd to +-cmdLimit, and where the clamp bit, mIerr restored and ONE increment iGain dt error added to the clamped command,
which therefore ends up beyond the clamp); SetForce then clamps at the joint's effort limit.  Under the shipped limits (100, 100,
100) and the commands the other modules send none of them is reached.  A variant lowers limits until one is:

  command             shipped gains, iLimit 0.03 (velocity Pid) / 0.3 (position Pid), cmdLimit 12 on both, effort limit 20; with the
                      tension distribution on, its bounds 0.5 / 18
  command_low_effort  as command with effort limit 9: SetForce clamps below the Pid's clamp (tension bounds 0.5 / 8: their middle
                      has to lie inside the effort limit, or every effort sits on SetForce's clamp and the Pid is invisible)
  integral            iGain 400 / 1400, iLimit 0.5 / 1.0, cmdLimit and effort limit at the shipped 100 (tension bounds as shipped)

The scripts (SCRIPTS) alternate runs and Joys; every command array is float32 and goes to every simulator unchanged.  Start poses:
parity.perturbed_poses(model, 130, rng, 0.02, 0.05) rounded to float32.

The hold ladder: JFC.cpp:72 runs the velocity Pid where abs(mVelocityTarget) > mVelocityEpsilon, in double, on a Joy axis that
is a float32.  The ladder puts targets on, one float32 below and one float32 above float32(eps), and at eps = 0 on +-0, the
smallest subnormal and the smallest normal float32.
"""
import copy
from dataclasses import replace

import numpy as np

import workspace_poses as wp
from parity import perturbed_poses

B = 130
SEED_OFFSET = 4000  # added to the cell's own seed (workspace_poses.CELLS)
VARIANTS = {
    #                     iLimit (vel, pos)   iGain (vel, pos) or None   cmdLimit   effort limit   tension bounds or None
    "command":            dict(i_limit=(0.03, 0.3), i_gain=None, cmd_limit=12.0, effort_limit=20.0, td=(0.5, 18.0)),
    "command_low_effort": dict(i_limit=(0.03, 0.3), i_gain=None, cmd_limit=12.0, effort_limit=9.0, td=(0.5, 8.0)),
    "integral":           dict(i_limit=(0.5, 1.0), i_gain=(400.0, 1400.0), cmd_limit=100.0, effort_limit=100.0, td=None),
}
LOW_EFFORT_CELLS = ("step", "split", "pair_stream", "cable", "gen_split", "f64_split", "per_robot")
CASES = [(cell, v) for v in ("command", "integral") for cell in wp.CELLS] + [(cell, "command_low_effort") for cell in LOW_EFFORT_CELLS]

_COMMAND_SCRIPT = (("run", 40), ("vel", "small_v", 1), ("run", 40), ("vel", "big_v", 1), ("run", 20), ("vel", "small_v", -1), ("run", 50),
                   ("pos", "big_p", 1), ("run", 30), ("pos", "small_p", 1), ("run", 50), ("vel", "big_v", -1), ("run", 12),
                   ("pos", "small_p", -1), ("run", 50))
SCRIPTS = {
    "command": _COMMAND_SCRIPT,
    "command_low_effort": _COMMAND_SCRIPT,
    "integral": (("run", 70), ("vel", "small_v", 1), ("run", 70), ("pos", "small_p", 1), ("run", 70), ("vel", "small_v", -1), ("run", 70),
                 ("pos", "small_p", -1), ("run", 70)),
}
SETTER = {"vel": "set_velocity_command", "pos": "set_position_command"}


def apply(cfg, variant):
    """A copy of `cfg` under `variant`: the limits, the integral gains and the tension bounds change, nothing else."""
    v = VARIANTS[variant]
    out = copy.deepcopy(cfg)
    for pid, k in ((out.velocityController, 0), (out.positionController, 1)):
        pid.iLimit, pid.cmdLimit = v["i_limit"][k], v["cmd_limit"]
        if v["i_gain"]:
            pid.iGain = v["i_gain"][k]
    out.model = replace(out.model, effort_limit=v["effort_limit"])
    if out.stages & 2 and v["td"]:
        out.tdFMin, out.tdFMax = v["td"]
    return out


def without(cfg, limit):
    """A copy of `cfg` with one limit out of reach: "i_limit", "cmd_limit" (1e6 on both Pids) or "effort_limit" (-1: no clamp)."""
    out = copy.deepcopy(cfg)
    if limit == "effort_limit":
        out.model = replace(out.model, effort_limit=-1.0)
    else:
        for pid in (out.velocityController, out.positionController):
            setattr(pid, {"i_limit": "iLimit", "cmd_limit": "cmdLimit"}[limit], 1e6)
    return out


def case_config(pkg, cell, variant):
    """(the cell's own Config, the Config under the variant, environment switches, seed)."""
    cfg, env, seed = wp.cell_config(pkg, cell, batch=B)
    return cfg, apply(cfg, variant), env, seed + SEED_OFFSET


def start_poses(model, rng, batch=B):
    return perturbed_poses(model, batch, rng, 0.02, 0.05).astype(np.float32)


def random_sign(rng, shape):
    return rng.choice([-1.0, 1.0], shape)


HOLD_FREE = 0.005  # above every velocityEpsilon of the cells (0.004 at most)


def commands(rng, batch, n, variant):
    """The command arrays of the scripts, float32: small_v +-0.03 m/s, small_p +-0.004 m (joint positions: 0 is the cable length
    at the spawn pose), big_v a random sign times 0.08 .. 0.2 m/s, big_p a random sign times 0.01 .. 0.03 m.  Under `integral`
    small_v is a random sign times HOLD_FREE .. 0.03: no cable falls into the hold branch there.  (A cable that does switches to a
    Pid whose window is stale, and the command that follows reaches the shipped cmdLimit of 100 - which `integral`, with its
    large anti-windup increments, must not meet.  The `command` variants keep such cables: their increments stay small.)"""
    small_v = rng.uniform(-0.03, 0.03, (batch, n))
    if variant == "integral":
        small_v = random_sign(rng, (batch, n)) * rng.uniform(HOLD_FREE, 0.03, (batch, n))
    return {
        "small_v": small_v.astype(np.float32),
        "small_p": rng.uniform(-0.004, 0.004, (batch, n)).astype(np.float32),
        "big_v": (random_sign(rng, (batch, n)) * rng.uniform(0.08, 0.2, (batch, n))).astype(np.float32),
        "big_p": (random_sign(rng, (batch, n)) * rng.uniform(0.01, 0.03, (batch, n))).astype(np.float32),
    }


def case_inputs(pkg, cell, variant):
    """(own Config, Config under the variant, environment switches, float32 start poses, commands) of a case."""
    own, cfg, env, seed = case_config(pkg, cell, variant)
    rng = np.random.default_rng(seed)
    pose = start_poses(cfg.model, rng)
    return own, cfg, env, pose, commands(rng, B, cfg.n_cables, variant)


def play(variant, cmds, sims):
    """Generator over the script: sends every Joy to every simulator of `sims` and yields (segment index, steps) at every run -
    the caller advances ALL simulators by that many steps before it resumes."""
    for j, seg in enumerate(SCRIPTS[variant]):
        if seg[0] == "run":
            yield j, seg[1]
            continue
        kind, key, sign = seg
        cmd = np.float32(sign) * cmds[key]
        assert cmd.dtype == np.float32
        for sim in sims:
            getattr(sim, SETTER[kind])(cmd)


# ---- the hold ladder -----------------------------------------------------------------------------------------------------------
LADDER_EPS = (0.001, 0.004, 0.01, 0.0)
LADDER_CHECKPOINTS = (1, 2, 5, 12, 20)
LADDER_SEED = 9400
SUBNORMAL = np.float32(1.401298464324817e-45)  # 2^-149
SMALLEST_NORMAL = np.finfo(np.float32).tiny    # 2^-126


def ladder_magnitudes(eps):
    e_f = np.float32(eps)
    if eps != 0.0:
        return np.array([0.0, np.nextafter(e_f, np.float32(0.0)), e_f, np.nextafter(e_f, np.float32(np.inf)), 0.03], dtype=np.float32)
    return np.array([0.0, SUBNORMAL, SMALLEST_NORMAL, 0.03], dtype=np.float32)


def ladder_values(eps):
    """Every value of the ladder with both signs (+0 and -0 are two values), float32."""
    m = ladder_magnitudes(eps)
    return np.concatenate([m, -m]).astype(np.float32)


def ladder_targets(eps, batch, n):
    """(first Joy, second Joy), float32 [batch, n]: per cable a value of the ladder; the second Joy is the first with the cables of
    every robot rotated by a per-robot amount (1 .. n - 1), so that cables change branch in both directions."""
    rng = np.random.default_rng(LADDER_SEED + int(round(eps * 1e6)))
    vals = ladder_values(eps)
    first = vals[rng.integers(0, len(vals), (batch, n))]
    shift = rng.integers(1, n, batch)
    second = np.stack([np.roll(first[r], shift[r]) for r in range(batch)])
    assert first.dtype == np.float32 and second.dtype == np.float32
    return first, second


def velocity_branch(t, eps):
    """The reference's rule (JFC.cpp:72), in double: True where the velocity Pid runs."""
    return np.abs(np.asarray(t, dtype=np.float32).astype(np.float64)) > float(eps)


def rounded_threshold(eps):
    """What the host hands the float32 kernels: the largest float32 that is not above eps."""
    e = np.float32(eps)
    if float(e) > float(eps):
        e = np.nextafter(e, np.float32(-np.inf))
    return e


def velocity_branch_float32(t, eps):
    """The float32 kernels' rule: a float32 target against rounded_threshold(eps)."""
    return np.abs(np.asarray(t, dtype=np.float32)) > rounded_threshold(eps)


# ---- the rollout case ----------------------------------------------------------------------------------------------------------
ROLLOUT = dict(B=12, S=16, H=24, n=8, seed=9500, eps=0.004, warm=30)
ROLLOUT_HANDLES = {"fast": dict(), "general": dict(velocityEpsilon=ROLLOUT["eps"]), "f64": dict(precision=64)}


def rollout_ref(ora):
    """The reference position of the cost [B, 3], float32: 0.01 m above where the oracle's robots are."""
    return ora.raw_state()[0][:, :3].astype(np.float32) + np.float32([0.0, 0.0, 0.01])


def rollout_inputs(pkg, handle, perturbation=0.01):
    """(Config under `command`, float32 start poses, commands [B, H, S, n] float32) of the rollout case: the nominal sequence is
    drawn from big_v, every sample adds +-`perturbation`; on the general handle a quarter of the entries are ladder values."""
    r = ROLLOUT
    cfg = apply(pkg.Config(model=pkg.eight_cable_model(), batch=r["B"], stages=3, **ROLLOUT_HANDLES[handle]), "command")
    rng = np.random.default_rng(r["seed"])
    pose = start_poses(cfg.model, rng, r["B"])
    shape = (r["B"], r["H"], 1, r["n"])
    nominal = random_sign(rng, shape) * rng.uniform(0.08, 0.2, shape)
    cmds = (nominal + rng.uniform(-perturbation, perturbation, (r["B"], r["H"], r["S"], r["n"]))).astype(np.float32)
    if handle == "general":
        rl = np.random.default_rng(r["seed"] + 1)
        vals = ladder_values(r["eps"])
        pick = rl.random(cmds.shape) < 0.25
        cmds[pick] = vals[rl.integers(0, len(vals), int(pick.sum()))]
    return cfg, pose, cmds
