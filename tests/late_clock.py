"""What tests/test_late_clock_inputs.py (CPU) and tests/test_gpu_late_clock.py (GPU) share: handles late in the world clock.

The world-step counter is an input of every kernel (ring slots, int32 stamps, the fp64 Pid words, the episode clock, the publish
decimation, "the first update since Load").  CDPR_STEP_ORIGIN=<step> makes cdpr_create start the clock there (and cdpr_reset return
there): `create` sets it around the create call alone (cdpr_create is the only reader), so a handle stands 48 steps in front of 2^24,
2^31 or 2^32 at once.  The origin is a pure relabelling: a handle created at origin S does at step S + k what a handle created at
origin 0 does at step k, to the bit, on everything a caller can read but the names of the absolute step (step_count, episode_start),
which `relabelled` subtracts.  The twin of a late handle is therefore a plain handle with the variable unset, and the oracle runs from
step 0: the seam is part of neither reference.

PERIOD[kind]: steps after which the kind's ring placement repeats - where in its rings the sample of a step sits is a function of the
absolute step, so an origin that is a multiple of PERIOD leaves every sample where the twin has it (`origin_for`), and one that is
not (`odd_origin_for`: + 3, the twin then a handle at origin 3) covers the residues the aligned origins cannot.

pytest rewrites asserts only in test modules, so every assert here carries its message.
"""
import numpy as np

import copy_robots as cr
import parity
import per_robot_kinds as prk
import robot_histories as ri
import workspace_poses as wp
import padded_stride as ps
from padded_stride import assert_same, state_everything  # noqa: F401  (the late-clock modules take them from here)

ENV = "CDPR_STEP_ORIGIN"
B = ri.B
EPS = ri.EPS
CROSSINGS = (2 ** 24, 2 ** 31, 2 ** 32)
MARGIN = 48  # steps on either side of a crossing: fills a 32-sample window, and a robot enters the general path's hot rows after 11
WRAP = 2 ** 32
ODD = 3
REFUSAL = "general controller path: world-step counter would pass 2^31"  # (run_steps, cdpr_engine_launch.hip; the rollout: cdpr_engine_rollout.hip)

# Ring lengths, from the code:
#   K_WIN = 10        kWin, cdpr_step_kernel.hpp: the register-resident kernels' ring of prior errors; ring_slot_of(step) = (step + 8) mod 10
#                     (cdpr_engine_internal.hpp), and the precision = 64 kernels' ring, ring_slot_of(step, win64) = (step + w - 2) mod w
#   K_WIN_LONG = 31   kWinLong, cdpr_step_kernel_f64.hpp: win64 of a precision = 64 handle with windows of 12 .. 32 samples
#   general path      "the ring slot of a sample is its stamp mod nbuf" (cdpr_general_step.hpp): nbuf = dBufferLength of each Pid
#   hold windows      kHoldWin = 11 / kHoldWinLong = 32 (cdpr_step_kernel_f64.hpp): their head moves by COUNT, not by the step
#                     (hold_finish64: head_old + 1), so they add no period of their own; PERIOD takes their length in all the same -
#                     a multiple of a period is a period, and a head that were taken from the step one day stays covered.
K_WIN, K_WIN_LONG = 10, 31


def rings_of(cfg):
    """The ring lengths the handle's kernels place samples in by the step, and the window lengths beside them (see above)."""
    nb = sorted({int(cfg.velocityController.dBufferLength), int(cfg.positionController.dBufferLength)})
    hold = float(cfg.velocityEpsilon) >= 0.0
    if cfg.precision == 64:
        ring = K_WIN_LONG if max(nb) > K_WIN + 1 else K_WIN
        return [ring] + (nb if hold or max(nb) > K_WIN + 1 else [])
    general = hold or max(nb) > K_WIN + 1 or any(f.cascade for p in (cfg.velocityController, cfg.positionController) for f in (p.pFilter, p.dFilter))
    return nb if general else [K_WIN]


PERIOD = {
    # register-resident kinds and families: kWin
    "fast_n8": 10, "fast_n4": 10, "fast_n7": 10,
    # general kinds on 11-sample windows: stamp mod 11
    "general_n8": 11, "general_lean_hot": 11, "general_one_wave": 11,
    # 32-sample windows: stamp mod 32
    "general_long": 32,
    # precision = 64: ring of kWin; with the hold branch lcm(10, 11); kWinLong = 31 beside 32-sample hold windows: 31 * 32
    "fp64_n8": 10, "fp64_hold_n8": 110, "fp64_hold_long": 992,
}
# the cells of the workspace matrix: the general path's three on 11-sample windows, every other cell a ring of kWin
PERIOD.update({cell: (11 if cell.startswith("gen_") else 10) for cell in wp.CELLS})
PERIOD["persist"] = 10  # the persistent one-wave kernel (the `step` cell under CDPR_PERSIST=1, tests/test_gpu_late_clock.py): kWin

GENERAL = ("general_n8", "general_lean_hot", "general_long", "general_one_wave", "gen_step", "gen_split", "gen_lean")  # int32 stamps: refuse at 2^31


def origin_for(kind, crossing):
    """the largest multiple of PERIOD[kind] that leaves MARGIN steps in front of the crossing"""
    return (crossing - MARGIN) // PERIOD[kind] * PERIOD[kind]


def odd_origin_for(kind, crossing):
    return origin_for(kind, crossing) + ODD


def run_length(origin, crossing):
    return crossing - origin + MARGIN


def against_the_oracle(eng, ora, cfg, where, rows=None):
    """padded_stride.against_the_oracle (parity.TOL, or TOL64 on precision = 64, every quantity finite) on the robots `rows` (default: all)"""
    return ps.against_the_oracle(eng, ora, cfg, where, rows=np.ones(cfg.batch, bool) if rows is None else rows)


# ---- handles ----------------------------------------------------------------------------------------------------------------------
def create(pkg, cfg, monkeypatch, origin, count=1):
    """`count` engines created with CDPR_STEP_ORIGIN=origin, or with it removed where origin is None; the variable is gone again afterwards."""
    with monkeypatch.context() as m:
        if origin is None:
            m.delenv(ENV, raising=False)
        else:
            m.setenv(ENV, str(int(origin)))
        return [pkg.Engine(cfg, 0) for _ in range(count)]


def assert_origin_took(eng, origin, where=""):
    """Without this a case proves nothing: the handle stands at the origin and every episode starts there (age 0)."""
    assert eng.step_count == origin, f"{where}: the origin {origin} did not take (step_count {eng.step_count})"
    start = eng.episode_start()
    assert start.dtype == np.uint32 and (start == np.uint32(origin & 0xFFFFFFFF)).all(), f"{where}: episode_start is {start[:4]}, not the low word of {origin}"


def pair(pkg, cfg, monkeypatch, origin, twin_origin=None, pose=None, late=1, where=""):
    """(the twin at twin_origin - None: the variable unset -, [late handles at origin]) at `pose`, the origin checked on every one"""
    (t,) = create(pkg, cfg, monkeypatch, twin_origin)
    assert_origin_took(t, twin_origin or 0, where + ", the twin")
    ls = create(pkg, cfg, monkeypatch, origin, late)
    for e in ls:
        assert_origin_took(e, origin, where)
    if pose is not None:
        for e in [t] + ls:
            put(e, cfg, pose)
    return t, ls


def put(eng, cfg, pose):
    if cfg.precision == 64:
        eng.set_platform_state_f64(pose7=np.asarray(pose, dtype=np.float32).astype(np.float64))
    else:
        eng.set_platform_state(pose7=np.asarray(pose, dtype=np.float32))


def relabelled(state, origin):
    """a state_everything dict with the names of the absolute step taken out: the episode starts and the step count less the origin, modulo 2^32"""
    out = dict(state)
    out["start"] = (np.asarray(state["start"], dtype=np.uint32) - np.uint32(origin & 0xFFFFFFFF)).astype(np.uint32)
    out["step_count"] = np.asarray((int(state["step_count"]) - origin) % WRAP)
    return out


def state(eng, cfg, origin):
    return relabelled(state_everything(eng, cfg), origin)


# ---- the command script -----------------------------------------------------------------------------------------------------------
# Steps are RELATIVE to the handle's origin; c = crossing - origin is the relative step of the crossing.  Events, in step order:
#   0                a velocity Joy for every robot
#   20               a position Joy (offsets of +-4 mm) for the robots of group 0 (per-robot handles) or for everyone (uniform handles)
#   30, 40, ...      velocity Joys again, re-latched every 10 steps: to everyone at 30, then to alternating halves (per-robot handles)
#                    or everyone (uniform); none inside c - 6 .. c + 8, where the switch Joys below stand
#   c - 5, c - 1, c, c + 1, c + 7   the chosen cables (SWITCH_CABLES of the robots of SWITCH_ROBOTS: one or two in every wavefront)
#                    change sides of velocityEpsilon: on kinds with the hold branch such a cable changes Pids, and the Pid it comes
#                    back to has a window with a gap, fitted on its real stamps, which straddles the crossing
#   c - 2            reset_robots on ri.reset_mask() (per-robot handles)
#   c + 2            copy_robots with cr.copy_map() (per-robot handles)
SWITCH_AT = (-5, -1, 0, 1, 7)
SWITCH_CABLES = (1, 2)
RESET_AT, COPY_AT = -2, 2
TIMEOUT_AT, TIMEOUT_STEPS = (-1, 1), 5  # the timeout verdicts of the wrap: the reset robots are 1 and 3 steps old, the others at least MARGIN - 1


def switch_robots(batch=B):
    """Robots of every wavefront that ri.reset_mask() leaves alone (a reset at c - 2 empties the windows), and the last robot: the
    third wavefront of B = 130 holds robots 128 and 129 only, both of the reset mask - on a uniform handle nothing resets robot 129,
    on a per-robot handle the copy at c + 2 hands it the records of robot 65 (cr.copy_map), a switch robot."""
    m = np.zeros(batch, bool)
    m[1::7] = True
    m &= ~ri.reset_mask(batch).astype(bool)
    m[[5, 65, 66, batch - 1]] = True
    return m


def script(cfg, seed, c):
    """[(relative step, action)], sorted; actions: ("joy", kind, rows float32[B, n], mask uint8[B] or None), ("reset", mask, pose),
    ("copy", source).  Every array is drawn here once, from `seed`."""
    rng = np.random.default_rng(seed)
    n, pr = cfg.n_cables, bool(cfg.perRobotCommands)
    steps = c + MARGIN
    assert c >= MARGIN - ODD, f"script: the crossing at relative step {c} leaves no {MARGIN - ODD} steps in front of it"
    ones = np.ones(B, np.uint8) if pr else None

    def joy_rows():
        v = rng.uniform(-0.03, 0.03, (B, n)).astype(np.float32)
        v[np.abs(v) <= 2 * EPS] = np.float32(3 * EPS)  # every cable clearly on the velocity Pid ...
        v[::2, 0::4] = np.float32(0.5 * EPS)          # ... but cables 0 and 4 of the even robots, which hold position throughout
        return v

    out = []
    cur = joy_rows()
    out.append((0, ("joy", "velocity", cur.copy(), ones)))
    off = rng.uniform(-0.004, 0.004, (B, n)).astype(np.float32)
    out.append((20, ("joy", "position", off, (np.arange(B) % 3 == 0).astype(np.uint8) if pr else None)))
    quiet = range(c - 6, c + 9)
    sw = switch_robots()
    cols = np.ix_(np.flatnonzero(sw), SWITCH_CABLES)
    below = False
    for at in sorted([a for a in range(30, steps, 10) if a not in quiet] + switch_steps(c)):
        if at in switch_steps(c):
            below = not below
            sign = np.where(rng.random((int(sw.sum()), len(SWITCH_CABLES))) < 0.5, -1, 1).astype(np.float32)
            cur[cols] = np.float32(0.5 * EPS) if below else np.float32(4 * EPS) * sign
            who = sw
        else:
            new = joy_rows()
            who = np.ones(B, bool) if (at == 30 or not pr) else (np.arange(B) % 2 == (at // 10) % 2)
            new[:, SWITCH_CABLES] = cur[:, SWITCH_CABLES]  # the chosen cables move at the switch steps only
            cur[who] = new[who]
        out.append((at, ("joy", "velocity", cur.copy(), who.astype(np.uint8) if pr else None)))
    if pr:
        out.append((c + RESET_AT, ("reset", ri.reset_mask(), parity.perturbed_poses(cfg.model, B, rng, 0.02, 0.05).astype(np.float32))))
        out.append((c + COPY_AT, ("copy", cr.copy_map())))
    out.sort(key=lambda e: e[0])
    at = [e[0] for e in out]
    assert len(set(at)) == len(at) and at[-1] < steps, f"script: two events on one step, or one behind the run ({at})"
    return out


def switch_steps(c):
    return [c + d for d in SWITCH_AT]


def pid_of_a_chosen_cable(c):
    """{relative step: "v" or "p"} from step 30 on (every robot is in Velocity mode from there; a Joy at step s is latched by the update
    that runs step s): the Pid a chosen cable of a switch robot calls on a kind with the hold branch - the position Pid while its
    velocity target is at or below velocityEpsilon."""
    out, below = {}, False
    for s in range(30, c + MARGIN):
        if s in switch_steps(c):
            below = not below
        out[s] = "p" if below else "v"
    return out


def straddling(c, nbuf):
    """[(step, Pid, stamps)]: the calls at or behind c whose Pid's window (its newest nbuf calls, full) holds samples from both sides of c
    with a gap between them - what the kernels fit on the real stamps."""
    calls = pid_of_a_chosen_cable(c)
    out = []
    for s in range(c, c + MARGIN):
        stamps = [t for t in range(30, s + 1) if calls[t] == calls[s]][-nbuf:]
        if len(stamps) == nbuf and stamps[0] < c <= stamps[-1] and stamps[-1] - stamps[0] != nbuf - 1:
            out.append((s, calls[s], stamps))
    return out


# ---- playing a script -------------------------------------------------------------------------------------------------------------
def apply(sim, action, is_oracle=False):
    """one action of a script on an engine or on the oracle (the reset recipe of tests/robot_histories.py; a copy does not exist there:
    its destinations leave the comparison with the oracle, `touched_by`)"""
    if action[0] == "joy":
        _, kind, rows, mask = action
        rc = getattr(sim, wp.SETTER[kind])(rows) if mask is None else getattr(sim, wp.SETTER[kind])(rows, mask=mask)
        assert rc == 0, f"late_clock.apply: {wp.SETTER[kind]} returned {rc}"
    elif action[0] == "reset":
        ri.oracle_reset(sim, action[1], action[2]) if is_oracle else sim.reset_robots(action[1], action[2])
    elif not is_oracle:
        sim.copy_robots(action[1])


def play(engines, ora, events, steps, advance, check, apply=apply):
    """The script on `engines` (and the oracle, where given) in lock step: advance(sim, k, is_oracle) runs k steps, check(relative step,
    rows the oracle still speaks for) after every segment; apply(sim, action, is_oracle): default `apply` above."""
    t = 0
    rows = np.ones(B, bool)
    for at, action in list(events) + [(steps, None)]:
        if at > t:
            for e in engines:
                advance(e, at - t, False)
            if ora is not None:
                advance(ora, at - t, True)
            t = at
            check(t, rows)
        if action is None:
            break
        for e in engines:
            apply(e, action, False)
        if ora is not None:
            apply(ora, action, True)
        if action[0] == "copy":
            rows = rows & ~cr.destinations_of(action[1])


def kind_config(pkg, kind, monkeypatch, **more):
    """per_robot_kinds.config_of (a per-robot handle of `kind`, the kind's environment switches set)"""
    return prk.config_of(pkg, kind, monkeypatch, **more)


def cell_config(pkg, cell, monkeypatch):
    cfg, env, seed = wp.cell_config(pkg, cell)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return cfg, seed


# ---- publish decimation, restated -------------------------------------------------------------------------------------------------
def sim_time(step, dt):
    """cdpr_engine_launch.hip's sim_time and orc's: integer nanoseconds, then sec + nsec * 1e-9 in double"""
    dt_ns = int(round(dt * 1e9))
    now_ns = int(step) * dt_ns
    return float(now_ns // 1000000000) + float(now_ns % 1000000000) * 1e-9


def publish_pattern(origin, steps, dt, period):
    """([published?] per relative step, the smallest | (now - last) - period | met): `last` starts at sim_time(origin) and moves to
    every step that publishes (publish_mask, cdpr_engine_launch.hip; PLG.cpp:236-242: strict '>')"""
    last, out, closest = sim_time(origin, dt), [], np.inf
    for k in range(steps):
        now = sim_time(origin + k, dt)
        closest = min(closest, abs((now - last) - period))
        pub = (now - last) > period
        out.append(pub)
        if pub:
            last = now
    return out, closest
