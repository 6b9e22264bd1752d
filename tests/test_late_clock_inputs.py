"""The inputs of tests/test_gpu_late_clock.py can expose a defect: established on the oracle and numpy alone (no GPU).

  origins      every origin the GPU module uses is a multiple of PERIOD[kind] (or that + 3), the run straddles the crossing with MARGIN
               steps on either side, PERIOD is a common multiple of the ring and window lengths of the kind's Config (late_clock.rings_of).
  live Pids    run from step 0 over the same number of steps, the oracle keeps every robot inside the edge box of the workspace
               (workspace_poses.BOXES["E"]) and, at every checkpoint within 8 steps of relative step c, the efforts of at least half of
               the cables are neither zero (|effort| > 1 mN) nor on the clamp (|effort| < 0.999 effort limit).
  straddling   on kinds with the hold branch the switch robots cover every wavefront, none of them is reset at c - 2, and a chosen
               cable's Pid is called on a full window with samples from both sides of c and a gap between them (late_clock.straddling:
               the script's switch steps and the hold rule |target| <= velocityEpsilon, restated); on the oracle the chosen cables'
               efforts move by newtons at the switch steps, so the switch is not idle.  (The oracle's `pid` topic speaks of one cable
               of robot 0 only: the per-cable Pid is taken from the rule.)
  decimation   for publish periods 0.0025 and 0.0035 and every origin used, the pattern sim_time(S + k) - last > period, restated as
               cdpr_engine_launch.hip and oracle/cdpr_oracle.c spell it, is the origin-0 pattern, and no comparison is within 1e-6 s of
               equality (doubles at t = 4.3e6 s resolve 1e-9 s; a period that is a multiple of dt would sit ON equality and is not used).
  verdicts     done_rules.done_reference for the timeout cases of the GPU module gives counts strictly between 0 and B on both sides of
               the 2^32 wrap.
"""
from math import lcm

import numpy as np
import pytest

import copy_robots as cr
import done_rules as dr
import late_clock as lc
import parity
import per_robot_kinds as prk
import robot_histories as ri
import workspace_poses as wp

clean_env = prk.clean_env

B = lc.B
KINDS = list(prk.HANDLES)
HOLD_KINDS = [k for k in KINDS if "velocityEpsilon" in prk.HANDLES[k][1]]
PERIODS = (0.0025, 0.0035)


def config(pkg, name, monkeypatch):
    return lc.kind_config(pkg, name, monkeypatch) if name in prk.HANDLES else lc.cell_config(pkg, name, monkeypatch)[0]


# ---- origins -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", KINDS + list(wp.CELLS))
def test_origins_are_aligned_and_the_run_straddles_the_crossing(pkg, monkeypatch, name):
    cfg = config(pkg, name, monkeypatch)
    rings = lc.rings_of(cfg)
    assert lc.PERIOD[name] % lcm(*rings) == 0, f"{name}: PERIOD {lc.PERIOD[name]} is no common multiple of {rings}"
    for crossing in lc.CROSSINGS:
        for origin, residue in ((lc.origin_for(name, crossing), 0), (lc.odd_origin_for(name, crossing), lc.ODD)):
            assert origin % lc.PERIOD[name] == residue, (name, crossing, origin)
            steps = lc.run_length(origin, crossing)
            assert crossing - origin >= lc.MARGIN - residue and origin + steps - crossing == lc.MARGIN and steps <= 1088 + lc.ODD, (name, crossing, steps)
        assert lc.origin_for(name, crossing) + lc.PERIOD[name] > crossing - lc.MARGIN, f"{name}: not the LARGEST aligned origin"


def test_the_general_origin_of_section_c_ends_on_the_last_step_allowed():
    assert 2 ** 31 - 60 + 59 == 2 ** 31 - 1


# ---- live Pids, switches that matter ---------------------------------------------------------------------------------------------
def oracle_run(pkg, oracle, cfg, seed, c, pose):
    """{relative step: (pose, effort)} at every checkpoint of the script, on the oracle alone"""
    ora = parity.oracle_at(oracle, cfg, pose)
    out = {}

    def check(t, rows):
        p, _, _, _, e = parity.observed(ora)
        out[t] = (np.array(p), np.array(e))

    lc.play([], ora, lc.script(cfg, seed, c), c + lc.MARGIN, lambda sim, k, is_oracle: sim.update(k), check)
    ora.close()
    return out


def assert_live(cfg, run, c, where):
    box, lim = wp.BOXES["E"], float(cfg.to_struct().effort_limit)
    near = [t for t in run if abs(t - c) <= 8]
    assert len(near) >= 5, f"{where}: {len(near)} checkpoints around the crossing"
    for t, (p, e) in run.items():
        assert np.isfinite(p).all() and (np.abs(p[:, :2]) <= box["dxy"]).all() and ((p[:, 2] >= box["zlo"]) & (p[:, 2] <= box["zhi"])).all(), f"{where}: a robot left the workspace by step {t}"
    for t in near:
        e = run[t][1]
        live = (np.abs(e) > 1e-3) & (np.abs(e) < 0.999 * lim)
        assert live.mean() >= 0.5, f"{where}: only {live.mean():.2f} of the efforts are live at relative step {t}"


@pytest.mark.parametrize("crossing", lc.CROSSINGS)
@pytest.mark.parametrize("kind", KINDS)
def test_the_script_keeps_the_pids_live_on_every_kind(pkg, oracle, monkeypatch, kind, crossing):
    cfg = lc.kind_config(pkg, kind, monkeypatch)
    c = crossing - lc.origin_for(kind, crossing)
    pose = ri.history_inputs(cfg.model, 501)["pose"]
    run = oracle_run(pkg, oracle, cfg, 77, c, pose)
    assert_live(cfg, run, c, f"{kind}, 2^{crossing.bit_length() - 1}")
    if kind in HOLD_KINDS:  # the switch Joys are not idle: a chosen cable's effort moves where it changes Pids
        sw = lc.switch_robots()
        for s in lc.switch_steps(c)[1:]:
            nxt = min(t for t in run if t > s)  # (the checkpoint behind the switch: at most 6 steps on)
            moved = np.abs(run[nxt][1][sw][:, lc.SWITCH_CABLES] - run[s][1][sw][:, lc.SWITCH_CABLES]).max(axis=1)
            assert np.median(moved) > 0.1, f"{kind}: the switch at relative step {s} moves the chosen cables' efforts by {np.median(moved):.3e} N"


@pytest.mark.parametrize("cell", list(wp.CELLS))
def test_the_script_keeps_the_pids_live_on_every_cell(pkg, oracle, monkeypatch, cell):
    cfg, seed = lc.cell_config(pkg, cell, monkeypatch)
    c = 2 ** 24 - lc.origin_for(cell, 2 ** 24)
    run = oracle_run(pkg, oracle, cfg, seed, c, wp.start_poses(cfg.model, cfg.batch, np.random.default_rng(seed)))
    assert_live(cfg, run, c, cell)


# ---- straddling windows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", HOLD_KINDS + ["gen_step", "gen_split", "gen_lean"])
def test_a_window_with_a_gap_straddles_every_crossing(pkg, monkeypatch, kind):
    cfg = config(pkg, kind, monkeypatch)
    assert float(cfg.velocityEpsilon) > 0.0, kind
    sw = lc.switch_robots()
    reset = np.flatnonzero(sw & ri.reset_mask().astype(bool))
    assert set(np.flatnonzero(sw) // 64) == {0, 1, 2} and list(reset) == [B - 1] and sw[cr.copy_map()[B - 1]], "the switch robots: every wavefront; only the last is reset at c - 2, and copies a switch robot at c + 2"
    nbuf = int(cfg.velocityController.dBufferLength)
    assert nbuf == int(cfg.positionController.dBufferLength)
    for crossing in lc.CROSSINGS:
        c = crossing - lc.origin_for(kind, crossing)
        events = lc.script(cfg, 77, c)
        # the script does what pid_of_a_chosen_cable restates: the chosen cables' targets change sides of epsilon at the switch steps only
        below, seen = None, {}
        for at, action in events:
            if action[0] == "joy" and action[1] == "velocity":
                now = np.abs(action[2][sw][:, lc.SWITCH_CABLES]) <= float(cfg.velocityEpsilon)
                assert now.all() or not now.any(), (kind, at)
                if at >= 30 and below is not None and bool(now.all()) != below:
                    seen[at] = True
                below = bool(now.all())
        assert sorted(seen) == lc.switch_steps(c), f"{kind}: the chosen cables change sides at {sorted(seen)}, not at {lc.switch_steps(c)}"
        found = lc.straddling(c, nbuf)
        assert found and {p for _, p, _ in found} == {"v", "p"} or (found and nbuf > 11), f"{kind}, c = {c}: no full window with a gap straddles the crossing"
        for s, _, stamps in found:
            assert stamps[0] < c <= stamps[-1] and len(stamps) == nbuf and any(b - a > 1 for a, b in zip(stamps, stamps[1:])), (kind, s, stamps)


# ---- publish decimation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("period", PERIODS)
def test_the_publish_pattern_does_not_depend_on_the_origin(pkg, period):
    dt = float(pkg.Config(model=pkg.cube_model(), batch=1).to_struct().dt)
    assert abs(period / dt - round(period / dt)) > 0.25, "a period that is a multiple of dt sits on equality"
    for kind in prk.LAYOUTS:
        for crossing in lc.CROSSINGS:
            for origin in (lc.origin_for(kind, crossing), lc.odd_origin_for(kind, crossing)):
                steps = lc.run_length(origin, crossing)
                want, closest0 = lc.publish_pattern(0, steps, dt, period)
                got, closest = lc.publish_pattern(origin, steps, dt, period)
                assert got == want and 0 < sum(got) < steps, f"{kind}, origin {origin}, period {period}: the published steps differ from origin 0's"
                assert min(closest, closest0) >= 1e-6, f"{kind}, origin {origin}: a comparison is within {closest:.3e} s of equality"


# ---- verdict counts --------------------------------------------------------------------------------------------------------------
def timeout_cases(crossing, origin):
    """[(absolute step of the evaluation, episode starts)] of section e: the robots of ri.reset_mask() were reset at c - 2, the others
    never; evaluated at c - 1 and at c + 1 (late_clock.TIMEOUT_AT: in front of the copy at c + 2, which hands on its sources' starts)
    under max_steps = late_clock.TIMEOUT_STEPS."""
    start = np.full(B, origin & 0xFFFFFFFF, np.uint32)
    start[ri.reset_mask().astype(bool)] = np.uint32((crossing + lc.RESET_AT) & 0xFFFFFFFF)
    return [(crossing + d, start) for d in lc.TIMEOUT_AT]


@pytest.mark.parametrize("kind", prk.LAYOUTS)
def test_timeout_counts_tell_the_robots_apart_on_both_sides_of_the_wrap(pkg, kind):
    crossing = 2 ** 32
    origin = lc.origin_for(kind, crossing)
    pose = np.tile(np.asarray(pkg.cube_model().home_pose(), dtype=np.float32), (B, 1))
    for at, start in timeout_cases(crossing, origin):
        rule = pkg.DoneRule(enable=dr.TIMEOUT, max_steps=lc.TIMEOUT_STEPS)
        mask, reason, counts = dr.done_reference(rule, pose=pose, twist=np.zeros((B, 6), np.float32), fk_residual=None, infeasible=None, limit_mask=np.zeros(B, np.uint32),
                                                 start=start, step_count=at, f64=False)
        young = ri.reset_mask().astype(bool)
        assert 0 < counts[0] < B and np.array_equal(mask.astype(bool), ~young), f"{kind}, step {at}: {counts[0]} of {B} robots time out"
