"""Every kernel family and handle kind LATE in the world clock: across step 2^24 (where an int that passes through a float stops being
exact), 2^31 (where (int)step changes sign) and 2^32 (where the episode clock's low word wraps).  Helpers, origins, the script and the
reasons: tests/late_clock.py; that the inputs can tell: tests/test_late_clock_inputs.py.

CDPR_STEP_ORIGIN puts a handle MARGIN = 48 steps in front of a crossing; its twin is a plain handle (the variable unset) stepped through
the same script, the oracle runs from step 0.  Two assertions throughout, on all B = 130 robots, after every segment of the script:
  same bits   the late handle equals its twin on everything a caller can read (late_clock.state: step count and episode starts less the
              origin), np.array_equal, no exception of any kind;
  reference   the late handle is held to the oracle at parity.TOL / TOL64 - the same-bits check would pass if both were wrong alike.
Every case first asserts that the origin took (late_clock.assert_origin_took).

  a  the family matrix: the 21 cells of workspace_poses.CELLS and the persistent one-wave kernel, across 2^24; every cell off the general
     path across 2^31 and 2^32 as well (d).  Launch forms: one-step launches, update(k, 10), and - uniform handles - every Joy as a
     one-batch schedule (cdpr_update_scheduled_kind: the stream kernel of the 4-cable lane-pair handle).
     test_zy_every_family_ran_late.
  b  launch forms: per_robot_kinds.HANDLES in the six forms of tests/launch_forms.py across 2^24, the kinds off the general path across
     2^31 (d) and 2^32 (e); reset_robots at c - 2, copy_robots at c + 2; one MPC rollout at c - 1, its horizon across c, against the
     oracle's and the twin's; the timeout verdict and the AGE observation at c - 1 and c + 1 (reset robots young, the others old);
     reset_done_device at the end.
  c  the general path's refusal at 2^31 (int32 stamps): the last step allowed runs and equals the twin; the next update is refused in
     three forms, and the rollout by its horizon, the handle bit for bit as it was and a pending command still pending; cdpr_reset
     makes it step again.
  f  odd origins (origin_for + 3, twin at origin 3), one kind per record layout and crossing.
  g  publish decimation (periods 0.0025 and 0.0035) and the `pid` topic late: the published steps are the twin's and the restated rule's.
  h  cdpr_reset returns a late handle to its origin: 30 steps on it equals a fresh handle of the same origin.
"""
import numpy as np
import pytest

import done_handles as gd
import done_rules as dr
import env_view as ev
import late_clock as lc
import launch_forms as lf
import parity
import per_robot_kinds as prk
import robot_histories as ri
import workspace_poses as wp

pytestmark = pytest.mark.gpu

clean_env = prk.clean_env  # (autouse here too: clears CDPR_STEP_ORIGIN with the routing overrides)

B = lc.B
UNSUPPORTED = -3  # CDPR_ERR_UNSUPPORTED (include/cdpr.h)
RAN = {}          # section a: cell -> kernel names that ran on late handles
PERSIST = "persist"  # the persistent one-wave kernel: the `step` cell under CDPR_PERSIST=1 (no family of workspace_poses.FAMILIES)
CELLS = list(wp.CELLS) + [PERSIST]


def power(crossing):
    return f"2^{crossing.bit_length() - 1}"


def crossings_of(name):
    """a general kind keeps int32 stamps: it refuses at 2^31 (section c) and is proven up to there"""
    return lc.CROSSINGS[:1] if name in lc.GENERAL else lc.CROSSINGS


class Player(lf.Player):
    """launch_forms.Player with the Joy of a script event held back until its segment is run (form sched sends it as a schedule), and
    with the unmasked Joys of a uniform handle"""
    held = None

    def advance(self, k):
        joy, self.held = self.held, None
        if joy is None:
            return self.run(k)
        _, kind, rows, mask = joy
        if mask is not None:
            return self.joy(kind, rows, mask, k)
        s = self.sim
        if self.form != "sched":
            assert getattr(s, lf.SETTER[kind])(rows) == 0
            return self.run(k)
        d_rows = s.device_upload(np.ascontiguousarray(rows, dtype=np.float32).reshape(1, self.cfg.batch, -1))
        s.update_scheduled(k, k, d_rows, kind=kind)
        s.synchronize()
        s.device_free(d_rows)
        self._log(k)


def apply(p, action, is_oracle=False):
    if action[0] == "joy":
        p.held = action
    else:
        lc.apply(p.sim, action, is_oracle)


def advance(p, k, is_oracle):
    p.advance(k)


def cell_config(pkg, cell, monkeypatch):
    if cell != PERSIST:
        return lc.cell_config(pkg, cell, monkeypatch)
    cfg, seed = lc.cell_config(pkg, "step", monkeypatch)
    monkeypatch.delenv("CDPR_ONESTEP")
    monkeypatch.setenv("CDPR_PERSIST", "1")
    return cfg, seed + 50


def run_case(pkg, oracle, monkeypatch, cfg, name, crossing, origin, twin_origin, forms, pose, seed, hooks=None, with_oracle=True):
    """The script across `crossing` on late handles in `forms`, the twin (one-step launches) and the oracle; after every segment: each
    late form against the twin, the first against the oracle; hooks {relative step or "end": f(players, twin, ora, rows)}."""
    where = f"{name}, {power(crossing)}, origin {origin}"
    c = crossing - origin
    steps = c + lc.MARGIN
    twin, late = lc.pair(pkg, cfg, monkeypatch, origin, twin_origin, pose, late=len(forms), where=where)
    tw = Player(twin, "one", cfg)
    players = [Player(e, form, cfg) for e, form in zip(late, forms)]
    ora = Player(parity.oracle_at(oracle, cfg, pose), "oracle", cfg) if with_oracle else None
    t0 = twin_origin or 0
    worst = {}

    def check(t, rows):
        want = lc.state(twin, cfg, t0)
        assert int(want["step_count"]) == t, (where, t)
        for p in players:
            lc.assert_same(lc.state(p.sim, cfg, origin), want, f"{where}, relative step {t}: form {p.form} against the twin at origin {t0}")
        if ora is not None:
            w = lc.against_the_oracle(players[0].sim, ora.sim, cfg, f"{where}, relative step {t}", rows=rows)
            for k, v in w.items():
                worst[k] = max(worst.get(k, 0.0), v[0])
        if hooks and t in hooks:
            hooks[t](players, tw, ora, rows)

    # (the twin among the engines; the oracle apart: it gets the recipe of a reset and no copy)
    lc.play(players + [tw], ora, lc.script(cfg, seed, c), steps, advance, check, apply)
    assert players[0].sim.step_count == crossing + lc.MARGIN, where
    if hooks and "end" in hooks:
        hooks["end"](players, tw, ora, None)
    if worst:
        print(f"late clock, {where}: " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    names = {n for p in players for _, n in p.launches}
    for p in players + [tw] + ([ora] if ora else []):
        p.close()
    return names


# ---- a (and d, e on the families) ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell,crossing", [(cell, x) for cell in CELLS for x in crossings_of(cell)], ids=lambda v: power(v) if isinstance(v, int) else v)
def test_the_family_matrix_late(pkg, oracle, monkeypatch, cell, crossing):
    cfg, seed = cell_config(pkg, cell, monkeypatch)
    pose = wp.start_poses(cfg.model, cfg.batch, np.random.default_rng(seed))
    forms = ("one", "fused10") + (() if cfg.perRobotCommands else ("sched",))
    names = run_case(pkg, oracle, monkeypatch, cfg, cell, crossing, lc.origin_for(cell, crossing), None, forms, pose, seed)
    RAN.setdefault(cell, set()).update(names)
    if cell == PERSIST:
        assert any("PERSIST" in n for n in names), names


# ---- b (and d, e on the kinds) -------------------------------------------------------------------------------------------------
def forms_hooks(pkg, cfg, kind, c, pose):
    general = kind in lf.GENERAL
    roll = lf.rollout_inputs(cfg, pose, 331)
    rule = pkg.DoneRule(enable=dr.TIMEOUT, max_steps=lc.TIMEOUT_STEPS)
    young = ri.reset_mask().astype(bool)

    def rollout(players, tw, ora, rows):
        where = f"{kind}: the rollout at c - 1 over {roll['cmds'].shape[1]} steps"
        assert roll["cmds"].shape[1] > 2, where
        before = lc.state_everything(players[0].sim, cfg)
        want = tw.sim.rollout_velocity(roll["cmds"], roll["ref"])
        assert tw.sim.kernel_name == pkg.plan_kernel(cfg, roll["cmds"].shape[1], flags=pkg._abi.PLAN_ROLLOUT), (where, tw.sim.kernel_name)
        for p in players:
            got = p.sim.rollout_velocity(roll["cmds"], roll["ref"])
            assert got.shape == (B, lf.SAMPLES) and np.isfinite(got).all() and np.array_equal(got, want), f"{where}: form {p.form} differs from the twin's costs"
            assert p.sim.kernel_name == tw.sim.kernel_name, where
        oc = ora.sim.rollout_velocity(roll["cmds"], roll["ref"].astype(np.float64))
        err, bound = float(np.abs(want - oc).max()), lf.rollout_tolerance(cfg, general, oc)
        print(f"late clock ROLLOUT {where}: max |cost - oracle| {err:.3e} = {err / bound:.3f} x the tolerance")
        assert err <= bound, f"{where}: the costs differ from the oracle's by {err:.3e} (tolerance {bound:.3e})"
        lc.assert_same(lc.state_everything(players[0].sim, cfg), before, f"{where} changed what a getter returns")

    def verdict(players, tw, ora, rows):
        where = f"{kind}: the timeout verdict at relative step {tw.sim.step_count}"
        want = tw.sim.evaluate_done(rule)
        assert np.array_equal(want[0].astype(bool), ~young), f"{where}: the twin does not tell the reset robots from the others"
        for p in players:
            got = p.sim.evaluate_done(rule)
            gd.assert_verdict(got, gd.expect(p.sim, cfg, rule), f"{where}, form {p.form}: done_reference on the late handle's own getters")
            gd.assert_verdict(got, want, f"{where}, form {p.form}: the twin's verdict")
            assert 0 < got[2][0] < B, where
            obs = p.sim.observe(ev.AGE)
            assert np.array_equal(obs, ev.observation_reference(ev.AGE, **ev.view_getters(p.sim, cfg))) and np.array_equal(obs, tw.sim.observe(ev.AGE)), f"{where}: the AGE column"
            assert obs.max() >= lc.MARGIN - lc.ODD - 1 and obs[young].max() <= 3.0, (where, obs.max(), obs[young].max())

    def end(players, tw, ora, rows):
        where = f"{kind}: reset_done_device behind the run"
        two = (np.arange(B) % 5 == 1).astype(np.uint8)
        late_rule = pkg.DoneRule(enable=dr.TIMEOUT, max_steps=10)
        for p in [tw, players[0]]:
            p.sim.reset_robots(two)
            p.sim.update(5)
        want = tw.sim.evaluate_done(late_rule)
        got = players[0].sim.evaluate_done(late_rule)
        gd.assert_verdict(got, want, where)
        assert np.array_equal(got[0].astype(bool), ~two.astype(bool)), where
        for p in [tw, players[0]]:
            p.sim.reset_done_device(late_rule)
            p.sim.update(3)
        s = players[0].sim
        start = s.episode_start()
        assert (start[~two.astype(bool)] == np.uint32((s.step_count - 3) & 0xFFFFFFFF)).all() and (start[two.astype(bool)] == np.uint32((s.step_count - 8) & 0xFFFFFFFF)).all(), where
        lc.assert_same(lc.state(s, cfg, s.step_count - tw.sim.step_count), lc.state(tw.sim, cfg, 0), f"{where}, 3 steps on")

    hooks = {c - 1: lambda *a: (rollout(*a), verdict(*a)), c + 1: verdict, "end": end}
    assert lc.RESET_AT < -1 and lc.COPY_AT > 1 and c - 1 in lc.switch_steps(c) and c + 1 in lc.switch_steps(c)  # (both are checkpoints, between reset and copy)
    return hooks


@pytest.mark.parametrize("kind,crossing", [(kind, x) for kind in prk.HANDLES for x in crossings_of(kind)], ids=lambda v: power(v) if isinstance(v, int) else v)
def test_launch_forms_late(pkg, oracle, monkeypatch, kind, crossing):
    cfg = lc.kind_config(pkg, kind, monkeypatch)
    origin = lc.origin_for(kind, crossing)
    pose = ri.history_inputs(cfg.model, 501)["pose"]
    hooks = forms_hooks(pkg, cfg, kind, crossing - origin, pose)

    def named_at_the_end(players, tw, ora, rows):
        prk.named(players[0].sim, kind)
        for p in players:
            last, name = p.launches[-1]
            assert name == pkg.plan_kernel(cfg, last), (kind, p.form, last, name)
        hooks["end"](players, tw, ora, rows)

    run_case(pkg, oracle, monkeypatch, cfg, kind, crossing, origin, None, lf.FORMS, pose, 77, dict(hooks, end=named_at_the_end))


# ---- c -------------------------------------------------------------------------------------------------------------------------
def refused(pkg, call, where):
    with pytest.raises(pkg.CdprError) as e:
        call()
    assert e.value.code == UNSUPPORTED and lc.REFUSAL in str(e.value), f"{where}: {e.value}"


@pytest.mark.parametrize("kind", [k for k in prk.HANDLES if k in lc.GENERAL])
def test_the_general_path_refuses_at_2_31(pkg, monkeypatch, kind):
    cfg = lc.kind_config(pkg, kind, monkeypatch)
    origin = 2 ** 31 - 60
    t0 = origin % lc.PERIOD[kind]
    pose = ri.history_inputs(cfg.model, 501)["pose"]
    twin, (late,) = lc.pair(pkg, cfg, monkeypatch, origin, t0, pose, where=kind)
    a = ri.after_inputs(cfg.model, 78)
    roll = lf.rollout_inputs(cfg, pose, 331)
    ones = np.ones(B, np.uint8)

    def same(label):
        lc.assert_same(lc.state(late, cfg, origin), lc.state(twin, cfg, t0), f"{kind}, {label}")

    for e in (twin, late):
        assert e.set_velocity_command(a["v"], mask=ones) == 0
        e.update(58, 10)
    same("58 steps in front of the boundary")
    for e in (twin, late):
        assert e.set_position_command(a["p"], mask=a["p_mask"]) == 0  # ... stays pending through every refusal below
    d_rows = late.device_upload(np.ascontiguousarray(a["v"]).reshape(1, B, -1))
    d_mask = late.device_upload(ones.reshape(1, B))

    def every_refusal(k, label):
        before, count = lc.state_everything(late, cfg), late.step_count
        refused(pkg, lambda: late.update(k), f"{kind}, {label}: update")
        refused(pkg, lambda: late.update(k, 10), f"{kind}, {label}: fused update")
        refused(pkg, lambda: late.update_record(k, 10), f"{kind}, {label}: recorded update")
        refused(pkg, lambda: late.update_scheduled(k, k, d_rows, kind="velocity", d_robot_masks=d_mask), f"{kind}, {label}: scheduled update")
        refused(pkg, lambda: late.rollout_velocity(np.ascontiguousarray(roll["cmds"][:, :k]), roll["ref"]), f"{kind}, {label}: rollout")
        late.synchronize()
        assert late.step_count == count, f"{kind}, {label}: a refused call moved the clock"
        lc.assert_same(lc.state_everything(late, cfg), before, f"{kind}, {label}: a refused call changed the handle")

    every_refusal(2, "two steps with one left")
    for e in (twin, late):
        e.update(1)  # the last step allowed; it latches the position Joy that was pending through five refusals
    assert late.step_count == 2 ** 31 - 1
    same("on step 2^31 - 1: the pending command survived the refusals")
    every_refusal(1, "one step on the boundary")
    late.device_free(d_rows), late.device_free(d_mask)
    # cdpr_reset makes the handle step again, from its origin
    for e in (twin, late):
        e.reset()
        lc.put(e, cfg, pose)
    lc.assert_origin_took(late, origin, f"{kind}, after cdpr_reset")
    for e in (twin, late):
        assert e.set_velocity_command(a["v"], mask=a["v_mask"]) == 0
        e.update(12)
    same("12 steps after cdpr_reset")
    twin.close(), late.close()


# ---- f -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,crossing", [(kind, x) for kind in prk.LAYOUTS for x in crossings_of(kind)], ids=lambda v: power(v) if isinstance(v, int) else v)
def test_odd_origins(pkg, oracle, monkeypatch, kind, crossing):
    cfg = lc.kind_config(pkg, kind, monkeypatch)
    pose = ri.history_inputs(cfg.model, 502)["pose"]
    run_case(pkg, oracle, monkeypatch, cfg, kind, crossing, lc.odd_origin_for(kind, crossing), lc.ODD, ("one", "fused10", "long"), pose, 78)


# ---- g -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("period", (0.0025, 0.0035))
@pytest.mark.parametrize("kind,crossing", [(kind, x) for kind in prk.LAYOUTS for x in crossings_of(kind)[:2]], ids=lambda v: power(v) if isinstance(v, int) else v)
def test_publish_decimation_and_the_pid_topic_late(pkg, oracle, monkeypatch, kind, crossing, period):
    from dataclasses import replace

    cfg = replace(lc.kind_config(pkg, kind, monkeypatch, more_stages=pkg._abi.STAGE_PID_DEBUG), publishPeriod=period)
    origin = lc.origin_for(kind, crossing)
    c, where = crossing - origin, f"{kind}, {power(crossing)}, period {period}"
    pose = ri.history_inputs(cfg.model, 503)["pose"]
    twin, (late, fused) = lc.pair(pkg, cfg, monkeypatch, origin, None, pose, late=2, where=where)
    ora = parity.oracle_at(oracle, cfg, pose)
    want, _ = lc.publish_pattern(0, c + lc.MARGIN, float(cfg.to_struct().dt), period)
    published, last, t = [], None, 0
    f64 = cfg.precision == 64
    for at, action in lc.script(cfg, 79, c) + [(c + lc.MARGIN, None)]:
        if at > t:
            fused.update(at - t, 10)
        for _ in range(at - t):
            for e in (twin, late, ora):
                e.update(1)
            q_late, q_twin = (e.observables_f64()[0] if f64 else e.observables()[0] for e in (late, twin))
            assert np.array_equal(q_late, q_twin), f"{where}: the published joint positions differ from the twin's at relative step {t}"
            published.append(last is None or not np.array_equal(q_late, last))
            last = q_late
            t += 1
        want_state = lc.state(twin, cfg, 0)
        lc.assert_same(lc.state(late, cfg, origin), want_state, f"{where}, relative step {t}: one-step launches against the twin")
        lc.assert_same(lc.state(fused, cfg, origin), want_state, f"{where}, relative step {t}: fused launches against the twin")
        lc.against_the_oracle(late, ora, cfg, f"{where}, relative step {t}")
        assert np.abs(late.pid_debug() - ora.pid_debug()).max() < (1e-5 if f64 else 5e-2), f"{where}: the pid topic at relative step {t}"
        if action is None:
            break
        if action[0] == "joy":  # (the script's reset and copy are sections b's: here every robot stays with the oracle)
            for e in (twin, late, fused, ora):
                lc.apply(e, action, e is ora)
    # step 0 publishes nothing (the observables before it are the home pose: `published` sees a change only where a step published)
    assert published[1:] == want[1:] and 0 < sum(want) < len(want), f"{where}: the published steps {np.flatnonzero(published)[:12]} are not those of the rule {np.flatnonzero(want)[:12]}"
    for e in (twin, late, fused, ora):
        e.close()


# ---- h -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,crossing", [(kind, crossings_of(kind)[-1]) for kind in prk.LAYOUTS], ids=lambda v: power(v) if isinstance(v, int) else v)
def test_cdpr_reset_returns_to_the_origin(pkg, monkeypatch, kind, crossing):
    cfg = lc.kind_config(pkg, kind, monkeypatch)
    origin = crossing - 17  # (any origin: 30 steps from it cross the crossing)
    h, a = ri.history_inputs(cfg.model, 504), ri.after_inputs(cfg.model, 505)
    used, fresh = lc.create(pkg, cfg, monkeypatch, origin, 2)
    lc.assert_origin_took(used, origin, kind)
    lc.put(used, cfg, h["pose"])
    ri.play_history([used], h)
    used.reset_robots(ri.reset_mask(), a["pose"])
    used.update(3)
    assert used.step_count == origin + ri.HISTORY + 3 and (used.episode_start() != np.uint32(origin & 0xFFFFFFFF)).any()
    used.reset()
    lc.assert_origin_took(used, origin, f"{kind}, after cdpr_reset")
    for k in (1, 9, 20):
        for e in (used, fresh):
            if k == 9:
                assert e.set_velocity_command(a["v"], mask=a["v_mask"]) == 0
            e.update(k, 10 if k == 20 else 1)
        lc.assert_same(lc.state_everything(used, cfg), lc.state_everything(fresh, cfg), f"{kind}: {k} steps further behind cdpr_reset against a fresh handle at origin {origin}")
    assert used.step_count == origin + 30 > crossing
    used.close(), fresh.close()


# ---- coverage ------------------------------------------------------------------------------------------------------------------
def test_zy_every_family_ran_late():
    """as test_zy_every_family_ran of tests/test_gpu_workspace.py, on what section a recorded of its LATE handles"""
    missing = [fam for fam, (cell, pred) in wp.FAMILIES.items() if not any(pred(k) for k in RAN.get(cell, ()))]
    assert not missing, (f"families that did not run on a late handle IN THIS PROCESS: {missing}.  This test reads what test_the_family_matrix_late recorded: "
                         f"run the whole module in one process.  Ran: { {c: sorted(v) for c, v in RAN.items()} }")
    print(f"late clock: all {len(wp.FAMILIES)} families ran on a late handle")
