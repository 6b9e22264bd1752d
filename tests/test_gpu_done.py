"""cdpr_evaluate_done / cdpr_evaluate_done_device / cdpr_reset_done_device / cdpr_get_episode_start: the verdict of a done rule computed
on the device, and the per-robot episode clock.  The verdict is specified as a pure function of what the getters return, so every
verdict here is compared - equal, not close - with tests/done_rules.py's done_reference on the engine's own getters; the closed loop
is compared with the fp64 oracle at the tolerances of tests/parity.py (TOL, TOL64) under the
oracle-side condition tests/test_done_rule_inputs.py establishes.

Handle kinds (tests/done_handles.py): one per record layout of tests/per_robot_kinds.py (fast_n8, general_lean_hot, fp64_hold_n8: per-robot commands), a
uniform n = 8 handle with FK + TD, a uniform n = 4 lane-pair handle, a uniform n = 12 handle.

  1  static verdicts   2  after real steps (FK residual, infeasible flag, travel bits; publish decimation)   3  forms and outputs
  4  evaluation changes nothing   5  the episode clock   6  reset_done_device = evaluate_done_device + reset_robots_device
  7  the closed loop against the oracle   8  refusals   9  sharded

B = 130: two full wavefronts and a ragged one, stride 192.
"""
import ctypes as C

import numpy as np
import pytest

import done_rules as dr
import parity
import per_robot_kinds as prk
import robot_histories as ri
from done_handles import B, KINDS, LAYOUTS, STRIDE, UNIFORM, assert_verdict, config_of, drive, expect, getters, limited, put

pytestmark = pytest.mark.gpu

clean_env = prk.clean_env  # (autouse here too)


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_static_verdicts(pkg, monkeypatch, kind):
    cfg = config_of(pkg, kind, monkeypatch)
    f64 = cfg.precision == 64
    rule, pose, twist = dr.static_scenario(pkg, cfg.model, f64)
    eng = pkg.Engine(cfg, 0)
    if kind == "uniform_n4_pair":
        assert eng.mapping == "lane-pair"
    put(eng, cfg, pose, twist)
    g = getters(eng, cfg)
    assert np.array_equal(g["pose"], pose, equal_nan=True) and np.array_equal(g["twist"], twist, equal_nan=True) and g["pose"].dtype == pose.dtype
    for name, d in dr.metric_margins(rule, g["pose"], g["twist"]).items():
        assert d.min() > 1e-5, f"{kind}: a robot's {name} metric is within 1e-5 relative of its threshold"
    want = dr.done_reference(rule, **g)
    got = eng.evaluate_done(rule)
    print(f"done, {kind}: counts {got[2][:10].tolist()}")
    assert_verdict(got, want, kind)
    assert set(np.unique(got[0])) == {0, 1} and got[2][1] == len(dr.NONFINITE_ROBOTS)
    for k in dr.ON_LO + dr.ON_HI:
        assert not got[1][k] & dr.WORKSPACE, (kind, k)
    for k in dr.BELOW_LO + dr.ABOVE_HI:
        assert got[1][k] == dr.WORKSPACE, (kind, k)
    assert got[1][dr.NAN_POSITION] == dr.NONFINITE and got[1][dr.INF_TWIST] == dr.NONFINITE | dr.SPEED
    # the non-finite robots are evaluated, then reset: no step runs on them
    bad = np.zeros(B, np.uint8)
    bad[list(dr.NONFINITE_ROBOTS)] = 1
    if cfg.perRobotCommands:
        eng.reset_robots(bad)
    else:
        home = np.tile(np.asarray(cfg.model.home_pose()), (B, 1))
        put(eng, cfg, np.where(bad[:, None] != 0, home, pose.astype(np.float64)).astype(pose.dtype), np.where(bad[:, None] != 0, 0.0, twist.astype(np.float64)).astype(twist.dtype))
    after = eng.evaluate_done(rule)
    assert_verdict(after, expect(eng, cfg, rule), f"{kind}, after the reset")
    assert after[2][1] == 0 and not after[1][bad != 0].any()
    eng.close()


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("period", [0.0, 0.0025], ids=["every_step", "decimated"])
@pytest.mark.parametrize("kind", KINDS)
def test_after_real_steps(pkg, monkeypatch, kind, period):
    """37 steps under tension bounds of 1 .. 12 N (the infeasible flag fires for some robots), one FK iteration per step (the
    residuals spread), travel limits of +-15 mm (some cables cross them); the FK threshold is one robot's own residual."""
    n = UNIFORM[kind][0] if kind in UNIFORM else 8
    extra = dict(publishPeriod=period)
    if n >= 6:
        extra.update(tdFMin=1.0, tdFMax=12.0, fkMaxIterations=1)
    cfg = config_of(pkg, kind, monkeypatch, limited, **extra)
    h = ri.history_inputs(cfg.model, 301)
    eng = pkg.Engine(cfg, 0)
    put(eng, cfg, h["pose"])
    drive([eng], cfg, h, ri.HISTORY)
    g = getters(eng, cfg)
    lim = g["limit_mask"] != 0
    assert 0 < lim.sum() < B, f"{kind}: the travel bits do not tell the robots apart ({int(lim.sum())})"
    enable = dr.TRAVEL
    if n >= 6:
        enable |= dr.FK_RESIDUAL | dr.INFEASIBLE
        assert 0 < (g["infeasible"] != 0).sum() < B, f"{kind}: the infeasible flag does not tell the robots apart"
        res = g["fk_residual"]
        distinct = np.unique(res)  # (fp32 handles: a few multiples of the lengths' rounding unit; precision = 64: one value per robot)
        assert res.dtype == np.float32 and len(distinct) >= 3, f"{kind}: the FK residuals do not spread ({distinct})"
        k = int(np.nonzero(res == distinct[len(distinct) // 2])[0][0])  # a robot with a middle residual: some lie above it, some do not
        thresholds = (res[k], np.nextafter(res[k], np.float32(-np.inf)))
    else:
        k, thresholds = 0, (np.float32(0.0),)
    for j, thr in enumerate(thresholds):
        rule = pkg.DoneRule(enable=enable, max_fk_residual=float(thr))
        got = eng.evaluate_done(rule)
        assert_verdict(got, dr.done_reference(rule, **g), f"{kind}, period {period}, threshold {j}")
        if n >= 6:
            assert bool(got[1][k] & dr.FK_RESIDUAL) == (j == 1), f"{kind}: a residual equal to the threshold is not done, one value above it is"
            assert 0 < got[2][1 + 5] < B
    print(f"done, {kind}, period {period}: counts {got[2][:10].tolist()}")
    if period > 0.0:
        # Three more steps, of which the period lets at most two publish (the joint states tell which did): after a step that does not
        # publish, pose and twist have moved on while the residual and the flags are still those of the last published step.
        quiet = 0
        for _ in range(3):
            before, last = eng.joint_states(), eng.evaluate_done(rule)
            eng.update(1)
            g2 = getters(eng, cfg)
            assert_verdict(eng.evaluate_done(rule), dr.done_reference(rule, **g2), f"{kind}, period {period}, a later step")
            if all(np.array_equal(x, y) for x, y in zip(before, eng.joint_states())):
                quiet += 1
                assert not np.array_equal(g2["pose"], g["pose"])
                assert_verdict(eng.evaluate_done(rule), last, f"{kind}: a step that does not publish")
            g = g2
        assert quiet >= 1
    eng.close()


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", LAYOUTS + ["uniform_n8"])
def test_forms_and_outputs(pkg, monkeypatch, kind):
    cfg = config_of(pkg, kind, monkeypatch)
    rule, pose, twist = dr.static_scenario(pkg, cfg.model, cfg.precision == 64)
    eng = pkg.Engine(cfg, 0)
    put(eng, cfg, pose, twist)
    host = eng.evaluate_done(rule)
    canary_m, canary_r, canary_c = np.full(STRIDE, 0xA5, np.uint8), np.full(STRIDE, 0xDEADBEEF, np.uint32), np.full(2 * dr.COUNTS, 0xDEADBEEF, np.uint32)
    d_mask, d_reason, d_counts = eng.device_upload(canary_m), eng.device_upload(canary_r), eng.device_upload(canary_c)

    def download():
        return eng.device_download(d_mask, STRIDE, np.uint8), eng.device_download(d_reason, STRIDE, np.uint32), eng.device_download(d_counts, 2 * dr.COUNTS, np.uint32)

    # the device form equals the host form; entries 130 .. 191 and the words behind the counts keep their canary
    eng.evaluate_done_device(rule, d_mask, d_reason, d_counts)
    m, r, c = download()
    assert_verdict((m[:B], r[:B], c[:dr.COUNTS]), host, f"{kind}, device form")
    assert (m[B:] == 0xA5).all() and (r[B:] == 0xDEADBEEF).all() and (c[dr.COUNTS:] == 0xDEADBEEF).all(), f"{kind}: the device form wrote past row B"
    # two consecutive calls do not accumulate
    eng.evaluate_done_device(rule, d_mask, d_reason, d_counts)
    eng.evaluate_done_device(rule, d_mask, d_reason, d_counts)
    assert np.array_equal(download()[2][:dr.COUNTS], host[2]), f"{kind}: counts accumulate over calls"
    assert_verdict(eng.evaluate_done(rule), host, f"{kind}, host form again")
    # d_reason and d_counts may be NULL
    for x, v in ((d_mask, canary_m), (d_reason, canary_r), (d_counts, canary_c)):
        eng.device_upload_into(x, v)
    eng.evaluate_done_device(rule, d_mask)
    m, r, c = download()
    assert np.array_equal(m[:B], host[0]) and (m[B:] == 0xA5).all() and (r == 0xDEADBEEF).all() and (c == 0xDEADBEEF).all(), kind
    # in the host form any output may be NULL
    from cdpr_simulation_amd._native import lib

    s = rule.to_struct()
    only_counts = np.zeros(dr.COUNTS, np.uint32)
    assert lib().cdpr_evaluate_done(eng._h, C.byref(s), None, None, only_counts.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
    assert np.array_equal(only_counts, host[2])
    assert lib().cdpr_evaluate_done(eng._h, C.byref(s), None, None, None) == 0
    # an all-clear and an all-done rule
    clear = eng.evaluate_done(pkg.DoneRule())
    assert not clear[0].any() and not clear[1].any() and not clear[2].any(), kind
    everyone = pkg.DoneRule(enable=dr.TIMEOUT, max_steps=0)
    eng.evaluate_done_device(everyone, d_mask, d_reason, d_counts)
    m, r, c = download()
    assert (m[:B] == 1).all() and (r[:B] == dr.TIMEOUT).all() and c[0] == B and c[1 + 8] == B and c[1:9].sum() == 0 and (m[B:] == 0xA5).all(), kind
    assert_verdict(eng.evaluate_done(everyone), (m[:B], r[:B], c[:dr.COUNTS]), f"{kind}, all done")
    eng.synchronize()
    for x in (d_mask, d_reason, d_counts):
        eng.device_free(x)
    # (the non-finite robots leave before the handle goes: no step has run on them)
    eng.reset()
    eng.close()


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_evaluation_changes_nothing(pkg, monkeypatch, kind):
    cfg = config_of(pkg, kind, monkeypatch)
    h = ri.history_inputs(cfg.model, 401)
    rule = dr.loop_rule(pkg, cfg.model)
    eng, twin = pkg.Engine(cfg, 0), pkg.Engine(cfg, 0)
    for e in (eng, twin):
        put(e, cfg, h["pose"])
    drive([eng, twin], cfg, h, 20)
    name = eng.kernel_name
    d_mask, d_reason, d_counts = eng.device_alloc(B), eng.device_alloc(4 * B), eng.device_alloc(4 * dr.COUNTS)
    first = eng.evaluate_done(rule)
    eng.evaluate_done_device(rule, d_mask, d_reason, d_counts)
    assert eng.kernel_name == name == twin.kernel_name, f"{kind}: an evaluation changed kernel_name"
    assert first[2][0] > 0  # (the rule decides something here: 20 steps against max_steps = 15)
    for x, y in zip(prk.state_of(eng, cfg), prk.state_of(twin, cfg)):
        assert np.array_equal(x, y), f"{kind}: an evaluation changed the engine's state"
    assert not eng.episode_start().any()
    for step in range(20):
        eng.update(1), twin.update(1)
        eng.evaluate_done_device(rule, d_mask, d_reason, d_counts)
        if step % 7 == 0:
            eng.evaluate_done(rule)
    assert eng.kernel_name == twin.kernel_name and eng.step_count == twin.step_count == 40
    for x, y in zip(prk.state_of(eng, cfg), prk.state_of(twin, cfg)):
        assert np.array_equal(x, y), f"{kind}: an engine evaluated every step drifts from its twin"
    eng.synchronize()
    for x in (d_mask, d_reason, d_counts):
        eng.device_free(x)
    eng.close(), twin.close()


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", LAYOUTS)
def test_the_episode_clock(pkg, monkeypatch, kind):
    cfg = config_of(pkg, kind, monkeypatch)
    h = ri.history_inputs(cfg.model, 501)
    eng = pkg.Engine(cfg, 0)
    assert eng.episode_start().dtype == np.uint32 and not eng.episode_start().any()  # zero after create
    put(eng, cfg, h["pose"])
    drive([eng], cfg, h, ri.HISTORY)
    assert not eng.episode_start().any()
    mask = ri.reset_mask()
    m = mask.astype(bool)
    eng.reset_robots(mask, h["pose"])
    assert eng.step_count == 37
    start = eng.episode_start()
    assert (start[m] == 37).all() and not start[~m].any(), kind
    eng.update(5)  # ages: 5 for the reset robots, 42 for the others
    for max_steps, who in ((5, np.ones(B, bool)), (6, ~m), (42, ~m), (43, np.zeros(B, bool))):
        rule = pkg.DoneRule(enable=dr.TIMEOUT, max_steps=max_steps)
        got = eng.evaluate_done(rule)
        assert np.array_equal(got[0].astype(bool), who) and got[2][0] == who.sum() == got[2][1 + 8], (kind, max_steps)
        assert_verdict(got, expect(eng, cfg, rule), f"{kind}, max_steps {max_steps}")
    # the device form of the reset stamps the clock too
    d_mask = eng.device_upload((np.arange(B) == 1).astype(np.uint8))
    eng.reset_robots_device(d_mask)
    assert eng.episode_start()[1] == 42 and eng.episode_start()[2] == 0
    eng.device_free(d_mask)
    eng.reset()
    assert not eng.episode_start().any() and eng.step_count == 0  # zero again after cdpr_reset
    eng.close()


def test_the_episode_clock_of_a_uniform_handle(pkg, monkeypatch):
    cfg = config_of(pkg, "uniform_n8", monkeypatch)
    h = ri.history_inputs(cfg.model, 502)
    eng = pkg.Engine(cfg, 0)
    put(eng, cfg, h["pose"])
    drive([eng], cfg, h, 12)
    assert not eng.episode_start().any()
    for max_steps, done in ((12, B), (13, 0)):  # never refused: every robot's episode began at world step 0
        got = eng.evaluate_done(pkg.DoneRule(enable=dr.TIMEOUT, max_steps=max_steps))
        assert got[2][0] == done and got[0].sum() == done
    eng.close()


# ---- 6 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", LAYOUTS)
def test_reset_done_device_is_evaluate_then_reset(pkg, monkeypatch, kind):
    cfg = config_of(pkg, kind, monkeypatch)
    rule = dr.loop_rule(pkg, cfg.model)
    h, respawn = dr.loop_inputs(cfg.model)
    one, two = pkg.Engine(cfg, 0), pkg.Engine(cfg, 0)
    for e in (one, two):
        put(e, cfg, h["pose"])
    drive([one, two], cfg, h, 10)
    twist = np.random.default_rng(601).uniform(-0.01, 0.01, (B, 6)).astype(np.float32)
    bufs = []
    for e in (one, two):
        bufs.append((e, e.device_upload(respawn[0]), e.device_upload(twist), e.device_alloc(4 * dr.COUNTS), e.device_alloc(B)))
    (_, p1, t1, c1, _), (_, p2, t2, c2, m2) = bufs
    want = expect(one, cfg, rule)
    assert 0 < want[2][0] < B
    for rnd in range(2):  # the second round: 5 steps on, the robots the first round reset are 5 steps old
        one.reset_done_device(rule, p1, t1, c1)
        two.evaluate_done_device(rule, m2, 0, c2)
        two.reset_robots_device(m2, p2, t2)
        counts = [e.device_download(c, dr.COUNTS, np.uint32) for e, c in ((one, c1), (two, c2))]
        assert np.array_equal(counts[0], counts[1]) and (rnd > 0 or np.array_equal(counts[0], want[2])), f"{kind}, round {rnd}"
        assert np.array_equal(one.episode_start(), two.episode_start())
        if rnd == 0:
            done = want[0].astype(bool)
            assert (one.episode_start()[done] == 10).all() and not one.episode_start()[~done].any()
            p, t = one.raw_state()
            assert np.array_equal(p[done], respawn[0][done]) and np.array_equal(t[done], twist[done]), kind
        for e in (one, two):
            e.update(5)
        for x, y in zip(prk.state_of(one, cfg), prk.state_of(two, cfg)):
            assert np.array_equal(x, y), f"{kind}, round {rnd}: reset_done_device differs from evaluate_done_device + reset_robots_device"
    for e, *ptrs in bufs:
        e.synchronize()
        for x in ptrs:
            e.device_free(x)
        e.close()


# ---- 7 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", LAYOUTS)
def test_the_closed_loop_against_the_oracle(pkg, oracle, monkeypatch, kind):
    cfg = config_of(pkg, kind, monkeypatch)
    rule = dr.loop_rule(pkg, cfg.model)
    h, respawn = dr.loop_inputs(cfg.model)
    (eng,), ora = parity.sims_at(pkg, oracle, cfg, h["pose"])
    points = dr.LOOP_STEPS // dr.LOOP_EVERY
    d_pose, d_counts = eng.device_alloc(B * 7 * 4), eng.device_alloc(points * dr.COUNTS * 4)

    def check(j, mask, reason, counts, p, t):
        parity.against_the_oracle(eng, ora, cfg.precision == 64, printed="reset_robots", where=f"done rules, {kind}, evaluation point {j}")

    def reset_engine(j, poses):
        eng.device_upload_into(d_pose, poses)  # fresh poses from a device buffer (on the engine's stream, behind the reset that read it last)
        eng.reset_done_device(rule, d_pose, 0, d_counts + j * dr.COUNTS * 4)

    verdicts = dr.run_loop([eng], ora, rule, h, respawn, reset_engine, check)
    got = eng.device_download(d_counts, (points, dr.COUNTS), np.uint32)
    want = np.array([v[2] for v in verdicts])
    print(f"done rules, closed loop, {kind}: robots reset per evaluation point {got[:, 0].tolist()}")
    assert np.array_equal(got, want), f"{kind}: the engine's counts differ from the oracle side's\n{got}\n{want}"
    assert (got[:, 0] > 0).sum() >= 3
    # the episode clock after the loop: the step of every robot's last reset
    start = np.zeros(B, np.uint32)
    for j, (mask, _, _) in enumerate(verdicts):
        start[mask.astype(bool)] = (j + 1) * dr.LOOP_EVERY
    assert np.array_equal(eng.episode_start(), start)
    eng.update(1), ora.update(1)
    parity.against_the_oracle(eng, ora, cfg.precision == 64, printed="reset_robots", where=f"done rules, {kind}, one step after the last reset")
    eng.device_free(d_pose), eng.device_free(d_counts)
    eng.close(), ora.close()


# ---- 8 -------------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg, monkeypatch):
    from cdpr_simulation_amd._native import lib

    L = lib()
    INVALID, UNSUPPORTED = pkg._abi.ERR_INVALID, pkg._abi.ERR_UNSUPPORTED
    cfg = config_of(pkg, "fast_n8", monkeypatch)
    eng = pkg.Engine(cfg, 0)
    twin = pkg.Engine(cfg, 0)
    good = pkg.DoneRule(enable=dr.TIMEOUT, max_steps=0).to_struct()
    d_mask = eng.device_upload(np.full(B, 7, np.uint8))
    mask = np.full(B, 7, np.uint8)
    u8 = mask.ctypes.data_as(C.POINTER(C.c_uint8))
    # NULL rule, NULL mask (device form), a struct of another size
    assert L.cdpr_evaluate_done_device(eng._h, None, C.c_void_p(d_mask), None, None) == INVALID and b"null rule" in L.cdpr_last_error(eng._h)
    assert L.cdpr_evaluate_done(eng._h, None, u8, None, None) == INVALID and b"null rule" in L.cdpr_last_error(eng._h)
    assert L.cdpr_reset_done_device(eng._h, None, None, None, None) == INVALID and b"null rule" in L.cdpr_last_error(eng._h)
    assert L.cdpr_evaluate_done_device(eng._h, C.byref(good), None, None, None) == INVALID and b"null robot mask" in L.cdpr_last_error(eng._h)
    with pytest.raises(pkg.CdprError) as ei:
        eng.evaluate_done_device(pkg.DoneRule(), 0)
    assert ei.value.code == INVALID
    bad = pkg.DoneRule(enable=dr.TIMEOUT).to_struct()
    bad.struct_size = 52
    for call in (lambda: L.cdpr_evaluate_done_device(eng._h, C.byref(bad), C.c_void_p(d_mask), None, None), lambda: L.cdpr_evaluate_done(eng._h, C.byref(bad), u8, None, None),
                 lambda: L.cdpr_reset_done_device(eng._h, C.byref(bad), None, None, None)):
        assert call() == INVALID and b"struct_size" in L.cdpr_last_error(eng._h)
    assert L.cdpr_get_episode_start(eng._h, None) == INVALID
    # a NULL handle
    assert L.cdpr_evaluate_done_device(None, C.byref(good), C.c_void_p(d_mask), None, None) == INVALID
    assert L.cdpr_evaluate_done(None, C.byref(good), u8, None, None) == INVALID
    assert L.cdpr_reset_done_device(None, C.byref(good), None, None, None) == INVALID
    # nothing was queued or written by a refused call
    assert (mask == 7).all() and (eng.device_download(d_mask, B, np.uint8) == 7).all() and not eng.episode_start().any()
    for x, y in zip(prk.state_of(eng, cfg), prk.state_of(twin, cfg)):
        assert np.array_equal(x, y)
    eng.device_free(d_mask)
    eng.close(), twin.close()
    # FK_RESIDUAL without CDPR_STAGE_FK, INFEASIBLE without CDPR_STAGE_TD
    for stages, bit, word in ((2, dr.FK_RESIDUAL, "CDPR_STAGE_FK"), (1, dr.INFEASIBLE, "CDPR_STAGE_TD"), (0, dr.FK_RESIDUAL | dr.INFEASIBLE, "CDPR_STAGE_FK")):
        eng = pkg.Engine(pkg.Config(model=ri.model_of(pkg, 8), batch=B, stages=stages), 0)
        d_mask = eng.device_alloc(B)
        for call in (lambda: eng.evaluate_done(pkg.DoneRule(enable=bit)), lambda: eng.evaluate_done_device(pkg.DoneRule(enable=bit), d_mask),
                     lambda: eng.reset_done_device(pkg.DoneRule(enable=bit))):
            with pytest.raises(pkg.CdprError) as ei:
                call()
            assert ei.value.code == UNSUPPORTED and word in str(ei.value), (stages, str(ei.value))
        ok = dr.TRAVEL | (dr.INFEASIBLE if stages & 2 else 0) | (dr.FK_RESIDUAL if stages & 1 else 0)  # what the handle has may be asked for
        assert not eng.evaluate_done(pkg.DoneRule(enable=ok, max_fk_residual=1.0))[0].any()
        eng.device_free(d_mask)
        eng.close()
    # cdpr_reset_done_device on a uniform handle
    cfg = config_of(pkg, "uniform_n8", monkeypatch)
    eng = pkg.Engine(cfg, 0)
    with pytest.raises(pkg.CdprError) as ei:
        eng.reset_done_device(pkg.DoneRule(enable=dr.TIMEOUT, max_steps=0))
    assert ei.value.code == UNSUPPORTED and "per_robot_commands" in str(ei.value)
    assert eng.evaluate_done(pkg.DoneRule(enable=dr.TIMEOUT, max_steps=0))[2][0] == B  # ... which evaluates all the same
    p, _ = eng.raw_state()
    assert np.array_equal(p, np.tile(np.asarray(cfg.model.home_pose(), dtype=np.float32), (B, 1)))
    eng.close()


# ---- 9 -------------------------------------------------------------------------------------------------------------------------
def test_sharded(pkg, monkeypatch):
    cfg = config_of(pkg, "fast_n8", monkeypatch)
    rule, pose, twist = dr.static_scenario(pkg, cfg.model, False)
    one = pkg.Engine(cfg, 0)
    sh = pkg.ShardedEngine(cfg, devices=[0, 0, 0])
    one.set_platform_state(pose, twist), sh.set_platform_state(pose, twist)
    want, got = one.evaluate_done(rule), sh.evaluate_done(rule)
    assert_verdict(got, want, "three shards on one device")
    assert got[2][0] == want[0].sum() and [hi - lo for lo, hi in sh.spans] == [44, 43, 43]
    # per-shard reset: home pose, zero twist; counts into one buffer per shard
    d_counts = [e.device_alloc(4 * dr.COUNTS) for e in sh.engines]
    sh.reset_done_device(rule, d_counts=d_counts)
    one.reset_done_device(rule)
    summed = np.sum([e.device_download(d, dr.COUNTS, np.uint32) for e, d in zip(sh.engines, d_counts)], axis=0, dtype=np.uint32)
    assert np.array_equal(summed, want[2])
    for x, y in zip(sh.raw_state(), one.raw_state()):
        assert np.array_equal(x, y)
    assert not sh.episode_start().any() and np.isfinite(sh.raw_state()[0]).all()  # (world step 0: the clock reads 0 either way)
    assert_verdict(sh.evaluate_done(rule), one.evaluate_done(rule), "three shards, after the reset")
    assert not sh.evaluate_done(rule)[0].any()
    for e, d in zip(sh.engines, d_counts):
        e.device_free(d)
    sh.close(), one.close()
