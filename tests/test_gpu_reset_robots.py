"""cdpr_reset_robots / cdpr_reset_robots_device: chosen robots of a per-robot handle go back to the state Load leaves, at a pose of the
caller's, while the others run on - on every record layout (register-resident per-robot records, the general path's record buffer
with its hot rows, the precision = 64 rows), against the fp64 oracle at the tolerances of tests/parity.py (TOL, TOL64).  On the oracle
a reset is the recipe of tests/robot_histories.py (oracle_reset), whose history independence tests/test_reset_robots_inputs.py
establishes on the oracle alone.

  1  against the oracle on every handle kind: robots in Position / Velocity / Force mode by index mod 3, 37 steps, every fourth robot
     plus 0, 63, 64, 129 reset to fresh poses; compared 1 and 7 steps later, 30 steps after a masked velocity Joy whose even cables
     sit below epsilon, 25 steps after a masked position Joy.
  2  the others are untouched: a twin engine runs the same sequence without the reset; raw_state, joint_states and observables of the
     robots outside the mask are equal to the bit at every checkpoint.
  3  read-out before any update.  4  host form = device form, pose7 None = home, the all-zero and the all-ones mask.
  5  a command pending at the reset survives it.  6  a reset through the device form in front of every step.  7  refusals.
  8  the engine against itself: a second engine driven by the recipe (raw_state, set_platform_state, masked velocity 0, masked
     position 0) instead of the call.

B = 130: two full wavefronts and a ragged one, stride 192.
"""
import ctypes as C

import numpy as np
import pytest

import parity
import robot_histories as ri
from parity import TOL, TOL64, perturbed_poses, sims_at
from per_robot_kinds import ALL, LAYOUTS, clean_env, config_of, named, state_of  # noqa: F401  (clean_env: autouse here too)

pytestmark = pytest.mark.gpu

B = ri.B
BIT_EQUAL = ("fast_n8", "fast_n4", "fast_n7", "fp64_n8")   # one Pid record per robot: the recipe and the call zero it the same way


def against_the_oracle(eng, ora, cfg, where):
    parity.against_the_oracle(eng, ora, cfg.precision == 64, where, printed="reset_robots")


# ---- 1, 2 ----------------------------------------------------------------------------------------------------------------------
def run_scenario(pkg, oracle, monkeypatch, kind, twin):
    cfg = config_of(pkg, kind, monkeypatch)
    model = cfg.model
    h, a = ri.history_inputs(model, 31), ri.after_inputs(model, 32)
    mask = ri.reset_mask()
    engs, ora = sims_at(pkg, oracle, cfg, h["pose"], 2 if twin else 1)
    eng = engs[0]
    ri.play_history(engs + [ora], h)
    named(eng, kind)
    eng.reset_robots(mask, a["pose"])
    ri.oracle_reset(ora, mask, a["pose"])
    others = ~mask.astype(bool)

    def check(label, with_oracle=True):
        if with_oracle:
            against_the_oracle(eng, ora, cfg, f"{kind}, {label}")
        if twin:
            for x, y in zip(state_of(eng, cfg), state_of(engs[1], cfg)):
                assert np.array_equal(x[others], y[others]), f"{kind}, {label}: the reset changed a robot outside the mask"

    if twin:
        check("right after the reset", with_oracle=False)  # (the oracle takes the recipe in at its next update)
    ri.play_after(engs + [ora], a, check)
    named(eng, kind)
    for e in engs + [ora]:
        e.close()


@pytest.mark.parametrize("kind", ALL)
def test_reset_against_the_oracle(pkg, oracle, monkeypatch, kind):
    run_scenario(pkg, oracle, monkeypatch, kind, twin=False)


@pytest.mark.parametrize("kind", LAYOUTS)
def test_the_other_robots_are_untouched(pkg, oracle, monkeypatch, kind):
    run_scenario(pkg, oracle, monkeypatch, kind, twin=True)


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", LAYOUTS)
def test_read_out_before_any_update(pkg, oracle, monkeypatch, kind):
    cfg = config_of(pkg, kind, monkeypatch)
    f64 = cfg.precision == 64
    h, a = ri.history_inputs(cfg.model, 41), ri.after_inputs(cfg.model, 42)
    mask = ri.reset_mask()
    m = mask.astype(bool)
    (eng,), ora = sims_at(pkg, oracle, cfg, h["pose"])
    ri.play_history([eng], h)
    before = state_of(eng, cfg) + eng.fk_state() + (eng.limit_state(),) + eng.td_state()
    steps = eng.step_count
    twist = np.random.default_rng(43).uniform(-0.01, 0.01, (B, 6)).astype(np.float32)
    eng.reset_robots(mask, a["pose"], twist)
    after = state_of(eng, cfg) + eng.fk_state() + (eng.limit_state(),) + eng.td_state()
    assert eng.step_count == steps  # a model reset, not a world reset
    for x, y in zip(before, after):
        assert np.array_equal(x[~m], y[~m]), f"{kind}: a robot outside the mask reads differently"
    want = a["pose"].astype(np.float64) if f64 else a["pose"]
    raw_p, raw_t = after[0], after[1]
    assert np.array_equal(raw_p[m], want[m]) and np.array_equal(raw_t[m], twist.astype(raw_t.dtype)[m]), kind
    q, qd, eff, pose, tw = eng.observables_f64() if f64 else eng.observables()
    assert pose.dtype == (np.float64 if f64 else np.float32)
    assert np.array_equal(pose[m], want[m]), kind
    for name, x in (("twist", tw), ("q", q), ("qd", qd), ("effort", eff)):
        assert not x[m].any(), f"{kind}: {name} of a reset robot is not zero before its first publish"
    fk_pose, fk_res, fk_it = eng.fk_state()
    assert np.array_equal(fk_pose[m], a["pose"][m]) and not fk_res[m].any() and not fk_it[m].any(), kind
    assert not eng.limit_state()[m].any() and not eng.td_state()[1][m].any() and not eng.td_state()[0][m].any(), kind
    eng.close(), ora.close()


def test_read_out_of_the_pid_topic(pkg, oracle, monkeypatch):
    """the `pid` debug row of a reset robot is zero, the others' rows stay (fp32 and precision = 64)"""
    for precision in (32, 64):
        cfg = pkg.Config(model=ri.model_of(pkg, 8), batch=B, stages=3 | pkg._abi.STAGE_PID_DEBUG, perRobotCommands=True, precision=precision)
        h = ri.history_inputs(cfg.model, 44)
        (eng,), ora = sims_at(pkg, oracle, cfg, h["pose"])
        ri.play_history([eng], h, 15)
        m = ri.reset_mask().astype(bool)
        before = eng.pid_debug()
        assert before[~m].any()
        eng.reset_robots(m)
        after = eng.pid_debug()
        assert not after[m].any() and np.array_equal(after[~m], before[~m]), precision
        eng.close(), ora.close()


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", LAYOUTS)
def test_forms_and_defaults(pkg, oracle, monkeypatch, kind):
    cfg = config_of(pkg, kind, monkeypatch)
    h, a = ri.history_inputs(cfg.model, 51), ri.after_inputs(cfg.model, 52)
    rng = np.random.default_rng(53)
    mask = ri.reset_mask()
    twist = rng.uniform(-0.01, 0.01, (B, 6)).astype(np.float32)
    (host, dev, twin, every), ora = sims_at(pkg, oracle, cfg, h["pose"], 4)
    ri.play_history([host, dev, twin, every, ora], h)
    # host form = device form, with a twist
    host.reset_robots(mask, a["pose"], twist)
    bufs = [dev.device_upload(x) for x in (mask, a["pose"], twist)]
    dev.reset_robots_device(*bufs)
    for e in (host, dev):
        e.update(3)
    for x, y in zip(state_of(host, cfg), state_of(dev, cfg)):
        assert np.array_equal(x, y), f"{kind}: the device form differs from the host form"
    # pose7 None = home_pose (host form, then device form with null pointers)
    m = mask.astype(bool)
    host.reset_robots(mask)
    dev.reset_robots_device(bufs[0])
    home = np.asarray(cfg.model.home_pose(), dtype=np.float32)
    for e in (host, dev):
        p, t = e.raw_state()
        assert np.array_equal(p[m], np.tile(home, (int(m.sum()), 1))) and not t[m].any(), kind
    for x, y in zip(state_of(host, cfg), state_of(dev, cfg)):
        assert np.array_equal(x, y), kind
    dev.synchronize()
    for b in bufs:
        dev.device_free(b)
    # an all-zero mask changes nothing
    every.reset_robots(np.zeros(B, np.uint8), a["pose"], twist)
    every.update(4), twin.update(4)
    for x, y in zip(state_of(every, cfg), state_of(twin, cfg)):
        assert np.array_equal(x, y), f"{kind}: an all-zero mask changed something"
    # an all-ones mask is the recipe on every robot
    ora.update(4)
    every.reset_robots(np.ones(B, np.uint8), a["pose"], twist)
    ri.oracle_reset(ora, np.ones(B, np.uint8), a["pose"], twist)
    every.update(1), ora.update(1)
    against_the_oracle(every, ora, cfg, f"{kind}, all-ones mask, 1 step")
    every.update(12), ora.update(12)
    against_the_oracle(every, ora, cfg, f"{kind}, all-ones mask, 13 steps")
    for e in (host, dev, twin, every, ora):
        e.close()


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fast_n8", "general_n8", "fp64_n8"])
def test_a_pending_command_survives_the_reset(pkg, oracle, monkeypatch, kind):
    """A masked force command sent BEFORE the reset, to robots the reset takes and to others: it is latched at the next update onto the
    reset robots, as a Joy sent right after Load - the latch order velocity, position, force leaves them in Force mode with fresh Pids."""
    cfg = config_of(pkg, kind, monkeypatch)
    h, a = ri.history_inputs(cfg.model, 61), ri.after_inputs(cfg.model, 62)
    mask = ri.reset_mask()
    (eng,), ora = sims_at(pkg, oracle, cfg, h["pose"])
    ri.play_history([eng, ora], h)
    f = ri.forces(cfg.n_cables, np.random.default_rng(63))
    f_mask = (np.arange(B) % 8 < 3).astype(np.uint8)  # robots 0, 8, 16 ... are reset AND addressed; 1, 2, 9 ... only addressed
    assert eng.set_force_command(f, mask=f_mask) == 0 and ora.set_force_command(f, mask=f_mask) == 0
    eng.reset_robots(mask, a["pose"])
    ri.oracle_reset(ora, mask, a["pose"])
    eng.update(1), ora.update(1)
    against_the_oracle(eng, ora, cfg, f"{kind}, pending force command, 1 step")
    eng.update(20), ora.update(20)
    against_the_oracle(eng, ora, cfg, f"{kind}, pending force command, 21 steps")
    for s in (eng, ora):  # ... and from Force mode into a Pid that the reset left fresh
        assert s.set_velocity_command(a["v"], mask=a["v_mask"]) == 0
        s.update(30)
    against_the_oracle(eng, ora, cfg, f"{kind}, velocity Joy after the pending force command")
    eng.close(), ora.close()


# ---- 6 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fast_n8", "general_n8"])
def test_a_reset_in_front_of_every_step(pkg, oracle, monkeypatch, kind):
    """The loop this is for: 40 steps, each behind a device-form reset of a fresh random 5 % of the robots; twice in between an
    update(10), so that the graph-chained launches of the small batch are crossed."""
    cfg = config_of(pkg, kind, monkeypatch)
    h = ri.history_inputs(cfg.model, 71)
    rng = np.random.default_rng(72)
    (eng,), ora = sims_at(pkg, oracle, cfg, h["pose"])
    ri.play_history([eng, ora], h)
    d_mask, d_pose = eng.device_alloc(B), eng.device_alloc(B * 7 * 4)
    for step in range(40):
        mask = (rng.random(B) < 0.05).astype(np.uint8)
        pose = perturbed_poses(cfg.model, B, rng, 0.02, 0.05).astype(np.float32)
        eng.device_upload_into(d_mask, mask)  # (on the engine's stream, behind the reset that read the buffers last)
        eng.device_upload_into(d_pose, pose)
        eng.reset_robots_device(d_mask, d_pose)
        ri.oracle_reset(ora, mask, pose)
        eng.update(1), ora.update(1)
        if step in (12, 30):
            eng.update(10), ora.update(10)
        if step == 19:
            against_the_oracle(eng, ora, cfg, f"{kind}, a reset before every step, step 20")
    against_the_oracle(eng, ora, cfg, f"{kind}, a reset before every step, the end")
    eng.synchronize()
    eng.device_free(d_mask), eng.device_free(d_pose)
    eng.close(), ora.close()


# ---- 7 -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_it_was(pkg, oracle, monkeypatch):
    from cdpr_simulation_amd._native import lib

    # a uniform handle: one mode and one Pid call count for the whole batch
    cfg = config_of(pkg, "fast_n8", monkeypatch, per_robot=False)
    h = ri.history_inputs(cfg.model, 81)
    (eng,), ora = sims_at(pkg, oracle, cfg, h["pose"])
    for s in (eng, ora):
        s.set_velocity_command(h["v"])
        s.update(20)
    d = eng.device_upload(np.ones(B, np.uint8))
    for call in (lambda: eng.reset_robots(np.ones(B, np.uint8)), lambda: eng.reset_robots_device(d)):
        with pytest.raises(pkg.CdprError) as ei:
            call()
        assert ei.value.code == pkg._abi.ERR_UNSUPPORTED and "per_robot_commands" in str(ei.value)
    eng.device_free(d)
    eng.update(5), ora.update(5)
    against_the_oracle(eng, ora, cfg, "uniform handle after the refused calls")
    eng.close(), ora.close()
    # a null mask, a null handle
    cfg = config_of(pkg, "fast_n8", monkeypatch)
    (eng,), ora = sims_at(pkg, oracle, cfg, h["pose"])
    ri.play_history([eng, ora], h, 20)
    assert lib().cdpr_reset_robots(eng._h, None, None, None) == pkg._abi.ERR_INVALID
    assert lib().cdpr_reset_robots_device(eng._h, None, None, None) == pkg._abi.ERR_INVALID
    with pytest.raises(pkg.CdprError) as ei:
        eng.reset_robots_device(0)
    assert ei.value.code == pkg._abi.ERR_INVALID
    assert lib().cdpr_reset_robots(None, np.ones(B, np.uint8).ctypes.data_as(C.POINTER(C.c_uint8)), None, None) == pkg._abi.ERR_INVALID
    assert lib().cdpr_reset_robots_device(None, None, None, None) == pkg._abi.ERR_INVALID
    eng.update(5), ora.update(5)
    against_the_oracle(eng, ora, cfg, "per-robot handle after the refused calls")
    eng.close(), ora.close()


# ---- 8 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ALL)
def test_the_engine_against_itself(pkg, oracle, monkeypatch, kind):
    """A second engine driven by the recipe instead of the call.  One Pid record per robot (register-resident, precision = 64 without the
    hold branch): the same bits on the reset robots after the first update.  Two records per cable (general path, HOLD): at TOL / TOL64
    - the recipe leaves a velocity Pid that was in use, and mLastPosition, to be overwritten later - and the test prints whether the
    bits were equal too.  The robots OUTSIDE the mask are compared at TOL / TOL64 on every handle: cdpr_set_platform_state has no mask
    and moves the FK seed of every robot it is given a pose for onto that pose, so the recipe (not the call) restarts their estimator,
    and with FK + TD the tension distribution at the estimate moves their efforts by rounding."""
    cfg = config_of(pkg, kind, monkeypatch)
    f64 = cfg.precision == 64
    h, a = ri.history_inputs(cfg.model, 91), ri.after_inputs(cfg.model, 92)
    mask = ri.reset_mask()
    m = mask.astype(bool)
    (eng, rec), ora = sims_at(pkg, oracle, cfg, h["pose"], 2)
    ri.play_history([eng, rec], h)
    eng.reset_robots(mask, a["pose"])
    if f64:
        p, t = rec.raw_state_f64()
        p[m], t[m] = a["pose"].astype(np.float64)[m], 0.0
        rec.set_platform_state_f64(p, t)
    else:
        p, t = rec.raw_state()
        p[m], t[m] = a["pose"][m], 0.0
        rec.set_platform_state(p, t)
    zero = np.zeros(cfg.n_cables, np.float32)
    assert rec.set_velocity_command(zero, mask=mask) == 0 and rec.set_position_command(zero, mask=mask) == 0
    tol = TOL64 if f64 else TOL
    equal = []

    def check(label):
        sa, sb = state_of(eng, cfg), state_of(rec, cfg)
        same = all(np.array_equal(x[m], y[m]) for x, y in zip(sa, sb))
        equal.append((same, all(np.array_equal(x[~m], y[~m]) for x, y in zip(sa, sb))))
        if kind in BIT_EQUAL:
            assert same, f"{kind}, {label}: the call and the recipe leave different bits on the reset robots"
        xs, ys = ((e.observables_f64() if f64 else e.observables()) for e in (eng, rec))
        for name, x, y in zip(("q", "qd", "eff", "pose", "twist"), xs, ys):
            assert np.abs(x - y).max() <= tol[name], f"{kind}, {label}: {name} differs between the call and the recipe by {np.abs(x - y).max():.3e}"

    ri.play_after([eng, rec], a, check)
    print(f"reset_robots, {kind}: the call and the recipe gave the same bits at the checkpoints (reset robots, the others): {equal}")
    for e in (eng, rec, ora):
        e.close()
