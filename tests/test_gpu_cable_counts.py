"""Every cable count the engine accepts (1 .. 12, cdpr_select.hpp validate_config) against the fp64 oracle.

Models are subsets of twelve_cable_model (as test_gpu_more_cables.py).  Robots with one to three cables are under-constrained and
swing (twist up to 0.7 at n = 1); the oracle stays bounded over the 110-step script below, and a 3e-8 m perturbation of the spawn
pose stays below 1e-7 in every observable there, so the fp32 tolerances (TOL) and the fp64 ones (TOL64) of tests/parity.py
hold unchanged at every count.  Measured on MI355X over this module (test_zz_report_measured_agreement
prints them with -s), worst over n = 1 .. 12: fp32 pose 4.3e-7, twist 2.0e-5, q 4.8e-7, qd 2.3e-5, effort 3.9e-3, pid topic 4.1e-4,
rollout cost 6.6e-5 relative; fp64 pose 1.0e-15, twist 5.3e-14, q 1.0e-15, qd 4.8e-14, effort 9.4e-12, rollout cost 5.3e-8 relative.

  a. the cable-count matrix: n x handle kind {uniform, per-robot, general (hold branch live), precision = 64} x every mapping the
     plan serves x stages {0, FK + TD from six cables on, FK only at 9, TD only at 6}: oracle parity after every segment of a
     spawn / zero-command / velocity / position / force / velocity script, one-step = fused = recorded = scheduled launches bit for
     bit, the kernel each launch form ran on (cdpr_kernel_name) = the planned one (cdpr_plan_kernel), the MPC rollout included;
  b. every read-out path agrees at every n: cdpr_get_observables in its three tiers (direct, pinned staging, caller arrays) =
     the separate getters bit for bit, with decimation, NULL outputs and repeated calls; the trajectory record's last image;
     on precision = 64 handles the float getters = observables_f64 cast to float32;
  c. the options accepted at nine to twelve cables (force mode, travel-limit flags of cables 9-12, the pid topic, publish
     decimation, velocity limit, unilateral cables, effort clamp) in fp32 and fp64 against the oracle;
  d. the drop-in facade at 10 and 12 cables, per world step (cdpr_get_observables) and 25 steps per call (the record)."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest

import parity
from parity import TOL, perturbed_poses, state_of
from parity import sliced_twelve as model_of

pytestmark = pytest.mark.gpu

FIRST, SCHEDULED, ROLLOUT, NOT_STEADY = 1, 2, 4, 8  # CDPR_PLAN_* (include/cdpr.h)
WORST = {}


def note(n, name, err):
    WORST[(n, name)] = max(WORST.get((n, name), 0.0), float(err))


def against_oracle(eng, ora, n, f64, where):
    """parity.against_the_oracle, the worst errors noted under the cable count"""
    for name, (err, _, _) in parity.against_the_oracle(eng, ora, f64, where).items():
        note(n, name + ("64" if f64 else ""), err)


# ---- a. the cable-count matrix ----------------------------------------------------------------------------------------------
def matrix_cells():
    cells = []
    for n in range(1, 13):
        for handle in ("uniform", "per_robot", "general", "fp64"):
            if n > 8 and handle in ("per_robot", "general"):
                continue  # (refused by name above eight cables: test_gpu_more_cables.py)
            maps = ["robot"]
            if handle == "uniform":
                maps += ["pair"] if n in (4, 8) else []
                maps += ["cable"] if n <= 8 else []
            for mapping in maps:
                for stages in ((0, 3) if n >= 6 else (0,)):
                    cells.append((n, handle, mapping, stages))
    cells += [(9, "uniform", "robot", 1), (6, "uniform", "robot", 2)]  # FK only, TD only
    return cells


def config_of(pkg, n, handle, mapping, stages, batch, **kw):
    kw.update(model=kw.pop("model", None) or model_of(pkg, n), batch=batch, stages=stages,
              mapping={"robot": pkg._abi.MAP_LANE_PER_ROBOT, "pair": pkg._abi.MAP_LANE_PAIR, "cable": pkg._abi.MAP_LANE_PER_CABLE}[mapping])
    if handle == "per_robot":
        kw["perRobotCommands"] = True
    elif handle == "general":
        kw["velocityEpsilon"] = 0.001
    elif handle == "fp64":
        kw["precision"] = 64
    return pkg.Config(**kw)


@pytest.mark.parametrize("n,handle,mapping,stages", matrix_cells(), ids=lambda v: str(v))
def test_cable_count_matrix(pkg, oracle, n, handle, mapping, stages):
    B, f64 = 70, handle == "fp64"
    rng = np.random.default_rng(7000 + 100 * n + stages)
    cfg = config_of(pkg, n, handle, mapping, stages, B)
    pkg.plan_kernel(cfg, 1)  # (raises where the plan refuses the cell)
    pose = perturbed_poses(cfg.model, B, rng, dp=0.02, dr=0.05).astype(np.float32)
    v, v2 = (rng.uniform(-0.03, 0.03, (B, n)).astype(np.float32) for _ in range(2))
    p = rng.uniform(-0.004, 0.004, (B, n)).astype(np.float32)
    f = rng.uniform(2.0, 6.0, (B, n)).astype(np.float32)
    script = (("hold", 5, None), ("velocity", 30, v), ("position", 30, p), ("force", 20, f), ("velocity", 25, v2))
    # a: one step per launch; b: fused (10 per launch); c: the trajectory record; d: each segment a schedule queued with one call
    engs = [pkg.Engine(cfg, 0) for _ in range(4)]
    a, b, c, d = engs
    ora = oracle.OracleSim(cfg.to_struct(), oracle.DERIV_EXACT)
    for e in engs:
        e.set_platform_state_f64(pose7=pose.astype(np.float64)) if f64 else e.set_platform_state(pose7=pose)
    ora.set_platform_state(pose7=pose.astype(np.float64))
    want_mapping = {"robot": "lane-per-robot", "pair": "lane-pair", "cable": "lane-per-cable"}[mapping]
    assert a.mapping == want_mapping
    setter = {"velocity": "set_velocity_command", "position": "set_position_command", "force": "set_force_command"}
    for kind, k, cmd in script:
        where = f"n = {n}, {handle}, {mapping}, stages {stages}, {kind}"
        if cmd is not None:
            for sim in (a, b, c, ora):
                getattr(sim, setter[kind])(cmd)
        a.update(k)
        b.update(k, 10)
        rec = c.update_record(k, 10)
        dptr = 0
        if cmd is None:
            d.update(k, k)
        else:
            dptr = d.device_upload(cmd[None])
            d.update_scheduled(k, k, dptr, kind=kind)
        ora.update(k)
        against_oracle(a, ora, n, f64, where)
        sa = state_of(a, f64)
        for e, form in ((b, "fused"), (c, "recorded"), (d, "scheduled")):
            for x, y in zip(sa, state_of(e, f64)):
                assert np.array_equal(x, y), f"{where}: {form} launches differ from one-step launches"
        for j, key in enumerate(("position", "velocity", "effort", "pose", "twist")):
            assert np.array_equal(rec[key][-1], sa[2 + j]), f"{where}: the record's last step is not the published one ({key})"
        if dptr:
            d.device_free(dptr)
        # what ran = what was planned, for every launch form
        # (a segment's last fused launch starts with a full window except in Force mode; the first one starts at world step 0)
        flags = (FIRST | NOT_STEADY) if kind == "hold" else NOT_STEADY if kind == "force" else 0
        last = k - 10 * ((k - 1) // 10)
        assert a.kernel_name == pkg.plan_kernel(cfg, 1), where
        assert b.kernel_name == pkg.plan_kernel(cfg, last, flags) == c.kernel_name, where
        if cmd is not None:
            assert d.kernel_name == pkg.plan_kernel(cfg, k, SCHEDULED | NOT_STEADY), where
    if stages & 1:
        gp, gr, gi = a.fk_state()
        op, orr, oi = ora.fk_state()
        assert np.abs(gp - op).max() < 1e-5 and np.array_equal(gi, oi) and gr.max() < 1e-5
    if stages & 2:
        gt, gf = a.td_state()
        ot, of = ora.td_state()
        assert np.abs(gt - ot).max() < TOL["eff"] and np.array_equal(gf, of)
    # the MPC rollout from the state the script left (the engine's own state stays untouched)
    S, H = 4, 10
    cmds = (rng.uniform(-0.03, 0.03, (B, H, 1, n)) + rng.normal(0.0, 0.01, (B, H, S, n))).astype(np.float32)
    ref = pose[:, :3].copy()
    before = state_of(a, f64)
    cost = a.rollout_velocity(cmds, ref)
    assert a.kernel_name == pkg.plan_kernel(cfg, H, ROLLOUT), f"n = {n}, {handle}: rollout"
    for x, y in zip(before, state_of(a, f64)):
        assert np.array_equal(x, y)
    assert np.isfinite(cost).all()
    if n in (1, 3, 5, 9, 12):
        ocost = ora.rollout_velocity(cmds, ref.astype(np.float64))
        rel = float(np.abs(cost - ocost).max() / np.abs(ocost).max())
        note(n, "rollout64" if f64 else "rollout", rel)
        assert rel <= (3e-7 if f64 else 2e-4), f"n = {n}, {handle}: rollout cost differs by {rel:.3e} (relative)"
    for e in engs:
        e.close()


# ---- b. every read-out path agrees -------------------------------------------------------------------------------------------
def tier_batches(n):
    """The batch at each tier boundary of cdpr_get_observables and one robot past it (rows of 4 (3 n + 13) bytes)."""
    row = 4 * (3 * n + 13)
    b1, b2 = (256 << 10) // row, (2 << 20) // row
    return (1, b1, b1 + 1, b2, b2 + 1)


def getters(eng):
    q, qd, e = eng.joint_states()
    p, t = eng.platform_state()
    return q, qd, e, p, t


@pytest.mark.parametrize("n", range(1, 13))
def test_observables_equal_the_separate_getters_in_every_tier(pkg, n):
    """cdpr_get_observables (3 n + 13 columns in one gather) = cdpr_get_joint_states + cdpr_get_platform_state bit for bit, in
    the direct tier (<= 256 KiB), the pinned staging tier (<= 2 MiB) and the caller-array tier, at and one robot past each
    boundary, call after call (the completion word's epoch), with NULL outputs and under publish decimation."""
    from cdpr_simulation_amd._native import lib

    fp = C.POINTER(C.c_float)
    null = fp()
    for batch in tier_batches(n):
        for period in (0.0, 0.0025):
            cfg = pkg.Config(model=model_of(pkg, n), batch=batch, stages=3 if n >= 6 else 0, publishPeriod=period)
            eng = pkg.Engine(cfg, 0)
            rng = np.random.default_rng(n * 100000 + batch)
            eng.set_platform_state(pose7=perturbed_poses(cfg.model, batch, rng, dp=0.02, dr=0.05).astype(np.float32))
            eng.set_velocity_command(rng.uniform(-0.03, 0.03, (batch, n)).astype(np.float32))
            for rounds in range(3):
                eng.update(3 + rounds)
                want = getters(eng)
                for _ in range(2):
                    got = eng.observables()
                    for name, x, y in zip(("q", "qd", "effort", "pose", "twist"), want, got):
                        assert x.shape == y.shape and np.array_equal(x, y), f"n = {n}, batch {batch}, period {period}: {name}"
            only = [np.full_like(want[3], np.nan), np.full_like(want[1], np.nan)]
            assert lib().cdpr_get_observables(eng._h, null, only[1].ctypes.data_as(fp), null, only[0].ctypes.data_as(fp), null) == 0
            assert np.array_equal(only[0], want[3]) and np.array_equal(only[1], want[1])
            eng.close()


@pytest.mark.parametrize("n", range(1, 13))
def test_record_image_and_double_read_outs_agree(pkg, oracle, n):
    """The last step of update_record = decode_observables of its image = observables(); on a precision = 64 handle the float
    getters are observables_f64 cast to float32, and all five double arrays match the oracle (velocity and twist included)."""
    B = 67
    rng = np.random.default_rng(4000 + n)
    stages = 3 if n >= 6 else 0
    cfg = pkg.Config(model=model_of(pkg, n), batch=B, stages=stages)
    pose = perturbed_poses(cfg.model, B, rng, dp=0.02, dr=0.05).astype(np.float32)
    v = rng.uniform(-0.03, 0.03, (B, n)).astype(np.float32)
    eng = pkg.Engine(cfg, 0)
    eng.set_platform_state(pose7=pose)
    eng.update(4)
    eng.set_velocity_command(v)
    image = eng.observable_image_bytes()
    steps = 12
    dptr = eng.device_alloc(image * steps)
    eng.update_record_device(steps, 5, dptr, image * steps)
    raw = eng.device_download(dptr, (steps, image), dtype=np.uint8)
    eng.device_free(dptr)
    from_image = eng.decode_observables(raw[-1])
    obs = eng.observables()
    for x, y in zip(from_image, obs):
        assert np.array_equal(x, y)
    eng.close()
    cfg64 = replace(cfg, precision=64)
    e64, ora = pkg.Engine(cfg64, 0), oracle.OracleSim(cfg64.to_struct(), oracle.DERIV_EXACT)
    e64.set_platform_state_f64(pose7=pose.astype(np.float64)), ora.set_platform_state(pose7=pose.astype(np.float64))
    e64.update(4), ora.update(4)
    e64.set_velocity_command(v), ora.set_velocity_command(v)
    rec = e64.update_record(steps, 5)
    ora.update(steps)
    d = e64.observables_f64()
    against_oracle(e64, ora, n, True, f"n = {n}, precision = 64")
    for j, key in enumerate(("position", "velocity", "effort", "pose", "twist")):
        assert np.array_equal(rec[key][-1], d[j])
    as32 = [x.astype(np.float32) for x in d]
    for x, y in zip(as32, e64.observables()):
        assert np.array_equal(x, y)
    for x, y in zip(as32, getters(e64)):
        assert np.array_equal(x, y)
    if stages:
        gp, gr, gi = e64.fk_state()
        op, orr, oi = ora.fk_state()
        assert np.abs(gp - op).max() < 1e-5 and np.array_equal(gi, oi)
        gt, gf = e64.td_state()
        ot, of = ora.td_state()
        assert np.abs(gt - ot).max() < 1e-5 and np.array_equal(gf, of)  # (tensions to 100 N, read out as float32)
    e64.close()


# ---- c. options accepted at nine to twelve cables ---------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("n,stages", [(9, 0), (10, 3), (11, 0), (12, 3)])
def test_options_above_eight_cables(pkg, oracle, n, stages, precision):
    """Travel limits that cables 8-11 cross (their limit bits against oracle.limit_state), the pid topic, publish decimation,
    velocity limit, unilateral cables, the effort clamp, and force mode with commands beyond the clamp."""
    B, f64 = 60, precision == 64
    rng = np.random.default_rng(9900 + 10 * n + stages)
    model = replace(model_of(pkg, n), travel_lower=-0.003, travel_upper=0.003, velocity_limit=0.04, unilateral_cables=True, effort_limit=30.0)
    cfg = pkg.Config(model=model, batch=B, stages=stages | pkg._abi.STAGE_PID_DEBUG, precision=precision, publishPeriod=0.0025)
    assert pkg.plan_kernel(cfg, 1).startswith(f"cdpr_step_kernel_f64<{n}" if f64 else f"cdpr_step_kernel<{n}, ")
    pose = perturbed_poses(model, B, rng, dp=0.01, dr=0.03).astype(np.float32)
    eng, ora = pkg.Engine(cfg, 0), oracle.OracleSim(cfg.to_struct(), oracle.DERIV_EXACT)
    eng.set_platform_state_f64(pose7=pose.astype(np.float64)) if f64 else eng.set_platform_state(pose7=pose)
    ora.set_platform_state(pose7=pose.astype(np.float64))
    v = rng.uniform(-0.01, 0.01, (B, n)).astype(np.float32)
    v[:, 8:] = rng.choice([-0.06, 0.06], (B, n - 8))  # cables 8 .. n-1 run past the travel limits
    where = f"n = {n}, stages {stages}, precision {precision}"
    eng.update(9), ora.update(9)
    eng.set_velocity_command(v), ora.set_velocity_command(v)
    limit_bits = 0
    for k in range(8):
        eng.update(11), ora.update(11)
        against_oracle(eng, ora, n, f64, f"{where}, block {k}")
        q = ora.joint_states()[0]
        near = (np.abs(np.abs(q) - 0.003) < (1e-9 if f64 else 2e-5)).any(axis=1)
        gm, om = eng.limit_state(), ora.limit_state()
        assert np.array_equal(gm[~near], om[~near]), f"{where}: limit masks differ after block {k}"
        limit_bits |= int(np.bitwise_or.reduce(gm))
        dbg = float(np.abs(eng.pid_debug() - ora.pid_debug()).max())
        note(n, "pid_debug64" if f64 else "pid_debug", dbg)
        assert dbg < (1e-4 if f64 else 2e-2), where
    for i in range(8, n):
        assert limit_bits & (1 << i), f"{where}: cable {i} never crossed its travel limit"
    f = rng.uniform(2.0, 45.0, (B, n)).astype(np.float32)  # (some beyond the 30 N clamp)
    eng.set_force_command(f), ora.set_force_command(f)
    eng.update(13), ora.update(13)
    against_oracle(eng, ora, n, f64, f"{where}, force mode")
    assert (f > 30.0).any() and np.abs(eng.joint_states()[2]).max() <= 30.0
    eng.update(20, 10), ora.update(20)
    against_oracle(eng, ora, n, f64, f"{where}, force mode fused")
    eng.close()


# ---- d. the facade ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_call", [1, 25])
@pytest.mark.parametrize("n", [10, 12])
def test_facade_publishes_the_oracle_at_ten_and_twelve_cables(pkg, oracle, n, per_call):
    """CdprGazeboPlugin.update(1) per world step publishes through cdpr_get_observables, update(25) through the trajectory record;
    every JointState and PlatformState message is the oracle's step (as test_facade_publishes_every_step_and_wire_states)."""
    B = 3
    cfg = pkg.Config(model=model_of(pkg, n), batch=B, stages=3)
    plug = pkg.CdprGazeboPlugin()
    plug.Load(cfg)
    got = {"joint": [], "platform": []}
    plug.bus.subscribe("jointStates", got["joint"].append)
    plug.bus.subscribe("platformPose", got["platform"].append)
    ora = oracle.OracleSim(cfg.to_struct())
    rng = np.random.default_rng(60 + n)
    expected = []
    for k in range(4):
        cmd = rng.uniform(-0.05, 0.05, (B, n)).astype(np.float32)
        plug.bus.publish("jointVelocities", pkg.Joy(axes=cmd))
        ora.set_velocity_command(cmd)
        for _ in range(25 // per_call):
            plug.update(per_call)
        for _ in range(25):
            ora.update(1)
            expected.append(ora.joint_states() + ora.platform_state())
    assert len(got["joint"]) == len(got["platform"]) == 99
    for k, (js, ps) in enumerate(zip(got["joint"], got["platform"])):
        oq, oqd, oe, op, ot = expected[k + 1]
        assert abs(js.header.stamp - 1e-3 * (k + 1)) < 1e-12 and abs(ps.header.stamp - js.header.stamp) < 1e-15
        for name, g, o in (("q", js.position, oq), ("qd", js.velocity, oqd), ("eff", js.effort, oe), ("pose", ps.pose.position, op[:, :3]),
                           ("pose", ps.pose.orientation, op[:, 3:]), ("twist", ps.velocity.linear, ot[:, :3]), ("twist", ps.velocity.angular, ot[:, 3:])):
            err = float(np.abs(np.asarray(g) - o).max())
            assert np.asarray(g).shape == o.shape and err <= TOL[name], f"n = {n}, update({per_call}), message {k}: {name} off by {err:.3e}"
    plug.engine.close()


def test_zz_report_measured_agreement():
    """Largest error seen per quantity and cable count in this module's run (printed with -s)."""
    for (n, name), err in sorted(WORST.items()):
        print(f"cable-count agreement: n = {n:2d} {name:12s} {err:.3e}")
