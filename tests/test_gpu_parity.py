"""Parity tests proper: the HIP engine, called through the C-ABI, against the CPU fp64 oracle on the same
seeded inputs.  Everything on the GPU is fp32; the tolerances (TOL), the comparison and the making of an engine with its oracle are
those of tests/parity.py.
"""
import numpy as np
import pytest
from scipy.spatial.transform import Rotation

from parity import FULL_SIZE_SLICES, TOL, check_slice, compare, pair, perturbed_poses, rollout_cost_tol, run_script

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["lane_per_robot", "lane_pair", "lane_per_cable"])
def mapping(request, monkeypatch):
    """Every test runs under the three wavefront mappings (CDPR_MAPPING overrides CDPR_MAP_AUTO at cdpr_create): one lane
    per robot, two lanes per robot (n = 4 or 8), one lane per cable (8 lanes per robot, cdpr_step_kernel_cable.hpp).  Handles
    a mapping cannot serve (other cable counts for the pair mapping; the general controller path, per-robot modes, the
    optional physics for both) fall back to one lane per robot by themselves; tests of such paths run once (`once`)."""
    monkeypatch.setenv("CDPR_MAPPING", {"lane_per_robot": "1", "lane_pair": "2", "lane_per_cable": "3"}[request.param])
    return request.param


def once(mapping):
    """For code paths that do not depend on the wavefront mapping (general controller path, one-shot solvers,
    rollout): run them under one fixture value only."""
    if mapping != "lane_per_robot":
        pytest.skip("independent of the wavefront mapping: run once")


def test_config1_sine_velocity_trajectory(pkg, oracle):
    """BASELINE config 1: the shipped 4-cable robot driven by sinevelocitytest (100 Hz, zero-order hold),
    3 000 steps of 1 ms, GPU fp32 vs oracle fp64 along the whole trajectory."""
    cfg = pkg.Config(batch=1)
    eng, ora = pair(pkg, oracle, cfg)
    gen = pkg.stimulus.sine_velocity(4)
    for k in range(300):
        cmd = next(gen)
        eng.set_velocity_command(cmd), ora.set_velocity_command(cmd)
        eng.update(10), ora.update(10)
        if k % 10 == 9:
            compare(eng, ora, where=f"step {10 * (k + 1)}")
    assert eng.step_count == ora.step_count == 3000


def test_position_hold_from_load(pkg, oracle):
    """No command at all: Position mode with target 0 (PLG.cpp:153-157) holds the platform against gravity."""
    eng, ora = pair(pkg, oracle, pkg.Config(batch=2))
    for _ in range(10):
        eng.update(100), ora.update(100)
        compare(eng, ora, where="hold")
    assert 0.2 < eng.platform_state()[0][0, 2] < 0.31  # hanging under its cables, not in free fall (would be -4.6 m)


def test_first_steps_match_exactly_in_structure(pkg, oracle):
    """Steps 0 and 1 apply zero force (JFC.cpp:61-66, Pid.cpp:123-126); step 0 is not published."""
    eng, ora = pair(pkg, oracle, pkg.Config(batch=1))
    eng.update(1), ora.update(1)
    assert np.all(eng.joint_states()[2] == 0.0)
    assert np.array_equal(eng.platform_state()[0], np.array([[0, 0, 0.3, 0, 0, 0, 1]], dtype=np.float32))
    eng.update(1), ora.update(1)
    assert np.all(eng.joint_states()[2] == 0.0) and eng.platform_state()[1][0, 2] < 0.0  # falling, published now
    eng.update(1), ora.update(1)
    assert np.all(eng.joint_states()[2] > 0.0)
    compare(eng, ora, where="step 3")


@pytest.mark.parametrize("B", [1, 63, 64, 65, 130, 1000])
def test_config2_random_batch_four_cable(pkg, oracle, B):
    """BASELINE config 2 at oracle-sized batches, including ragged sizes around the 64-lane wavefront."""
    rng = np.random.default_rng(1234)
    cfg = pkg.Config(batch=B)
    eng, ora = pair(pkg, oracle, cfg, perturbed_poses(cfg.model, B, rng))
    amp, freq, ph = rng.uniform(0.01, 0.05, (B, 1)), rng.uniform(0.05, 0.5, (B, 1)), rng.uniform(0, 2 * np.pi, (B, 1))
    for j in range(20):
        cmd = np.repeat(amp * np.sin(2 * np.pi * freq * j * 0.01 + ph), 4, axis=1).astype(np.float32)
        assert eng.set_velocity_command(cmd) == ora.set_velocity_command(cmd) == 0
        eng.update(10), ora.update(10)
    compare(eng, ora, where=f"B={B}")


@pytest.mark.parametrize("stages", [0, 1, 2, 3])
def test_config3_eight_cable_stage_combinations(pkg, oracle, stages):
    """BASELINE config 3 (IK + NR-FK + TD + PID + dynamics) and its stage subsets, 8 cables."""
    B = 200
    rng = np.random.default_rng(1235)
    cfg = pkg.Config(model=pkg.eight_cable_model(), batch=B, stages=stages)
    eng, ora = pair(pkg, oracle, cfg, perturbed_poses(cfg.model, B, rng))
    eng.update(30), ora.update(30)
    for j in range(20):
        cmd = rng.uniform(-0.05, 0.05, (B, 8)).astype(np.float32)
        eng.set_velocity_command(cmd), ora.set_velocity_command(cmd)
        eng.update(10), ora.update(10)
    compare(eng, ora, where=f"stages={stages}")
    if stages & 1:
        gp, gr, gi = eng.fk_state()
        op, orr, oi = ora.fk_state()
        assert np.array_equal(gi, oi) and np.abs(gp - op).max() < 1e-5 and gr.max() < 1e-6
        true_pose, _ = eng.platform_state()
        assert np.abs(gp[:, :3] - true_pose[:, :3]).max() < 2e-6  # the estimator recovers the true pose
    if stages & 2:
        gt, gf = eng.td_state()
        ot, of = ora.td_state()
        assert np.array_equal(gf, of) and np.abs(gt - ot).max() < TOL["eff"]
        assert gt.min() >= 5.0 and gt.max() <= 100.0


def test_six_and_seven_cable_robots(pkg, oracle, mapping):
    """Cable counts between the shipped 4 and the build-defined 8 (drop cables from the 8-cable layout)."""
    once(mapping)
    full = pkg.eight_cable_model()
    for keep in ([0, 1, 2, 3, 4, 6], [0, 1, 2, 3, 4, 5, 6]):
        m = pkg.Model(full.frame_anchors[keep], full.platform_anchors[keep])
        cfg = pkg.Config(model=m, batch=70, stages=1)
        eng, ora = pair(pkg, oracle, cfg)
        eng.update(100), ora.update(100)
        compare(eng, ora, where=f"n={len(keep)}")


def test_mode_switching_resets_the_right_pid(pkg, oracle):
    """Velocity -> Position -> Velocity, plus both commands in one update (velocity is applied first, then
    position: PLG.cpp:206-219), against the oracle's two-Pid JointForceCalculator."""
    B = 40
    rng = np.random.default_rng(77)
    cfg = pkg.Config(batch=B)
    eng, ora = pair(pkg, oracle, cfg)
    script = [("run", 25), ("vel", 0.03), ("run", 40), ("pos", -0.01), ("run", 40), ("vel", -0.02), ("run", 15), ("vel", 0.01), ("run", 15),
              ("both", (0.02, 0.005)), ("run", 40), ("pos", 0.0), ("run", 20)]
    for kind, val in script:
        for sim in (eng, ora):
            if kind == "vel":
                sim.set_velocity_command(np.full(4, val, dtype=np.float32))
            elif kind == "pos":
                sim.set_position_command(np.full((B, 4), val, dtype=np.float32))
            elif kind == "both":
                sim.set_velocity_command(np.full(4, val[0], dtype=np.float32))
                sim.set_position_command(np.full(4, val[1], dtype=np.float32))
            else:
                sim.update(val)
        if kind == "run":
            compare(eng, ora, where=f"after {kind} {val}")


def test_saturation_and_anti_windup(pkg, oracle):
    """A 2 m/s velocity demand saturates the command clamp (Pid.cpp:175-186) and the SetForce effort clamp.  cmdLimit equals the
    effort limit here (both 100), so what the anti-windup leaves one increment BEYOND the command clamp is cut off by SetForce and
    never reaches an observable: tests/test_gpu_pid_limits.py runs the clamps apart (cmdLimit 12 under an effort limit of 20 and
    above one of 9) in every kernel family."""
    cfg = pkg.Config(batch=3)
    eng, ora = pair(pkg, oracle, cfg)
    cmd = np.array([[2.0] * 4, [-2.0] * 4, [0.5, -0.5, 0.5, -0.5]], dtype=np.float32)
    eng.update(5), ora.update(5)
    eng.set_velocity_command(cmd), ora.set_velocity_command(cmd)
    eng.update(3), ora.update(3)
    ge = eng.joint_states()[2]
    assert np.all(np.abs(ge[0]) == 100.0) and np.all(np.abs(ge[1]) == 100.0)  # past the Pid clamp, held by the effort clamp
    eng.update(30), ora.update(30)
    compare(eng, ora, tol=dict(TOL, eff=5e-2), where="saturated")


def test_wrong_length_commands_are_ignored(pkg, oracle):
    """PLG.cpp:68-73,77-82: a Joy whose axes count is not n (or n*B) is dropped silently; state untouched."""
    cfg = pkg.Config(batch=5)
    eng, ref = pkg.Engine(cfg, 0), pkg.Engine(cfg, 0)
    assert eng.set_velocity_command(np.ones(3, dtype=np.float32)) == pkg._abi.IGNORED
    assert eng.set_position_command(np.ones(21, dtype=np.float32)) == pkg._abi.IGNORED
    assert eng.set_velocity_command(np.ones(8, dtype=np.float32)) == pkg._abi.IGNORED
    eng.update(50), ref.update(50)
    assert np.array_equal(eng.raw_state()[0], ref.raw_state()[0]) and np.array_equal(eng.joint_states()[2], ref.joint_states()[2])


def test_fused_launch_is_bit_identical_to_single_step_launches(pkg):
    """steps_per_launch only changes where state lives between steps, not the arithmetic."""
    B = 300
    rng = np.random.default_rng(5)
    cfg = pkg.Config(model=pkg.eight_cable_model(), batch=B, stages=3)
    pose = perturbed_poses(cfg.model, B, rng).astype(np.float32)
    a, b = pkg.Engine(cfg, 0), pkg.Engine(cfg, 0)
    for e in (a, b):
        e.set_platform_state(pose7=pose)
    cmd = rng.uniform(-0.04, 0.04, (B, 8)).astype(np.float32)
    a.update(7), b.update(7, 7)
    a.set_velocity_command(cmd), b.set_velocity_command(cmd)
    a.update(64), b.update(64, 16)
    a.update(5), b.update(5, 3)
    for x, y in zip(a.raw_state() + a.joint_states() + a.platform_state(), b.raw_state() + b.joint_states() + b.platform_state()):
        assert np.array_equal(x, y)
    assert a.step_count == b.step_count == 76


def test_publish_period_decimation(pkg, oracle):
    cfg = pkg.Config(batch=2, publishPeriod=0.0045)
    eng, ora = pair(pkg, oracle, cfg)
    for k in range(23):
        eng.update(1), ora.update(1)
        assert np.abs(eng.platform_state()[0] - ora.platform_state()[0]).max() < 1e-6, k
    eng2, ora2 = pair(pkg, oracle, cfg)
    eng2.update(23, 8), ora2.update(23)
    assert np.abs(eng2.platform_state()[0] - ora2.platform_state()[0]).max() < 1e-6
    assert np.array_equal(eng2.platform_state()[0], eng.platform_state()[0])


def test_pid_debug_topic(pkg, oracle):
    cfg = pkg.Config(batch=4, stages=pkg._abi.STAGE_PID_DEBUG)
    eng, ora = pair(pkg, oracle, cfg)
    eng.update(2), ora.update(2)
    assert np.all(eng.pid_debug() == 0.0) and np.all(ora.pid_debug() == 0.0)  # nothing written before the Pid really runs
    eng.update(40), ora.update(40)
    cmd = np.full(4, 0.02, dtype=np.float32)
    eng.set_velocity_command(cmd), ora.set_velocity_command(cmd)
    eng.update(1), ora.update(1)  # Pid reset: first call writes nothing, old P/I/D stay on the topic (Pid.cpp:123-126)
    g, o = eng.pid_debug(), ora.pid_debug()
    assert np.abs(g - o).max() < 2e-2 and np.all(g[:, 4] == 0.0) and np.all(g[:, 0] != 0.0)
    eng.update(30), ora.update(30)
    g, o = eng.pid_debug(), ora.pid_debug()
    assert np.abs(g - o).max() < 2e-2 and np.allclose(g[:, 3], 0.02) and np.all(g[:, 5:] == 0.0)


def test_reset_restores_load_state(pkg):
    cfg = pkg.Config(batch=10)
    eng = pkg.Engine(cfg, 0)
    eng.update(3)
    first = eng.raw_state()[0].copy(), eng.joint_states()[2].copy()
    eng.set_velocity_command(np.full(4, 0.03, dtype=np.float32))
    eng.update(100)
    eng.reset()
    assert eng.step_count == 0
    eng.update(3)
    assert np.array_equal(eng.raw_state()[0], first[0]) and np.array_equal(eng.joint_states()[2], first[1])


def test_plugin_facade_end_to_end(pkg, oracle):
    """The drop-in surface: topic strings, callback names, message fields (PLG.h:23-28,92-102)."""
    cfg = pkg.Config(batch=1)
    plug = pkg.CdprGazeboPlugin()
    plug.Load(cfg)
    got = {"joint": [], "platform": []}
    plug.bus.subscribe("jointStates", got["joint"].append)
    plug.bus.subscribe("platformPose", got["platform"].append)
    ora = oracle.OracleSim(cfg.to_struct())
    gen = pkg.stimulus.sine_velocity(4)
    for k in range(50):
        cmd = next(gen)
        plug.bus.publish("jointVelocities", pkg.Joy(axes=cmd))
        plug.bus.publish("jointVelocities", pkg.Joy(axes=np.zeros(3)))  # wrong size: ignored
        ora.set_velocity_command(cmd)
        plug.update(10), ora.update(10)
    # one message per world iteration, as the reference publishes at publishPeriod 0 (PLG.cpp:236-242); step 0 is not
    # published (0 - 0 > 0 is false): 500 steps -> 499 messages with stamps 0.001 .. 0.499
    assert len(got["joint"]) == len(got["platform"]) == 499
    assert all(abs(m.header.stamp - 1e-3 * (k + 1)) < 1e-12 for k, m in enumerate(got["joint"]))
    js, ps = got["joint"][-1], got["platform"][-1]
    assert js.name == ["cable0", "cable1", "cable2", "cable3"] and js.position.shape == (1, 4)
    oq, oqd, oe = ora.joint_states()
    op, ot = ora.platform_state()
    assert np.abs(js.effort - oe).max() < TOL["eff"] and np.abs(js.position - oq).max() < TOL["q"]
    assert np.abs(ps.pose.position - op[:, :3]).max() < TOL["pose"] and np.abs(ps.pose.orientation - op[:, 3:]).max() < TOL["pose"]
    assert np.abs(ps.velocity.linear - ot[:, :3]).max() < TOL["twist"]
    assert abs(js.header.stamp - 0.499) < 1e-12


def test_full_size_properties_config3(pkg, oracle):
    """BASELINE config 3 at full size (65 536 x 8 cables), the headline kernel at the headline size (every SIMD of the
    chip hosting an estimator and a controller wave): three 128-robot slices against the ORACLE, and on the whole batch
    the size-independent properties — unit quaternions, FK estimate == true pose, tensions inside [f_min, f_max], robots
    started identically stay identical (no cross-robot leakage), a permutation of the batch permutes the result."""
    B = 65536
    rng = np.random.default_rng(1235)
    cfg = pkg.Config(model=pkg.eight_cable_model(), batch=B, stages=3)
    pose = perturbed_poses(cfg.model, B, rng).astype(np.float32)
    pose[B // 2:] = pose[: B // 2]  # second half duplicates the first
    cmd = rng.uniform(-0.05, 0.05, (B, 8)).astype(np.float32)
    cmd[B // 2:] = cmd[: B // 2]
    eng = pkg.Engine(cfg, 0)
    eng.set_platform_state(pose7=pose)
    eng.update(20)
    eng.set_velocity_command(cmd)
    eng.update(200)
    p, t = eng.platform_state()
    q, qd, eff = eng.joint_states()
    assert np.isfinite(p).all() and np.isfinite(eff).all()
    assert np.abs(np.linalg.norm(p[:, 3:], axis=1) - 1.0).max() < 1e-6
    assert np.array_equal(p[: B // 2], p[B // 2:]) and np.array_equal(eff[: B // 2], eff[B // 2:])
    fk_pose, res, it = eng.fk_state()
    assert res.max() < 1e-6 and np.all(it == 4) and np.abs(fk_pose[:, :3] - p[:, :3]).max() < 5e-6
    ten, flag = eng.td_state()
    assert ten.min() >= 5.0 and ten.max() <= 100.0
    for sl in FULL_SIZE_SLICES:
        check_slice(pkg, oracle, dict(model=cfg.model, stages=3), sl, pose, [(20, None), (200, cmd)], (p, t, q, qd, eff))
    # permutation equivariance on a slice
    perm = rng.permutation(4096)
    cfg2 = pkg.Config(model=pkg.eight_cable_model(), batch=4096, stages=3)
    e2 = pkg.Engine(cfg2, 0)
    e2.set_platform_state(pose7=pose[:4096][perm])
    e2.update(20)
    e2.set_velocity_command(cmd[:4096][perm])
    e2.update(200)
    assert np.array_equal(e2.platform_state()[0], p[:4096][perm])


def test_full_size_position_mode_config3(pkg, oracle):
    """The same 65 536 x 8 launch shape in Position mode (jointPositions Joys, the position Pid's gains 200 / 70 / 80):
    a velocity phase first, so that the mode switch resets the Pid records of the whole batch (JFC.cpp:101-103), then two
    position targets; three slices against the oracle."""
    B = 65536
    rng = np.random.default_rng(1237)
    cfg = pkg.Config(model=pkg.eight_cable_model(), batch=B, stages=3)
    pose = perturbed_poses(cfg.model, B, rng, 0.03, 0.06).astype(np.float32)
    vel = rng.uniform(-0.03, 0.03, (B, 8)).astype(np.float32)
    pos1 = rng.uniform(-0.004, 0.004, (B, 8)).astype(np.float32)
    pos2 = rng.uniform(-0.004, 0.004, (B, 8)).astype(np.float32)
    eng = pkg.Engine(cfg, 0)
    eng.set_platform_state(pose7=pose)
    eng.update(15)
    eng.set_velocity_command(vel)
    eng.update(40)
    eng.set_position_command(pos1)
    eng.update(90)
    eng.set_position_command(pos2)
    eng.update(75)
    got = eng.platform_state() + eng.joint_states()
    assert all(np.isfinite(x).all() for x in got)
    script = [(15, None), (40, vel), (90, ("pos", pos1)), (75, ("pos", pos2))]
    for sl in FULL_SIZE_SLICES:
        check_slice(pkg, oracle, dict(model=cfg.model, stages=3), sl, pose, script, got)


# ---------------------------------------------------------------------------------------------
# general controller path (cdpr_general_step.hpp): hold branch, biquad cascades, long windows, cmdLimit 0
# ---------------------------------------------------------------------------------------------
def test_general_path_position_hold_branch(pkg, oracle, mapping):
    """velocityEpsilon > 0: cables whose |target| <= eps hold position with the POSITION Pid while the others keep
    their velocity Pid (JFC.cpp:72-82); both Pids stay alive and are sampled at non-uniform times."""
    once(mapping)
    B = 50
    rng = np.random.default_rng(21)
    cfg = pkg.Config(batch=B, velocityEpsilon=0.01)
    eng, ora = pair(pkg, oracle, cfg, perturbed_poses(cfg.model, B, rng, 0.02, 0.05))
    script = [("run", 15)]
    for j in range(12):
        cmd = rng.uniform(-0.03, 0.03, (B, 4)).astype(np.float32)
        cmd[rng.random((B, 4)) < 0.4] *= 0.1  # a good share below eps -> hold branch
        script += [("vel", cmd), ("run", 7 + j)]
    script += [("pos", np.full(4, 0.002, dtype=np.float32)), ("run", 30), ("vel", np.zeros(4, dtype=np.float32)), ("run", 30)]
    run_script(eng, ora, script, label="hold")


@pytest.mark.parametrize("cascade", [1, 2])
def test_general_path_biquad_cascades(pkg, oracle, cascade, mapping):
    """P and D inputs of the velocity Pid through 1 or 2 low-pass biquads (Pid.cpp:27-44, Filter.h:130-165)."""
    once(mapping)
    B = 40
    rng = np.random.default_rng(22 + cascade)
    cfg = pkg.Config(batch=B)
    cfg.velocityController.pFilter.cascade = cascade
    cfg.velocityController.dFilter.cascade = cascade
    eng, ora = pair(pkg, oracle, cfg)
    # The filters' phase lag makes this velocity loop unstable (in the oracle too: efforts rail at +-100 N after
    # ~50 steps and any rounding difference is amplified from then on), so the comparison covers the 30 steps
    # before that, where GPU and oracle agree to 5e-3 N, and then only checks that both saturate alike.
    script = [("run", 20)]
    for j in range(3):
        script += [("vel", rng.uniform(-0.04, 0.04, (B, 4)).astype(np.float32)), ("run", 10)]
    run_script(eng, ora, script, tol=dict(TOL, eff=5e-3), label=f"cascade{cascade}")
    eng.update(60), ora.update(60)
    ge, oe = eng.joint_states()[2], ora.joint_states()[2]
    assert np.abs(ge - oe).max() < 0.5 and np.abs(eng.platform_state()[0] - ora.platform_state()[0]).max() < 1e-5
    # a gentle (stable) loop through the same filters, long horizon
    cfg2 = pkg.Config(batch=B)
    for f in (cfg2.velocityController.pFilter, cfg2.velocityController.dFilter):
        f.cascade, f.relCutoff, f.quality = cascade, 0.05, 0.5
    cfg2.velocityController.pGain, cfg2.velocityController.iGain, cfg2.velocityController.dGain = 4.0, 40.0, 0.01
    eng2, ora2 = pair(pkg, oracle, cfg2)
    script = [("run", 20)]
    for j in range(20):
        script += [("vel", rng.uniform(-0.02, 0.02, (B, 4)).astype(np.float32)), ("run", 10)]
    run_script(eng2, ora2, script, label=f"gentle cascade{cascade}")


@pytest.mark.parametrize("nbuf,deg", [(21, 3), (32, 4), (5, 1)])
def test_general_path_long_windows_and_degrees(pkg, oracle, nbuf, deg, mapping):
    once(mapping)
    B = 30
    rng = np.random.default_rng(nbuf)
    cfg = pkg.Config(model=pkg.eight_cable_model(), batch=B, stages=3, velocityEpsilon=0.0)
    for p in (cfg.velocityController, cfg.positionController):
        p.dBufferLength, p.dDegree = nbuf, deg
    eng, ora = pair(pkg, oracle, cfg, perturbed_poses(cfg.model, B, rng, 0.03, 0.05))
    script = [("run", 40), ("vel", rng.uniform(0.005, 0.04, (B, 8)).astype(np.float32)), ("run", 60), ("pos", np.zeros(8, dtype=np.float32)), ("run", 60)]
    run_script(eng, ora, script, tol=dict(TOL, eff=5e-2), label=f"N{nbuf}d{deg}")


def test_general_path_command_clamp_disabled(pkg, oracle, mapping):
    """cmdLimit = 0: mCmdMax == mCmdMin, so mCmd keeps its old value and the anti-windup branch integrates it
    (Pid.cpp:175-186) — a reference quirk the general path reproduces."""
    once(mapping)
    cfg = pkg.Config(batch=8)
    cfg.velocityController.cmdLimit = 0.0
    eng, ora = pair(pkg, oracle, cfg)
    script = [("run", 10), ("vel", np.full(4, 0.02, dtype=np.float32)), ("run", 100)]
    run_script(eng, ora, script, label="cmdlimit0")


def test_general_and_fast_path_agree_on_the_shipped_config(pkg, oracle):
    """velocityEpsilon = 0 with non-zero targets takes the same branches as the shipped -0.001 but forces the general
    kernels: both GPU paths must agree with each other to fp32 rounding and with the oracle."""
    B = 64
    rng = np.random.default_rng(31)
    pose = perturbed_poses(pkg.cube_model(), B, rng, 0.02, 0.05)
    cmd = rng.uniform(0.005, 0.04, (B, 4)).astype(np.float32) * rng.choice([-1.0, 1.0], (B, 4)).astype(np.float32)
    res = []
    for eps in (-0.001, 0.0):
        cfg = pkg.Config(batch=B, velocityEpsilon=eps, stages=pkg._abi.STAGE_PID_DEBUG)
        eng, ora = pair(pkg, oracle, cfg, pose)
        run_script(eng, ora, [("run", 20), ("vel", cmd), ("run", 80)], label=f"eps{eps}")
        assert np.abs(eng.pid_debug() - ora.pid_debug()).max() < 2e-2
        res.append((eng.platform_state()[0], eng.joint_states()[2]))
    assert np.abs(res[0][0] - res[1][0]).max() < 2e-6 and np.abs(res[0][1] - res[1][1]).max() < 5e-3


# ---------------------------------------------------------------------------------------------
# one-shot solvers (cdpr_solve_ik / cdpr_solve_fk / cdpr_solve_td)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model_name", ["cube", "eight"])
def test_solve_ik_matches_oracle(pkg, oracle, model_name, mapping):
    once(mapping)
    model = pkg.cube_model() if model_name == "cube" else pkg.eight_cable_model()
    B = 133
    rng = np.random.default_rng(3)
    cfg = pkg.Config(model=model, batch=B)
    s = cfg.to_struct()
    pose = perturbed_poses(model, B, rng).astype(np.float32)
    twist = rng.uniform(-0.3, 0.3, (B, 6)).astype(np.float32)
    eng = pkg.Engine(cfg, 0)
    q, qd, jac = eng.solve_ik(pose, twist)
    for r in range(0, B, 7):
        oq, oqd, oln, ojac = oracle.ik(s, pose[r].astype(np.float64), twist[r].astype(np.float64))
        assert np.abs(q[r] - oq).max() < 2e-7 and np.abs(qd[r] - oqd).max() < 2e-7 and np.abs(jac[r] - ojac).max() < 2e-7
    q2, _, _ = eng.solve_ik(pose)  # twist optional
    assert np.array_equal(q, q2)


def test_solve_fk_round_trip_and_oracle(pkg, oracle, mapping):
    """FK(IK(x)) = x on random poses, iteration counts equal to the oracle's (tolerance-controlled early exit)."""
    once(mapping)
    B = 500
    rng = np.random.default_rng(14)
    cfg = pkg.Config(model=pkg.eight_cable_model(), batch=B, stages=1, fkMaxIterations=8, fkTolerance=1e-6)
    s = cfg.to_struct()
    eng = pkg.Engine(cfg, 0)
    pose = perturbed_poses(cfg.model, B, rng).astype(np.float32)
    q, _, _ = eng.solve_ik(pose)
    lengths = cfg.model.reference_lengths()[None, :].astype(np.float32) - q
    seed = np.tile(cfg.model.home_pose(), (B, 1)).astype(np.float32)
    est, res, it = eng.solve_fk(lengths, seed)
    assert res.max() < 1e-6 and np.abs(est[:, :3] - pose[:, :3]).max() < 5e-6
    assert np.abs(np.abs((est[:, 3:] * pose[:, 3:]).sum(axis=1)) - 1.0).max() < 1e-6
    for r in range(0, B, 25):
        oest, ores, oit = oracle.fk(s, lengths[r].astype(np.float64), seed[r].astype(np.float64))
        assert abs(int(it[r]) - oit) <= 1 and np.abs(est[r] - oest).max() < 5e-6
    est0, res0, it0 = eng.solve_fk(np.tile(cfg.model.reference_lengths(), (B, 1)), seed)
    assert np.all(it0 == 0) and res0.max() < 1e-6  # already converged at the seed: no iteration taken


def test_solve_td_matches_oracle_and_flags_infeasible(pkg, oracle, mapping):
    once(mapping)
    B = 96
    rng = np.random.default_rng(15)
    cfg = pkg.Config(model=pkg.eight_cable_model(), batch=B, stages=2)
    s = cfg.to_struct()
    eng = pkg.Engine(cfg, 0)
    pose = perturbed_poses(cfg.model, B, rng, 0.03, 0.05).astype(np.float32)
    wrench = np.tile([0, 0, 9.8, 0, 0, 0], (B, 1)).astype(np.float32) + rng.uniform(-0.5, 0.5, (B, 6)).astype(np.float32) * [1, 1, 1, 0.02, 0.02, 0.02]
    wrench[-1] = [0, 0, 900.0, 0, 0, 0]  # cannot be balanced inside [5, 100] N
    wrench = wrench.astype(np.float32)
    t, flag = eng.solve_td(pose, wrench)
    _, _, jac = eng.solve_ik(pose)
    for r in range(B):
        ot, oflag = oracle.td_wrench(s, pose[r].astype(np.float64), wrench[r].astype(np.float64))
        assert int(flag[r]) == oflag and np.abs(t[r] - ot).max() < 5e-3
        if not oflag:
            assert np.abs(-jac[r].T.astype(np.float64) @ t[r] - wrench[r]).max() < 2e-3  # A T = w_d
    assert flag[-1] == 1 and flag[:-1].sum() == 0 and t.min() >= 5.0 and t.max() <= 100.0


def test_solvers_reject_robots_with_fewer_than_six_cables(pkg, mapping):
    once(mapping)
    eng = pkg.Engine(pkg.Config(batch=4), 0)
    with pytest.raises(pkg.CdprError) as ei:
        eng.solve_fk(np.ones((4, 4)), np.tile(pkg.cube_model().home_pose(), (4, 1)))
    assert ei.value.code == pkg._abi.ERR_UNSUPPORTED


def test_graph_replay_is_bit_identical_to_eager_launches(pkg):
    """update(n) replays captured hipGraphs of 16 launches once the controller is in steady state; the result must
    be bit-identical to n separate update(1) calls (which never form a chain long enough to be captured)."""
    B = 700  # small enough for the graph path (batch * n <= 131072)
    rng = np.random.default_rng(8)
    cfg = pkg.Config(model=pkg.eight_cable_model(), batch=B, stages=3)
    pose = perturbed_poses(cfg.model, B, rng).astype(np.float32)
    a, b = pkg.Engine(cfg, 0), pkg.Engine(cfg, 0)
    for e in (a, b):
        e.set_platform_state(pose7=pose)
    for rnd in range(3):
        cmd = rng.uniform(-0.04, 0.04, (B, 8)).astype(np.float32)
        a.set_velocity_command(cmd), b.set_velocity_command(cmd)
        a.update(100)
        for _ in range(100):
            b.update(1)
        for x, y in zip(a.raw_state() + a.joint_states() + a.platform_state(), b.raw_state() + b.joint_states() + b.platform_state()):
            assert np.array_equal(x, y), rnd
    a.update(70, 2)
    for _ in range(35):
        b.update(2, 2)
    assert np.array_equal(a.raw_state()[0], b.raw_state()[0]) and a.step_count == b.step_count == 370


# ---------------------------------------------------------------------------------------------
# MPC rollout (BASELINE config 5)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start_mode", ["position", "velocity"])
def test_rollout_velocity_matches_oracle_and_leaves_state_untouched(pkg, oracle, start_mode, mapping):
    once(mapping)
    B, S, H = 12, 16, 24
    rng = np.random.default_rng(1236)
    cfg = pkg.Config(model=pkg.eight_cable_model(), batch=B, stages=3)
    eng, ora = pair(pkg, oracle, cfg, perturbed_poses(cfg.model, B, rng, 0.03, 0.05))
    eng.update(30), ora.update(30)
    if start_mode == "velocity":  # controller already warm in Velocity mode: no reset at rollout entry
        cmd0 = rng.uniform(-0.02, 0.02, (B, 8)).astype(np.float32)
        eng.set_velocity_command(cmd0), ora.set_velocity_command(cmd0)
        eng.update(25), ora.update(25)
    nominal = rng.uniform(-0.03, 0.03, (B, H, 1, 8))
    commands = (nominal + rng.normal(0.0, 0.01, (B, H, S, 8))).astype(np.float32)
    ref = eng.raw_state()[0][:, :3].astype(np.float64) + [0.0, 0.0, 0.01]
    before = eng.raw_state() + eng.joint_states()
    gc = eng.rollout_velocity(commands, ref)
    oc = ora.rollout_velocity(commands, ref)
    assert gc.shape == (B, S)
    assert np.abs(gc - oc).max() < rollout_cost_tol(oc, 1e-6), (np.abs(gc - oc).max(), np.abs(oc).max())
    assert (gc.argmin(axis=1) == oc.argmin(axis=1)).mean() > 0.9  # the MPC would pick the same sample
    after = eng.raw_state() + eng.joint_states()
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    eng.update(10), ora.update(10)  # and the engine carries on as if nothing happened
    compare(eng, ora, where="after rollout")


def test_rollout_of_identical_samples_equals_plain_stepping(pkg, mapping):
    """Size-independent property: S copies of one command sequence give S equal costs, equal to stepping the engine."""
    once(mapping)
    B, S, H = 130, 4, 20
    rng = np.random.default_rng(5)
    cfg = pkg.Config(model=pkg.eight_cable_model(), batch=B, stages=3)
    eng = pkg.Engine(cfg, 0)
    eng.set_platform_state(pose7=perturbed_poses(cfg.model, B, rng).astype(np.float32))
    eng.update(40)
    seq = rng.uniform(-0.03, 0.03, (B, H, 1, 8)).astype(np.float32)
    ref = np.zeros((B, 3))
    cost = eng.rollout_velocity(np.repeat(seq, S, axis=2), ref)
    assert np.array_equal(cost[:, 0], cost[:, 1]) and np.array_equal(cost[:, 0], cost[:, S - 1])
    acc = np.zeros(B)
    for k in range(H):
        eng.set_velocity_command(seq[:, k, 0, :])
        eng.update(1)
        acc += (eng.raw_state()[0][:, :3].astype(np.float64) ** 2).sum(axis=1)
    assert np.abs(cost[:, 0] - acc).max() < 1e-4 * acc.max()


def test_sharded_engine_equals_single_engine(pkg, mapping):
    """Config-4 style placement in one process: contiguous robot blocks on several handles (here all on GPU 0, the box
    has one), no exchange between them; result identical to one handle holding the whole batch."""
    once(mapping)
    B = 333
    rng = np.random.default_rng(44)
    cfg = pkg.Config(model=pkg.eight_cable_model(), batch=B, stages=3, mapping=pkg._abi.MAP_LANE_PER_ROBOT)
    pose = perturbed_poses(cfg.model, B, rng).astype(np.float32)
    cmd = rng.uniform(-0.04, 0.04, (B, 8)).astype(np.float32)
    one = pkg.Engine(cfg, 0)
    many = pkg.ShardedEngine(cfg, devices=[0, 0, 0])
    assert [hi - lo for lo, hi in many.spans] == [111, 111, 111]
    for e in (one, many):
        e.set_platform_state(pose7=pose)
        e.update(20)
        assert e.set_velocity_command(cmd) == 0 and e.set_velocity_command(np.zeros(5)) == 1
        e.update(60)
        e.set_position_command(np.zeros(8, dtype=np.float32))
        e.update(30, 5)
    for x, y in zip(one.raw_state() + one.joint_states() + one.fk_state(), many.raw_state() + many.joint_states() + many.fk_state()):
        assert np.array_equal(x, y)
    assert many.step_count == one.step_count == 110
    cmds = rng.uniform(-0.03, 0.03, (B, 6, 3, 8)).astype(np.float32)
    ref = np.zeros((B, 3), dtype=np.float32)
    assert np.array_equal(one.rollout_velocity(cmds, ref), many.rollout_velocity(cmds, ref))
    many.close()


# ---------------------------------------------------------------------------------------------
# randomised configurations: every constant the step depends on, not only the shipped ones
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11])
def test_randomised_model_and_controller_parameters(pkg, oracle, seed):
    """Random mass / full inertia tensor / gravity direction / damping / effort limit / dt / gains / window length
    (fast path: N <= 11) / FK iteration count and tolerance / tension bounds, on 4-, 6- and 8-cable robots (seeds 0-5,
    90 robots) and on 5-, 7- and 8-cable robots in a ragged batch of 257 (seeds 6-11: odd cable counts pad a pair)."""
    rng = np.random.default_rng(100 + seed)
    base = pkg.eight_cable_model()
    n = [4, 6, 8][seed % 3] if seed < 6 else [7, 5, 8][seed % 3]
    B = 90 if seed < 6 else 257
    if n == 4:
        model = pkg.cube_model()
    else:
        keep = {8: list(range(8)), 7: [0, 1, 2, 3, 4, 5, 6], 6: [0, 1, 2, 3, 4, 6], 5: [0, 1, 2, 4, 6]}[n]
        model = pkg.Model(base.frame_anchors[keep] + rng.uniform(-0.01, 0.01, (n, 3)), base.platform_anchors[keep] * rng.uniform(0.8, 1.3))
    a = rng.uniform(0.5, 2.0, 3)
    off = rng.uniform(-0.1, 0.1, 3)
    model.mass = float(rng.uniform(0.5, 3.0))
    model.inertia = (a[0], a[1], a[2], off[0], off[1], off[2])  # full symmetric tensor -> gyroscopic term active
    model.joint_damping = float(rng.uniform(0.0, 3.0))
    model.effort_limit = float(rng.choice([50.0, 100.0, -1.0]))  # -1: SetForce clamp disabled
    stages = 0 if n < 6 else int(rng.integers(0, 4))  # the FK / TD stages need six cables
    dt = float(rng.choice([5e-4, 1e-3, 2e-3]))
    cfg = pkg.Config(model=model, batch=B, stages=stages, dt=dt,
                     gravity=tuple(rng.normal(0, 1, 3) * [1.0, 1.0, 0.2] + [0, 0, -9.8]),
                     fkMaxIterations=int(rng.integers(1, 7)), fkTolerance=float(rng.choice([0.0, 1e-6])),
                     tdFMin=float(rng.uniform(1.0, 8.0)), tdFMax=float(rng.uniform(60.0, 150.0)))
    for p in (cfg.velocityController, cfg.positionController):
        p.pGain, p.iGain, p.dGain = float(rng.uniform(50, 250)), float(rng.uniform(0, 80)), float(rng.uniform(0, 40)) * (0.05 if p is cfg.velocityController else 1.0)
        p.dBufferLength = int(rng.integers(3, 12))
        p.dDegree = int(rng.integers(1, min(3, p.dBufferLength - 1) + 1))
        p.iLimit, p.cmdLimit = float(rng.uniform(5, 100)), float(rng.uniform(40, 120))
    cfg.velocityController.forwardGain = float(rng.uniform(0, 20))
    if seed >= 6:
        # the second set is about odd cable counts and ragged batches, so its loops must be STABLE: with the free gain draw above
        # seeds 9 and 11 are not (velocity P = 110 / 208: the efforts flip sign every step with growing amplitude until they sit
        # on the command limit, -13 -> +17 -> -15 -> ... -> +-84 N, and any fp32 rounding difference grows with them: measured,
        # 0.2 % of the swing in 2 of 257 robots).  Shipped gains x (0.6 .. 1.1), windows and limits stay random.
        g = np.random.default_rng(1000 + seed)
        shipped = pkg.Config()
        for p, q in ((cfg.velocityController, shipped.velocityController), (cfg.positionController, shipped.positionController)):
            p.pGain, p.iGain, p.dGain = (float(v * g.uniform(0.6, 1.1)) for v in (q.pGain, q.iGain, q.dGain))
        cfg.velocityController.forwardGain = float(shipped.velocityController.forwardGain * g.uniform(0.6, 1.1))
    eng, ora = pair(pkg, oracle, cfg, perturbed_poses(model, B, rng, 0.03, 0.08), rng.uniform(-0.02, 0.02, (B, 6)))
    script = [("run", 17)]
    for j in range(6):
        kind = "vel" if j != 3 else "pos"
        amp = 0.04 if kind == "vel" else 0.004
        script += [(kind, rng.uniform(-amp, amp, (B, n)).astype(np.float32)), ("run", 9 + j)]
    run_script(eng, ora, script, tol=dict(TOL, eff=5e-2, twist=5e-4, qd=5e-4), label=f"seed{seed} n={n} stages={stages}")


# ---------------------------------------------------------------------------------------------
# the reference's other stimulus publishers, end to end through the facade
# ---------------------------------------------------------------------------------------------
def test_square_position_publisher_end_to_end(pkg, oracle):
    """squarepositiontest.cpp: 10 Hz square wave of +-0.05 m on jointPositions -> Position mode, position Pid
    (200 / 70 / 80), 100 world steps per command sample."""
    cfg = pkg.Config(batch=1)
    plug = pkg.CdprGazeboPlugin()
    plug.Load(cfg)
    ora = oracle.OracleSim(cfg.to_struct())
    gen = pkg.stimulus.square_position(4, amp=0.01)  # 0.05 m would rail the 100 N effort limit for most of the run
    last = []
    plug.bus.subscribe("jointStates", last.append)
    for k in range(12):
        cmd = next(gen)
        plug.bus.publish("jointPositions", pkg.Joy(axes=cmd))
        ora.set_position_command(cmd)
        plug.update(100), ora.update(100)
    oq, oqd, oe = ora.joint_states()
    assert np.abs(last[-1].position - oq).max() < TOL["q"] and np.abs(last[-1].effort - oe).max() < 5e-2
    assert np.all(last[-1].effort > 0.0)  # pulling towards the commanded (shorter) lengths against gravity


def test_square_velocity_publisher_with_position_hold(pkg, oracle, mapping):
    """squarevelocitytest.cpp (+-0.06 m/s gated by |sin| >= sqrt(1/2), else 0) with a POSITIVE velocityEpsilon: during
    the zero phases JointForceCalculator holds the last position with the position Pid (JFC.cpp:78-82) — the branch
    that is dead at the shipped epsilon of -0.001."""
    once(mapping)
    cfg = pkg.Config(batch=2, velocityEpsilon=0.001)
    plug = pkg.CdprGazeboPlugin()
    plug.Load(cfg)
    ora = oracle.OracleSim(cfg.to_struct())
    gen = pkg.stimulus.square_velocity(4, amp=0.02)
    got = []
    plug.bus.subscribe("platformPose", got.append)
    for k in range(60):  # 6 s: zero phase, +0.02 phase, zero phase (hold), ...
        cmd = next(gen)
        plug.bus.publish("jointVelocities", pkg.Joy(axes=cmd))
        ora.set_velocity_command(cmd)
        plug.update(100), ora.update(100)
        if k % 10 == 9:
            op, ot = ora.platform_state()
            assert np.abs(got[-1].pose.position - op[:, :3]).max() < TOL["pose"], k
            assert np.abs(plug.engine.joint_states()[2] - ora.joint_states()[2]).max() < 5e-2, k


def test_long_horizon_stays_on_the_oracle(pkg, oracle):
    """20 000 world steps (20 s of sim time) of the sine stimulus: fp32 rounding must not accumulate into drift — the
    ring window, the call counter folding (pid_calls -> [60, 70)) and the hipGraph replay all cycle thousands of times."""
    cfg = pkg.Config(batch=6)
    eng, ora = pair(pkg, oracle, cfg)
    gen = pkg.stimulus.sine_velocity(4)
    for k in range(200):
        cmd = next(gen)
        eng.set_velocity_command(cmd), ora.set_velocity_command(cmd)
        eng.update(100), ora.update(100)
        for _ in range(99):
            next(gen)  # the publisher ticks every 10 ms; this test latches one sample per 100 ms
        if k % 40 == 39:
            compare(eng, ora, tol=dict(TOL, pose=5e-5, q=5e-5), where=f"t = {(k + 1) * 0.1:.1f} s")
    assert eng.step_count == 20000


def test_optional_physics_terms_velocity_limit_and_unilateral_cables(pkg, oracle):
    """SURVEY 8(f) rank 3, two optional terms: Joint::SetForce's velocity truncation [EXT] and cables that cannot push
    [NEW].  Both must actually change the run (vs the reduced model) and still match the oracle."""
    B = 80
    rng = np.random.default_rng(61)
    results = {}
    for name, vlim, uni in (("reduced", -1.0, False), ("both", 0.01, True)):
        model = pkg.cube_model()
        model.velocity_limit, model.unilateral_cables = vlim, uni
        cfg = pkg.Config(model=model, batch=B)
        rng2 = np.random.default_rng(61)
        eng, ora = pair(pkg, oracle, cfg, perturbed_poses(model, B, rng2, 0.03, 0.08))
        script = [("run", 20)]
        for j in range(8):
            script += [("vel", rng2.uniform(-0.05, 0.05, (B, 4)).astype(np.float32)), ("run", 15)]
        run_script(eng, ora, script, tol=dict(TOL, eff=5e-2), label=name)
        results[name] = eng.platform_state()[0]
    assert np.abs(results["both"] - results["reduced"]).max() > 1e-4  # the options were exercised
    z = pkg.Config().to_struct()
    assert z.velocity_limit <= 0 and z.unilateral_cables == 0  # off by default: the contract's reduced model


def test_matches_the_reference_style_fit_while_it_is_accurate(pkg, oracle, mapping):
    """The oracle's FAITHFUL mode evaluates Pid::fitPolynomial exactly as the reference writes it (normal equations in
    absolute sim time, pow(), pivoted QR; Pid.cpp:219-247).  That fit is accurate for t <~ 2 s and degrades after
    (tests/test_oracle_pid.py); inside that window the GPU's closed-form FIR must agree with it too."""
    once(mapping)
    cfg = pkg.Config(batch=2)
    eng = pkg.Engine(cfg, 0)
    ora = oracle.OracleSim(cfg.to_struct(), oracle.DERIV_FAITHFUL)
    gen = pkg.stimulus.sine_velocity(4)
    for k in range(200):  # 2 s
        cmd = next(gen)
        eng.set_velocity_command(cmd), ora.set_velocity_command(cmd)
        eng.update(10), ora.update(10)
        if k % 25 == 24:
            compare(eng, ora, where=f"faithful, t = {(k + 1) * 0.01:.2f} s")


def test_error_codes_of_the_c_abi(pkg, mapping):
    """Integer return codes, no exceptions across the boundary: < 0 error with a message, > 0 accepted-but-ignored."""
    once(mapping)
    import ctypes as C

    from cdpr_simulation_amd._native import lib

    L = lib()
    eng = pkg.Engine(pkg.Config(batch=3), 0)
    h = eng._h
    f9 = (C.c_float * 27)()
    assert L.cdpr_get_pid_debug(h, f9) == pkg._abi.ERR_UNSUPPORTED and b"PID_DEBUG" in L.cdpr_last_error(h)
    assert L.cdpr_get_fk_state(h, None, None, None) == pkg._abi.ERR_UNSUPPORTED
    assert L.cdpr_get_td_state(h, None, None) == pkg._abi.ERR_UNSUPPORTED
    assert L.cdpr_update(h, -1) == pkg._abi.ERR_INVALID
    assert L.cdpr_update_fused(h, 10, 0) == pkg._abi.ERR_INVALID and L.cdpr_update_fused(h, 10, 65) == pkg._abi.ERR_INVALID
    assert L.cdpr_update(h, 0) == pkg._abi.OK and eng.step_count == 0
    assert L.cdpr_set_velocity_command(h, None, 4) == pkg._abi.ERR_INVALID
    assert L.cdpr_rollout_velocity(h, 0, 4, None, None, None) == pkg._abi.ERR_INVALID
    assert L.cdpr_update(None, 1) == pkg._abi.ERR_INVALID and L.cdpr_step_count(None) == 0
    L.cdpr_destroy(None)  # harmless
    assert L.cdpr_mapping(h) in (pkg._abi.MAP_LANE_PER_ROBOT, pkg._abi.MAP_LANE_PAIR)
    with pytest.raises(ValueError):
        pkg.Engine(pkg.Config(model=pkg.Model(np.zeros((13, 3)), np.zeros((13, 3)))), 0)  # (the engine takes 1..12 cables)
    h2 = C.c_void_p()
    assert L.cdpr_create(C.byref(pkg.Config().to_struct()), 99, C.byref(h2)) == pkg._abi.ERR_INVALID  # no such device
    cfg = pkg.Config(mapping=pkg._abi.MAP_LANE_PAIR, model=pkg.Model(pkg.eight_cable_model().frame_anchors[:6], pkg.eight_cable_model().platform_anchors[:6]))
    with pytest.raises(ValueError, match="lane-pair"):
        pkg.Engine(cfg, 0)


def test_trajectory_record_keeps_every_published_step(pkg, oracle):
    """cdpr_update_record: fused launches, yet nothing a subscriber would have received is lost — the observables of
    every world step, identical to stepping one at a time and reading the topic after each step."""
    B, T = 97, 35
    rng = np.random.default_rng(12)
    cfg = pkg.Config(model=pkg.eight_cable_model(), batch=B, stages=3)
    pose = perturbed_poses(cfg.model, B, rng).astype(np.float32)
    a, b = pkg.Engine(cfg, 0), pkg.Engine(cfg, 0)
    cmd = rng.uniform(-0.03, 0.03, (B, 8)).astype(np.float32)
    for e in (a, b):
        e.set_platform_state(pose7=pose)
        e.update(12)
        e.set_velocity_command(cmd)
    rec = a.update_record(T, steps_per_launch=10)
    for j in range(T):
        b.update(1)
        q, qd, eff = b.joint_states()
        p, t = b.platform_state()
        assert np.array_equal(rec["position"][j], q) and np.array_equal(rec["effort"][j], eff), j
        assert np.array_equal(rec["pose"][j], p) and np.array_equal(rec["twist"][j], t) and np.array_equal(rec["velocity"][j], qd), j
    assert np.array_equal(a.raw_state()[0], b.raw_state()[0])
    assert np.array_equal(a.platform_state()[0], b.platform_state()[0])  # the engine's own topic image follows
    ora = oracle.OracleSim(cfg.to_struct())  # and the recorded trajectory is the oracle's
    ora.set_platform_state(pose7=pose.astype(np.float64))
    ora.update(12), ora.set_velocity_command(cmd), ora.update(T)
    assert np.abs(rec["pose"][-1] - ora.platform_state()[0]).max() < TOL["pose"]
    assert a.step_count == 12 + T


def test_low_register_build_is_bit_identical(pkg, monkeypatch, mapping):
    """Batches above ~82 000 robots use the one-step kernel compiled for two waves per SIMD (cable constants re-read
    from LDS per Newton iteration, true J rebuilt after the Newton stage): same arithmetic, so bit-identical results."""
    once(mapping)
    B = 450
    rng = np.random.default_rng(17)
    cfg = pkg.Config(model=pkg.eight_cable_model(), batch=B, stages=3)
    pose = perturbed_poses(cfg.model, B, rng).astype(np.float32)
    cmd = rng.uniform(-0.04, 0.04, (B, 8)).astype(np.float32)
    out = []
    for flag in ("0", "1"):
        monkeypatch.setenv("CDPR_LOWREG", flag)
        e = pkg.Engine(cfg, 0)
        e.set_platform_state(pose7=pose)
        e.update(15)
        e.set_velocity_command(cmd)
        for _ in range(40):
            e.update(1)
        out.append(e.raw_state() + e.joint_states() + e.fk_state())
    for x, y in zip(*out):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("n_cables,stages", [(8, 3), (8, 1), (8, 2), (8, 0), (4, 0), (5, 0), (7, 3)])
def test_second_generation_onestep_kernel_is_bit_identical(pkg, monkeypatch, mapping, n_cables, stages):
    """cdpr_onestep_kernel (controller rows staged through LDS by LDS-DMA, Newton stage before the PID, structure matrix
    rebuilt) performs the same arithmetic as the first-generation one-step kernel (CDPR_ONESTEP=1): bit-identical state,
    observables, FK estimate and `pid` topic through Load -> position hold -> velocity Joy -> position Joy."""
    once(mapping)
    B = 200
    rng = np.random.default_rng(23)
    model = pkg.eight_cable_model() if n_cables == 8 else pkg.cube_model()
    if n_cables not in (4, 8):
        base = pkg.eight_cable_model()
        from dataclasses import replace

        model = replace(base, frame_anchors=base.frame_anchors[:n_cables], platform_anchors=base.platform_anchors[:n_cables])
    cfg = pkg.Config(model=model, batch=B, stages=stages | pkg._abi.STAGE_PID_DEBUG)
    pose = perturbed_poses(cfg.model, B, rng, 0.03, 0.05).astype(np.float32)
    vel = rng.uniform(-0.04, 0.04, (B, n_cables)).astype(np.float32)
    pos = rng.uniform(-0.002, 0.002, (B, n_cables)).astype(np.float32)
    out = []
    # first generation; second generation with the role-split two-wave kernel where it applies (FK + TD); second
    # generation with one wave per 64 robots everywhere
    for gen, split in (("1", "1"), ("2", "1"), ("2", "0")):
        monkeypatch.setenv("CDPR_ONESTEP", gen)
        monkeypatch.setenv("CDPR_SPLIT", split)
        e = pkg.Engine(cfg, 0)
        e.set_platform_state(pose7=pose)
        snaps = []
        for script in ((3, None), (14, ("v", vel)), (23, ("p", pos)), (12, ("v", -vel))):
            if script[1] is not None:
                (e.set_velocity_command if script[1][0] == "v" else e.set_position_command)(script[1][1])
            for _ in range(script[0]):
                e.update(1)
            snaps.append(e.raw_state() + e.joint_states() + e.platform_state() + (e.pid_debug(),) + (e.fk_state() if stages & 1 else ()))
        out.append(snaps)
        e.close()
    for other in out[1:]:
        for sa, sb in zip(out[0], other):
            for x, y in zip(sa, sb):
                assert np.array_equal(x, y)


def test_per_robot_command_arrival(pkg, oracle, mapping):
    """cdpr_set_*_command_masked on a handle created with per_robot_commands: half the batch gets a position Joy in
    mid-run while the other half stays in Velocity mode, some robots never hear anything, one group gets both kinds
    before the same update; against the oracle (which is B independent JointForceCalculator sets by construction)."""
    once(mapping)
    B = 300
    rng = np.random.default_rng(31)
    for model, stages in ((pkg.eight_cable_model(), 3), (pkg.cube_model(), 0)):
        n = model.n_cables
        cfg = pkg.Config(model=model, batch=B, stages=stages, perRobotCommands=True)
        eng, ora = pair(pkg, oracle, cfg, perturbed_poses(model, B, rng, 0.03, 0.05))
        groups = rng.integers(0, 4, B)  # 0: silent, 1: velocity only, 2: velocity then position, 3: both at once later
        v1 = rng.uniform(-0.03, 0.03, (B, n)).astype(np.float32)
        p1 = rng.uniform(-0.002, 0.002, (B, n)).astype(np.float32)
        for e in (eng, ora):
            e.update(15)
            assert e.set_velocity_command(v1, mask=(groups == 1) | (groups == 2)) == 0
            e.update(40)
        compare(eng, ora, where="after the masked velocity Joy")
        for e in (eng, ora):
            assert e.set_position_command(p1, mask=(groups == 2)) == 0  # group 2: Velocity -> Position, position Pid reset
            assert e.set_velocity_command(-v1, mask=(groups == 3)) == 0
            assert e.set_position_command(p1[0], mask=(groups == 3)) == 0  # broadcast row; both kinds in one update
            assert e.set_velocity_command(np.zeros(n + 1, np.float32), mask=np.ones(B)) == 1  # wrong length: dropped
            e.update(60)
        compare(eng, ora, where="after the mixed Joys")
        for e in (eng, ora):
            e.set_velocity_command(v1)  # an unmasked Joy addresses every robot
            e.update(30)
        compare(eng, ora, where="after the unmasked Joy")
        eng.close()
    plain = pkg.Engine(pkg.Config(batch=4), 0)
    with pytest.raises(pkg.CdprError):  # a handle without per_robot_commands refuses masks instead of guessing
        plain.set_velocity_command(np.zeros((4, 4), np.float32), mask=np.ones(4))


def test_bound_command_buffers_are_used_in_place(pkg, oracle, mapping):
    """cdpr_bind_*_command_device: the caller's HBM buffer is the latched Joy batch (no copy) on every path that reads a
    command: one-step and fused launches, graph replays, both kinds, switching between bound and copied commands."""
    B = 130
    rng = np.random.default_rng(41)
    cfg = pkg.Config(model=pkg.eight_cable_model(), batch=B, stages=3)
    eng, ora = pair(pkg, oracle, cfg, perturbed_poses(cfg.model, B, rng, 0.03, 0.05))
    v = [rng.uniform(-0.03, 0.03, (B, 8)).astype(np.float32) for _ in range(3)]
    p = rng.uniform(-0.002, 0.002, (B, 8)).astype(np.float32)
    dv = [eng.device_upload(x) for x in v]
    dp_ = eng.device_upload(p)
    eng.update(11), ora.update(11)
    assert eng.bind_velocity_command_device(dv[0], B * 8) == 0 and eng.bind_velocity_command_device(dv[0], 8) == 1
    ora.set_velocity_command(v[0])
    eng.update(30), ora.update(30)
    eng.bind_velocity_command_device(dv[1], B * 8), ora.set_velocity_command(v[1])
    eng.update(60, 10), ora.update(60)  # fused launches read the bound buffer too
    compare(eng, ora, where="bound velocity commands")
    eng.bind_position_command_device(dp_, B * 8), ora.set_position_command(p)
    eng.update(25), ora.update(25)
    eng.set_velocity_command(v[2]), ora.set_velocity_command(v[2])  # a copied command replaces the bound one
    eng.update(25), ora.update(25)
    compare(eng, ora, where="bound position command, then a copied velocity command")
    for d in dv + [dp_]:
        eng.device_free(d)


def test_facade_publishes_every_step_and_wire_states(pkg, oracle, mapping):
    """update(n) = n world iterations = n messages per topic, each the oracle's observables of ITS step (fused launch
    chain + trajectory record on the fast path, single steps on the general path); wireStates events when a cable's
    applied force changes sign."""
    once(mapping)
    for eps in (-0.001, 0.002):  # fast path, general controller path
        cfg = pkg.Config(model=pkg.eight_cable_model(), batch=3, stages=0, velocityEpsilon=eps)
        plug = pkg.CdprGazeboPlugin()
        plug.Load(cfg)
        got = {"joint": [], "platform": [], "wire": []}
        plug.bus.subscribe("jointStates", got["joint"].append)
        plug.bus.subscribe("platformPose", got["platform"].append)
        plug.bus.subscribe("wireStates", got["wire"].append)
        ora = oracle.OracleSim(cfg.to_struct())
        rng = np.random.default_rng(9)
        expected = []
        for k in range(4):
            cmd = rng.uniform(-0.2, 0.2, (3, 8)).astype(np.float32)  # large rates: some cables are asked to push
            plug.bus.publish("jointVelocities", pkg.Joy(axes=cmd))
            ora.set_velocity_command(cmd)
            plug.update(25)
            for _ in range(25):
                ora.update(1)
                expected.append((ora.joint_states()[2].copy(), ora.platform_state()[0].copy()))
        assert len(got["joint"]) == len(got["platform"]) == 99
        for k, (js, ps) in enumerate(zip(got["joint"], got["platform"])):
            oe, op = expected[k + 1]
            assert abs(js.header.stamp - 1e-3 * (k + 1)) < 1e-12 and abs(ps.header.stamp - js.header.stamp) < 1e-15
            assert np.abs(js.effort - oe).max() < TOL["eff"] and np.abs(ps.pose.position - op[:, :3]).max() < TOL["pose"]
        # wire events: exactly the sign changes of the published efforts, cable by cable
        taut = np.stack([m.effort > 0 for m in got["joint"]])
        flips = int((taut[1:] != taut[:-1]).sum())
        assert len(got["wire"]) == flips and flips > 0
        ev = got["wire"][0]
        assert ev.stateChange.key.startswith("cable") and ev.stateChange.value in ("slack", "taut") and 0 <= ev.robot < 3


def test_facade_frame_pose_rotates_gravity_and_composes_world_pose(pkg, mapping):
    """Load(frame_pose=...): the model spawned tilted in the world.  platformPose stays frame-relative (PLG.cpp:262-274),
    the engine sees the world's gravity rotated into the frame, worldPlatformPose() = WorldPose(frame) o platformPose."""
    once(mapping)
    rf = Rotation.from_rotvec([0.35, -0.2, 0.6])
    frame_pose = np.concatenate([[1.0, -2.0, 0.5], rf.as_quat()])
    cfg = pkg.Config(batch=2)
    plug = pkg.CdprGazeboPlugin()
    plug.Load(cfg, frame_pose=frame_pose)
    g_frame = rf.inv().apply([0.0, 0.0, -9.8])
    assert np.allclose(plug.config.gravity, g_frame)
    from dataclasses import replace

    ref = pkg.Engine(replace(cfg, gravity=tuple(g_frame)), 0)
    plug.update(200), ref.update(200)
    assert np.array_equal(plug.engine.platform_state()[0], ref.platform_state()[0])
    pose, _ = plug.engine.platform_state()
    wp, wq = plug.worldPlatformPose()
    assert np.allclose(wp, frame_pose[:3] + rf.apply(pose[:, :3]), atol=1e-6)
    assert np.allclose(np.abs((Rotation.from_quat(wq).inv() * rf * Rotation.from_quat(pose[:, 3:])).magnitude()), 0.0, atol=1e-6)
    # subtracting the frame's world pose again gives back what the topic carries
    back = rf.inv().apply(wp - frame_pose[:3])
    assert np.abs(back - pose[:, :3]).max() < 1e-6


def test_ros_bridge_end_to_end_with_a_fake_rospy(pkg, oracle, monkeypatch, mapping):
    """The rospy node around the real engine: Joys in through ROS subscribers, JointState / PlatformState out through
    ROS publishers, against the oracle."""
    once(mapping)
    import sys

    from fake_ros import install_fake_ros

    from cdpr_simulation_amd.ros_bridge import CdprRosBridge

    log = install_fake_ros(monkeypatch)
    cfg = pkg.Config(batch=1)
    plug = pkg.CdprGazeboPlugin()
    plug.Load(cfg)
    br = CdprRosBridge(plug)
    ora = oracle.OracleSim(cfg.to_struct())
    gen = pkg.stimulus.sine_velocity(4)
    RosJoy = sys.modules["sensor_msgs.msg"].Joy
    for k in range(30):
        cmd = next(gen)
        log["subs"]["jointVelocities"].deliver(RosJoy(axes=[float(v) for v in cmd]))
        ora.set_velocity_command(cmd)
        br.step(10), ora.update(10)
    js = log["pubs"]["jointStates"].sent
    assert len(js) == 299 and js[-1].name == ["cable0", "cable1", "cable2", "cable3"]
    assert np.abs(np.array(js[-1].effort) - ora.joint_states()[2][0]).max() < TOL["eff"]
    ps = log["pubs"]["platformPose"].sent[-1]
    op = ora.platform_state()[0][0]
    assert abs(ps.pose.position.z - op[2]) < TOL["pose"] and abs(ps.pose.orientation.w - op[6]) < TOL["pose"]


@pytest.mark.parametrize("scale", [1.0, 30.0])
def test_lumped_leg_physics_terms(pkg, oracle, mapping, scale):
    """passive joint damping (cube.sdf:396) and the leg links' masses / inertias (cube.sdf:359-382)
    as lumped terms in the world step (PHYS kernels): one-step and fused launches, the general controller path, the MPC
    rollout, 4 / 7 / 8 cables, at the shipped link values and 30x exaggerated, against the oracle."""
    once(mapping)
    from dataclasses import replace

    rng = np.random.default_rng(5)
    lumped = dict(passive_damping=0.01 * scale, leg_inertia=0.004 * scale, cable_axial_mass=0.001 * scale, anchor_point_mass=0.002 * scale,
                  anchor_inertia=0.001 * scale)
    eight = pkg.eight_cable_model()
    seven = replace(eight, frame_anchors=eight.frame_anchors[:7], platform_anchors=eight.platform_anchors[:7])
    for base, stages, eps in ((eight, 3, -0.001), (pkg.cube_model(), 0, -0.001), (seven, 3, -0.001), (eight, 3, 0.002)):
        n = base.n_cables
        model = replace(base, inertia=(0.9, 1.1, 1.0, 0.05, -0.03, 0.02), **lumped)
        B = 150
        cfg = pkg.Config(model=model, batch=B, stages=stages, velocityEpsilon=eps, gravity=(0.3, -0.2, -9.7))
        eng, ora = pair(pkg, oracle, cfg, perturbed_poses(model, B, rng, 0.03, 0.05))
        cmd = rng.uniform(-0.03, 0.03, (B, n)).astype(np.float32)
        eng.update(20), ora.update(20)
        eng.set_velocity_command(cmd), ora.set_velocity_command(cmd)
        eng.update(45), ora.update(45)
        compare(eng, ora, where=f"one-step launches, n={n}, eps={eps}")
        if eps < 0:
            eng.update(40, 10), ora.update(40)
            compare(eng, ora, where=f"fused launches, n={n}")
            if stages == 3 and n == 8:
                cmds = rng.uniform(-0.03, 0.03, (B, 10, 4, n)).astype(np.float32)
                ref = eng.raw_state()[0][:, :3].astype(np.float64) + [0.0, 0.0, 0.01]
                gc, oc = eng.rollout_velocity(cmds, ref), ora.rollout_velocity(cmds, ref)
                assert np.abs(gc - oc).max() < rollout_cost_tol(oc, 1e-6)
        eng.close()
    # the terms change the motion measurably (the test is not vacuous) ...
    a = pkg.Engine(pkg.Config(model=replace(eight, **lumped), batch=4, stages=3), 0)
    b = pkg.Engine(pkg.Config(model=eight, batch=4, stages=3), 0)
    for e in (a, b):
        e.set_velocity_command(np.full((4, 8), 0.03, np.float32))
        e.update(200)
    assert np.abs(a.raw_state()[1] - b.raw_state()[1]).max() > 1e-5 * scale
    # ... and a negative one is refused at create
    with pytest.raises(ValueError):
        pkg.Engine(pkg.Config(model=replace(eight, leg_inertia=-1.0), batch=1), 0)


def test_role_split_kernel_with_optional_terms_and_publish_decimation(pkg, oracle, mapping):
    """The FK + TD one-step path (cdpr_split_kernel) with everything switched on that the headline run leaves off:
    SetForce velocity truncation, unilateral cables, a publish period that decimates the observables, the `pid` topic,
    a batch that is no multiple of 64; against the oracle."""
    once(mapping)
    from dataclasses import replace

    B = 203
    rng = np.random.default_rng(71)
    model = replace(pkg.eight_cable_model(), velocity_limit=0.02, unilateral_cables=True)
    cfg = pkg.Config(model=model, batch=B, stages=3 | pkg._abi.STAGE_PID_DEBUG, publishPeriod=0.0035)
    eng, ora = pair(pkg, oracle, cfg, perturbed_poses(model, B, rng, 0.03, 0.06))
    assert eng.mapping == "lane-per-robot"
    for j in range(6):
        cmd = rng.uniform(-0.08, 0.08, (B, 8)).astype(np.float32)  # fast enough to trip the velocity truncation
        eng.set_velocity_command(cmd), ora.set_velocity_command(cmd)
        for _ in range(3):
            eng.update(7), ora.update(7)
            compare(eng, ora, tol=dict(TOL, eff=5e-2), where=f"command {j}")
            assert np.abs(eng.pid_debug() - ora.pid_debug()).max() < 5e-2
    assert np.abs(eng.raw_state()[0] - ora.raw_state()[0]).max() < TOL["pose"]  # the undecimated state as well
    gt, gf = eng.td_state()
    ot, of = ora.td_state()
    assert np.array_equal(gf, of)


def test_hip_path_against_the_second_derivation_directly(pkg, mapping):
    """Closing the triangle: the HIP engine against tests/second_derivation.py (numpy / scipy, written from the
    reference text, shares no code with the oracle) without the oracle in between.  Config 1's robot under
    sinevelocitytest for 1 s, then a position Joy; and an 8-cable robot with FK + TD off (the second derivation has
    neither).  Centred-time fit in the restatement (= the exact derivative the GPU's FIR computes)."""
    once(mapping)
    import second_derivation as sd

    for model, n in ((pkg.cube_model(), 4), (pkg.eight_cable_model(), 8)):
        cfg = pkg.Config(model=model, batch=1)
        eng = pkg.Engine(cfg, 0)
        bot = sd.SecondRobot(cfg, centred=True)
        gen = pkg.stimulus.sine_velocity(n)
        for k in range(60):
            cmd = next(gen) if k < 45 else np.full(n, 0.002 * (-1) ** k, dtype=np.float32)
            if k < 45:
                eng.set_velocity_command(cmd), bot.set_velocity_command(cmd)
            elif k % 5 == 0:
                eng.set_position_command(cmd), bot.set_position_command(cmd)
            eng.update(10), bot.update(10)
            gp, gt = eng.platform_state()
            gq, gqd, ge = eng.joint_states()
            quat_gap = min(np.abs(gp[0, 3:] - bot.obs["pose"][3:]).max(), np.abs(gp[0, 3:] + bot.obs["pose"][3:]).max())
            assert np.abs(gp[0, :3] - bot.obs["pose"][:3]).max() < TOL["pose"] and quat_gap < TOL["pose"], k
            assert np.abs(gt[0] - bot.obs["twist"]).max() < TOL["twist"] and np.abs(gq[0] - bot.obs["q"]).max() < TOL["q"], k
            assert np.abs(gqd[0] - bot.obs["qd"]).max() < TOL["qd"] and np.abs(ge[0] - bot.obs["effort"]).max() < TOL["eff"], k
        eng.close()


def test_observables_in_one_round_trip_equal_the_separate_getters(pkg, monkeypatch):
    """cdpr_get_observables (one gather launch into a pinned host image + completion word) returns exactly what
    cdpr_get_joint_states and cdpr_get_platform_state return, for ragged batches, both cable counts, under publish
    decimation (as of the last PUBLISHED step), call after call (the completion word's epoch) and with NULL outputs."""
    import ctypes as C

    from cdpr_simulation_amd._native import lib

    for n, batch, stages, period in ((4, 1, 0, 0.0), (8, 333, 3, 0.0), (8, 4097, 3, 0.0025), (4, 70000, 0, 0.0)):
        model = pkg.cube_model() if n == 4 else pkg.eight_cable_model()
        cfg = pkg.Config(model=model, batch=batch, stages=stages)
        cfg.publishPeriod = period
        eng = pkg.Engine(cfg, 0)
        rng = np.random.default_rng(n * 1000 + batch)
        eng.set_velocity_command(rng.uniform(-0.03, 0.03, size=(batch, n)).astype(np.float32))
        for rounds in range(4):
            eng.update(3 + rounds)
            q, qd, e = eng.joint_states()
            p, t = eng.platform_state()
            q2, qd2, e2, p2, t2 = eng.observables()
            for a, b in ((q, q2), (qd, qd2), (e, e2), (p, p2), (t, t2)):
                assert a.shape == b.shape and np.array_equal(a, b)
        only = np.empty((batch, 7), dtype=np.float32)
        null = C.POINTER(C.c_float)()
        assert lib().cdpr_get_observables(eng._h, null, null, null, only.ctypes.data_as(C.POINTER(C.c_float)), null) == 0
        assert np.array_equal(only, p)
        eng.close()


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_random_call_sequences_stay_on_the_oracle(pkg, oracle, mapping, seed):
    """The host-side state machine under random call sequences: commands in either mode at random moments, updates of 1..37
    steps issued one launch per step, fused 2 / 5 / 10 / 20 steps per launch, or as a trajectory record, world resets, state
    writes, reads in between (hipGraph replays, ring position, Pid call counter, mode switches, first-step rules all have to
    survive the mix) — compared with the oracle after every update."""
    rng = np.random.default_rng(500 + seed)
    n = [8, 4, 6, 8][seed]
    model = pkg.cube_model() if n == 4 else pkg.eight_cable_model()
    if n == 6:
        model = pkg.Model(model.frame_anchors[[0, 1, 2, 3, 4, 6]], model.platform_anchors[[0, 1, 2, 3, 4, 6]])
    B = [130, 70, 100, 1][seed]
    stages = {4: 0, 6: 1, 8: 3}[n]  # six cables: FK only (a tension distribution without redundancy is J^-T itself, cond^2 in fp32)
    cfg = pkg.Config(model=model, batch=B, stages=stages)
    eng, ora = pair(pkg, oracle, cfg, perturbed_poses(model, B, rng, 0.02, 0.05))
    total = 0
    for op in range(60):
        kind = rng.choice(["vel", "vel", "pos", "run", "run", "run", "fused", "record", "reset", "state"], p=[0.15, 0.1, 0.08, 0.2, 0.12, 0.1, 0.12, 0.06, 0.03, 0.04])
        where = f"seed {seed} op {op} ({kind}) after {total} steps"
        if kind == "vel":
            c = rng.uniform(-0.03, 0.03, (B, n)).astype(np.float32)
            eng.set_velocity_command(c), ora.set_velocity_command(c)
        elif kind == "pos":
            c = rng.uniform(-0.004, 0.004, (B, n)).astype(np.float32)
            eng.set_position_command(c), ora.set_position_command(c)
        elif kind == "reset":
            eng.reset(), ora.reset()
            total = 0
        elif kind == "state":
            p = perturbed_poses(model, B, rng, 0.02, 0.05).astype(np.float32)
            eng.set_platform_state(pose7=p), ora.set_platform_state(pose7=p.astype(np.float64))
        else:
            k = int(rng.integers(1, 38))
            if kind == "run":
                eng.update(k)
            elif kind == "fused":
                eng.update(k, int(rng.choice([2, 5, 10, 20])))
            else:
                rec = eng.update_record(k, int(rng.choice([1, 4, 10])))
                assert rec["pose"].shape == (k, B, 7)
            ora.update(k)
            total += k
            compare(eng, ora, where=where)
            if kind == "record" and total > k:  # the record's last image is the state the getters report
                assert np.array_equal(rec["pose"][-1], eng.platform_state()[0]), where
    eng.close()


@pytest.mark.parametrize("seed", [0, 1])
def test_random_masked_command_sequences(pkg, oracle, mapping, seed):
    """The per-robot path (per_robot_commands) under random sequences: Joys of either kind reach random subsets of the
    robots at random moments (also both kinds before one update, also nobody), resets in between — against the oracle,
    which is B independent JointForceCalculator sets by construction."""
    once(mapping)
    rng = np.random.default_rng(700 + seed)
    model = [pkg.eight_cable_model(), pkg.cube_model()][seed]
    n, B = model.n_cables, [193, 65][seed]
    cfg = pkg.Config(model=model, batch=B, stages=[3, 0][seed], perRobotCommands=True)
    eng, ora = pair(pkg, oracle, cfg, perturbed_poses(model, B, rng, 0.02, 0.05))
    total = 0
    for op in range(50):
        kind = rng.choice(["vel", "pos", "both", "run", "reset"], p=[0.25, 0.15, 0.1, 0.46, 0.04])
        if kind in ("vel", "both"):
            c = rng.uniform(-0.03, 0.03, (B, n)).astype(np.float32)
            m = rng.random(B) < rng.choice([0.0, 0.3, 0.7, 1.0])
            assert eng.set_velocity_command(c, mask=m) == 0 and ora.set_velocity_command(c, mask=m) == 0
        if kind in ("pos", "both"):
            c = rng.uniform(-0.003, 0.003, (B, n)).astype(np.float32)
            m = rng.random(B) < rng.choice([0.0, 0.3, 0.7, 1.0])
            assert eng.set_position_command(c, mask=m) == 0 and ora.set_position_command(c, mask=m) == 0
        if kind == "reset":
            eng.reset(), ora.reset()
            total = 0
        if kind == "run":
            k = int(rng.integers(1, 30))
            eng.update(k), ora.update(k)
            total += k
            compare(eng, ora, where=f"seed {seed} op {op} after {total} steps")
    eng.close()


def test_host_commands_upload_while_earlier_launches_run(pkg, oracle, mapping):
    """cdpr_set_*_command with a host pointer returns without waiting for the launches in flight (pinned staging + a copy
    stream + events): a caller that never synchronises — new Joy batch, ten steps, new Joy batch, ... — must still see
    every batch latched at exactly its update, whatever overtakes whatever; both kinds, broadcast rows, two commands
    before one update, a reset in the middle; against the oracle."""
    rng = np.random.default_rng(77)
    for n, B, stages in ((8, 4096, 3), (4, 777, 0)):
        model = pkg.cube_model() if n == 4 else pkg.eight_cable_model()
        cfg = pkg.Config(model=model, batch=B, stages=stages)
        eng, ora = pair(pkg, oracle, cfg, perturbed_poses(model, B, rng, 0.02, 0.04))
        scratch = np.empty((B, n), dtype=np.float32)  # ONE host buffer, overwritten right after every call
        for period in range(60):
            kind = "pos" if period % 7 == 5 else "vel"
            c = (rng.uniform(-0.03, 0.03, (B, n)) * (0.1 if kind == "pos" else 1.0)).astype(np.float32)
            scratch[:] = c
            if period % 11 == 3:  # a broadcast row
                row = c[0].copy()
                (eng.set_velocity_command if kind == "vel" else eng.set_position_command)(row)
                (ora.set_velocity_command if kind == "vel" else ora.set_position_command)(row)
            else:
                (eng.set_velocity_command if kind == "vel" else eng.set_position_command)(scratch)
                (ora.set_velocity_command if kind == "vel" else ora.set_position_command)(c)
            scratch[:] = np.nan  # the library must not read the caller's buffer after the call returned
            if period % 13 == 6:  # a second Joy of the same kind before the update: the later one wins (PLG.cpp:69,78)
                c2 = rng.uniform(-0.02, 0.02, (B, n)).astype(np.float32)
                scratch[:] = c2
                eng.set_velocity_command(scratch), ora.set_velocity_command(c2)
                scratch[:] = np.nan
            k = int(rng.integers(1, 15))
            eng.update(k), ora.update(k)  # no synchronisation: the host runs ahead of the device
            if period == 30:
                eng.reset(), ora.reset()
        compare(eng, ora, where=f"n={n} after 60 unsynchronised periods")
        eng.close()


def test_mixed_host_and_device_commands_with_long_updates_in_flight(pkg, oracle, mapping):
    """the host-batch double buffer under commands that arrive by DIFFERENT routes.  Host Joy A, a long
    update (thousands of launches in flight reading A), a Joy staged from a DEVICE buffer and latched (the buffers swap:
    the one holding A becomes the pending one), then host Joy C at once: its copy travels on the copy stream and must wait
    for the launches that still read A.  A stale 'buffer is free' event lets C land early and those steps silently run
    under C.  Large batch + long update so that the device is far behind the host; the oracle sees the Joys in order."""
    B, n = 32768, 8
    rng = np.random.default_rng(91)
    model = pkg.eight_cable_model()
    cfg = pkg.Config(model=model, batch=B, stages=3)
    pose = perturbed_poses(model, B, rng, 0.02, 0.04).astype(np.float32)
    eng = pkg.Engine(cfg, 0)
    eng.set_platform_state(pose7=pose)
    a, b, c = (rng.uniform(-0.01, 0.01, (B, n)).astype(np.float32) for _ in range(3))
    d_b = eng.device_upload(b)
    script = []
    for rep in range(3):  # the third round starts from a swapped pair of buffers
        eng.set_velocity_command(a)           # host route (copy stream)
        eng.update(1500)                      # far ahead of the device: ~12 ms of launches queued
        eng.set_velocity_command_device(d_b, B * n)  # device route: staged on the compute stream
        eng.update(7)                         # latches B: the buffer that held A is the pending one now
        eng.set_velocity_command(c)           # host route again, right away
        eng.update(5)
        script += [(1500, a), (7, b), (5, c)]
        a, c = c * np.float32(0.5), a
    got = eng.platform_state() + eng.joint_states()
    for sl in (slice(0, 64), slice(B - 64, B)):
        check_slice(pkg, oracle, dict(model=model, stages=3), sl, pose, script, got, tol=dict(TOL, pose=3e-5, q=3e-5))
    eng.device_free(d_b)
    eng.close()
    # per-robot handle: the latch KERNEL reads the pending buffer; a host Joy right behind it must wait for that read
    once_B = 20000
    cfg2 = pkg.Config(model=pkg.cube_model(), batch=once_B, perRobotCommands=True)
    pose2 = perturbed_poses(cfg2.model, once_B, rng, 0.02, 0.04).astype(np.float32)
    e2, o2 = pkg.Engine(cfg2, 0), oracle.OracleSim(pkg.Config(model=pkg.cube_model(), batch=64, perRobotCommands=True).to_struct(), oracle.DERIV_EXACT)
    e2.set_platform_state(pose7=pose2), o2.set_platform_state(pose7=pose2[:64].astype(np.float64))
    v = [rng.uniform(-0.03, 0.03, (once_B, 4)).astype(np.float32) for _ in range(6)]
    for j in range(6):
        e2.set_velocity_command(v[j]), o2.set_velocity_command(v[j][:64])
        e2.update(40), o2.update(40)  # no synchronisation in between
    gp, _ = e2.platform_state()
    ge = e2.joint_states()[2]
    assert np.abs(gp[:64] - o2.platform_state()[0]).max() <= TOL["pose"] and np.abs(ge[:64] - o2.joint_states()[2]).max() <= TOL["eff"]
    e2.close()


def test_rollout_launch_and_fetch_guard_their_order(pkg, mapping):
    """a second rollout_launch before the fetch must not leak the first one's buffer, a fetch with
    nothing pending says so, and rollout_discard drops a launched rollout."""
    once(mapping)
    B = 16
    eng = pkg.Engine(pkg.Config(model=pkg.eight_cable_model(), batch=B, stages=3), 0)
    cmds = np.zeros((B, 4, 3, 8), dtype=np.float32)
    ref = np.zeros((B, 3), dtype=np.float32)
    with pytest.raises(RuntimeError):
        eng.rollout_fetch()
    eng.rollout_launch(cmds, ref)
    with pytest.raises(RuntimeError):
        eng.rollout_launch(cmds, ref)
    cost = eng.rollout_fetch()
    assert cost.shape == (B, 3)
    eng.rollout_launch(cmds, ref)
    eng.rollout_discard()
    eng.rollout_launch(cmds, ref)
    assert np.array_equal(eng.rollout_fetch(), cost)
    eng.close()


def test_per_robot_handle_is_bit_identical_to_the_uniform_one_when_every_robot_hears_every_joy(pkg, oracle, mapping):
    """Per-robot handles run on the same register-resident kernels as uniform ones (PR instantiations: mode and Pid call
    count per lane).  When every Joy reaches every robot the two must agree BIT FOR BIT — one-step launches (role-split
    kernel at n = 8 with FK + TD, first-generation kernel otherwise), fused launches, the trajectory record, the MPC
    rollout — through mode switches in both directions and both kinds in one update."""
    once(mapping)
    rng = np.random.default_rng(53)
    for model, stages, B in ((pkg.eight_cable_model(), 3, 200), (pkg.cube_model(), 0, 130), (pkg.eight_cable_model(), 1, 70)):
        n = model.n_cables
        pose = perturbed_poses(model, B, rng, 0.03, 0.05).astype(np.float32)
        uni = pkg.Engine(pkg.Config(model=model, batch=B, stages=stages), 0)
        per = pkg.Engine(pkg.Config(model=model, batch=B, stages=stages, perRobotCommands=True), 0)
        v = [rng.uniform(-0.03, 0.03, (B, n)).astype(np.float32) for _ in range(3)]
        p = [rng.uniform(-0.003, 0.003, (B, n)).astype(np.float32) for _ in range(2)]
        everyone = np.ones(B, dtype=np.uint8)
        for e in (uni, per):
            e.set_platform_state(pose7=pose)
            e.update(13)
        def both(name, arr, masked):
            getattr(uni, name)(arr)
            getattr(per, name)(arr, mask=everyone) if masked else getattr(per, name)(arr)
        def same(where):
            for x, y in zip(uni.raw_state() + uni.joint_states() + uni.platform_state(), per.raw_state() + per.joint_states() + per.platform_state()):
                assert np.array_equal(x, y), where
        both("set_velocity_command", v[0], True)
        uni.update(37), per.update(37)
        same("velocity Joy, one-step launches")
        both("set_position_command", p[0], False)
        uni.update(30, 10), per.update(30, 10)
        same("position Joy, fused launches")
        both("set_velocity_command", v[1], True)
        both("set_position_command", p[1], True)  # both kinds before one update: velocity first, then position (PLG.cpp:206-219)
        uni.update(12), per.update(12)
        same("both kinds in one update")
        both("set_velocity_command", v[2], False)
        ru, rp = uni.update_record(24, 8), per.update_record(24, 8)
        for k in ru:
            assert np.array_equal(ru[k], rp[k]), f"trajectory record {k}"
        same("trajectory record")
        cmds = rng.uniform(-0.03, 0.03, (B, 9, 5, n)).astype(np.float32)
        ref = pose[:, :3] + np.float32([0.0, 0.0, 0.01])
        assert np.array_equal(uni.rollout_velocity(cmds, ref), per.rollout_velocity(cmds, ref))
        both("set_position_command", p[0], True)
        uni.update(5), per.update(5)
        assert np.array_equal(uni.rollout_velocity(cmds, ref), per.rollout_velocity(cmds, ref))  # rollout entered from Position mode
        uni.close(), per.close()


@pytest.mark.parametrize("nbuf,deg", [(3, 1), (4, 1), (5, 1)])
def test_per_robot_short_windows_with_staggered_resets(pkg, oracle, mapping, nbuf, deg):
    """Per-robot handle on the register-resident path with a SHORT derivative window (the ring still has kWin slots):
    groups of robots have their Pids reset at staggered steps (a Joy on the other topic), fewer than nbuf steps apart, so
    every reset Pid starts with stale samples of the other Pid in the ring slots it has not refilled yet.  The kernels
    never clear the ring on reset and rely on full = calls >= nbuf to hide those slots: any stale slot leaking into a
    derivative shows up against the oracle (B independent JointForceCalculator sets), which starts every reset window
    empty.  (Degree 1: with 4 - 5 samples and degree 2 the D term's noise gain makes the loop amplify fp32 rounding
    threefold per step for a few steps - the register-resident and the general path then both leave the oracle by ~2 N at
    the same steps, which says nothing about stale slots.)"""
    once(mapping)
    rng = np.random.default_rng(300 + nbuf)
    B, n = 192, 8
    model = pkg.eight_cable_model()
    cfg = pkg.Config(model=model, batch=B, stages=3, perRobotCommands=True)
    for c in (cfg.velocityController, cfg.positionController):
        c.dBufferLength, c.dDegree = nbuf, deg
    eng, ora = pair(pkg, oracle, cfg, perturbed_poses(model, B, rng, 0.03, 0.05))
    # (shipped velocityEpsilon < 0, one window for both Pids, <= 11 samples: the register-resident per-robot kernels)
    grp = rng.integers(0, 4, B)
    v = rng.uniform(0.004, 0.03, (B, n)).astype(np.float32) * rng.choice([-1.0, 1.0], (B, n)).astype(np.float32)
    p = rng.uniform(-0.003, 0.003, (B, n)).astype(np.float32)
    # a short end-point derivative amplifies the fp32 rounding of the errors more than the shipped 11-sample, degree-2 one,
    # and the loop feeds it back: tolerances scale with the RMS gain of the weights (x 0.9 - 2 here, doubled for the
    # feedback).  A stale ring slot (an error of the OTHER Pid, ~3e-3, in a derivative over 1 ms) moves the effort by newtons.
    def rms_gain(nb, dg):
        x = np.arange(nb) - (nb - 1.0)
        return float(np.sqrt((np.linalg.pinv(np.vander(x, dg + 1, increasing=True))[1] ** 2).sum()))
    scale = max(1.0, 2.0 * rms_gain(nbuf, deg) / rms_gain(11, 2))
    tol = {k: scale * t for k, t in TOL.items()}
    for e in (eng, ora):
        e.update(7)
    for rnd in range(6):
        for g in range(4):  # group g switches topic (= resets the Pid it switches to) 1, 2 or nbuf - 1 steps after group g - 1
            to_velocity = (rnd + g) % 2 == 0
            for e in (eng, ora):
                if to_velocity:
                    e.set_velocity_command(v if rnd % 3 else -v, mask=grp == g)
                else:
                    e.set_position_command(p * np.float32(1 + rnd), mask=grp == g)
            k = [1, 2, nbuf - 1, 1][g]
            eng.update(k, k if rnd % 2 else 1), ora.update(k)  # fused and one-step launches alternate
            compare(eng, ora, tol, where=f"nbuf={nbuf} round {rnd} group {g}")
        eng.update(nbuf + 2), ora.update(nbuf + 2)
        compare(eng, ora, tol, where=f"nbuf={nbuf} round {rnd} settled")


@pytest.mark.parametrize("kind", ["fast", "general"])
def test_per_robot_rollout_record_and_fused_updates_against_the_oracle(pkg, oracle, mapping, kind):
    """What per-robot handles gained with the register-resident path: fused launches, the trajectory record and the MPC
    rollout, with robots in DIFFERENT modes and with Pids reset at different times — against the oracle (B independent
    JointForceCalculator sets).  `general`: the same Joy sequence on a handle that still takes the general controller
    path (velocityEpsilon = 0 keeps the hold branch formally alive), one-step updates only."""
    once(mapping)
    rng = np.random.default_rng(59)
    B, n = 150, 8
    model = pkg.eight_cable_model()
    cfg = pkg.Config(model=model, batch=B, stages=3, perRobotCommands=True, **({"velocityEpsilon": 0.0} if kind == "general" else {}))
    eng, ora = pair(pkg, oracle, cfg, perturbed_poses(model, B, rng, 0.03, 0.05))
    grp = rng.integers(0, 3, B)
    v = rng.uniform(0.004, 0.03, (B, n)).astype(np.float32) * rng.choice([-1.0, 1.0], (B, n)).astype(np.float32)  # |v| > eps: no hold branch
    p = rng.uniform(-0.003, 0.003, (B, n)).astype(np.float32)
    spl = 10 if kind == "fast" else 1
    for e in (eng, ora):
        e.update(9)
        e.set_velocity_command(v, mask=grp >= 1)
    eng.update(23, spl), ora.update(23)
    compare(eng, ora, where=f"{kind}: masked velocity Joy, fused")
    for e in (eng, ora):
        e.set_position_command(p, mask=grp == 2)   # group 2 back to Position: its Pid restarts 23 steps after group 1's
        e.set_velocity_command(-v, mask=grp == 0)  # group 0 hears its first Joy now
    eng.update(31, spl), ora.update(31)
    compare(eng, ora, where=f"{kind}: mixed modes, fused")
    if kind == "general":
        return
    rec = eng.update_record(17, 6)
    ora.update(17)
    compare(eng, ora, where="trajectory record")
    assert np.array_equal(rec["pose"][-1], eng.platform_state()[0])
    cmds = rng.uniform(-0.03, 0.03, (B, 12, 4, n)).astype(np.float32)
    ref = (eng.platform_state()[0][:, :3] + np.float32([0.0, 0.0, 0.01])).astype(np.float32)
    gc, oc = eng.rollout_velocity(cmds, ref), ora.rollout_velocity(cmds, ref.astype(np.float64))
    assert np.abs(gc - oc).max() < rollout_cost_tol(oc, 1e-6)
    eng.update(3), ora.update(3)  # the rollout left the handle's own state alone
    compare(eng, ora, where="after the rollout")


@pytest.mark.parametrize("case", ["split", "onestep", "fused", "general", "four_cable"])
def test_travel_limit_flags_against_the_oracle(pkg, oracle, mapping, case):
    """Prismatic travel limits (cube.sdf:436-437) as per-cable flags in the observables, on every kernel family that
    publishes: role-split (FK + TD, n = 8), second-generation one-step (FK only), first-generation fused, the general
    path's platform kernel, and the shipped 4-cable robot.  A geometry that reaches the limits: +-4 mm."""
    once(mapping)
    rng = np.random.default_rng(61)
    four = case == "four_cable"
    model = pkg.cube_model() if four else pkg.eight_cable_model()
    model.travel_lower, model.travel_upper = -0.004, 0.004
    n, B = model.n_cables, 150
    kw = {"split": dict(stages=3), "onestep": dict(stages=1), "fused": dict(stages=3), "general": dict(stages=3, velocityEpsilon=0.0), "four_cable": {}}[case]
    cfg = pkg.Config(model=model, batch=B, **kw)
    eng, ora = pair(pkg, oracle, cfg, perturbed_poses(model, B, rng, 0.002, 0.01))
    jac = oracle.ik(cfg.to_struct(), model.home_pose())[3]
    tw = np.concatenate([rng.uniform(-0.05, 0.05, (B, 3)), rng.uniform(-0.2, 0.2, (B, 3))], axis=1)
    cmd = (-(jac @ tw.T).T).astype(np.float32)
    cmd[np.abs(cmd) < 1e-4] = 1e-4  # |v| > eps on the general path: no hold branch
    spl = 10 if case == "fused" else 1
    seen = np.zeros(B, dtype=np.uint32)
    for e in (eng, ora):
        e.update(10)
        e.set_velocity_command(cmd)
    for k in range(12):
        eng.update(20, spl), ora.update(20)
        gm, om = eng.limit_state(), ora.limit_state()
        q = ora.joint_states()[0]
        near = (np.abs(np.abs(q) - 0.004) < 2e-5).any(axis=1)  # fp32 vs fp64 may disagree on a joint that sits ON a limit
        assert np.array_equal(gm[~near], om[~near]), f"{case}: limit masks differ after {10 + 20 * (k + 1)} steps"
        seen |= gm
        if case in ("split", "fused", "general"):
            assert np.array_equal(eng.td_state()[1], ora.td_state()[1])  # the tension-distribution flag shares the component
    compare(eng, ora, where=case)
    assert (seen != 0).mean() > 0.5 and (seen == 0).any()  # most robots reached a limit, some never did
    plain = pkg.Engine(pkg.Config(model=pkg.cube_model() if four else pkg.eight_cable_model(), batch=4, **kw), 0)
    plain.update(30)
    assert np.all(plain.limit_state() == 0)


@pytest.mark.parametrize("lumped", [False, True])
def test_travel_stop_against_the_oracle(pkg, oracle, mapping, lumped):
    """The inelastic joint stop (cdpr_config_t.travel_stop sweeps) in the PHYS instantiations, alone and together with
    the lumped-leg terms.  A stop is a threshold: fp32 and fp64 may see a joint reach its limit one step apart; for that
    step the two differ by the rate the stop takes away, and the joint then rests one step's travel from where the other
    precision holds it - and which joints rest where shapes everything after.  So the oracle comparison covers the
    first contacts (most robots still bit-for-tolerance alike, every robot within one step of slip); after that the
    check is physical (joints within one step's travel of their limits, flags raised) and structural: fused launches
    are bit-identical to one-step launches."""
    once(mapping)
    rng = np.random.default_rng(67)
    model = pkg.eight_cable_model()
    model.travel_lower, model.travel_upper, model.travel_stop = -0.004, 0.004, 4
    if lumped:
        model.passive_damping, model.leg_inertia, model.cable_axial_mass, model.anchor_point_mass, model.anchor_inertia = 0.01, 0.004, 0.001, 0.002, 0.001
    B = 120
    cfg = pkg.Config(model=model, batch=B, stages=3)
    pose = perturbed_poses(model, B, rng, 0.002, 0.01)
    eng, ora = pair(pkg, oracle, cfg, pose)
    fused = pkg.Engine(cfg, 0)
    fused.set_platform_state(pose7=pose.astype(np.float32))
    jac = oracle.ik(cfg.to_struct(), model.home_pose())[3]
    tw = np.concatenate([rng.uniform(-0.05, 0.05, (B, 3)), rng.uniform(-0.2, 0.2, (B, 3))], axis=1)
    cmd = (-(jac @ tw.T).T).astype(np.float32)
    for e in (eng, ora, fused):
        e.update(10)
        e.set_velocity_command(cmd)
    tight = dict(TOL, eff=5e-2)
    slip = {"pose": 3e-4, "twist": 0.1, "q": 3e-4, "qd": 0.1, "eff": 25.0}  # one step of travel at <= 0.1 m/s, the rate itself, the Pid's answer to it
    for k in range(6):  # 120 steps: the first joints reach their stops after ~60
        eng.update(20), ora.update(20)
        got = eng.platform_state() + eng.joint_states()
        ref = ora.platform_state() + ora.joint_states()
        ok = np.ones(B, dtype=bool)
        for name, g, o in zip(("pose", "twist", "q", "qd", "eff"), got, ref):
            err = np.abs(g - o).max(axis=1)
            assert np.isfinite(g).all() and err.max() <= slip[name], f"lumped={lumped}, {20 * (k + 1)} steps: {name} off by {err.max():.3e}"
            ok &= err <= tight[name]
        assert ok.mean() >= 0.7, f"lumped={lumped}, {20 * (k + 1)} steps: only {ok.mean():.2f} of the robots within the tight tolerances"
    assert (eng.limit_state() != 0).mean() > 0.3  # the stops are in play
    fused.update(120, 10)
    eng.update(180), fused.update(180, 10)
    for x, y in zip(eng.raw_state() + eng.joint_states(), fused.raw_state() + fused.joint_states()):
        assert np.array_equal(x, y)
    for sim in (eng, ora):
        q = sim.joint_states()[0]
        assert np.abs(q).max() < 0.004 + 1.5e-4 and (np.abs(q) > 0.004 - 1e-5).any()
    assert (eng.limit_state() != 0).any()
    # the same Joys without the stop carry the joints far beyond
    free = pkg.eight_cable_model()
    free.travel_lower, free.travel_upper = -0.004, 0.004
    e3 = pkg.Engine(pkg.Config(model=free, batch=B, stages=3), 0)
    e3.set_platform_state(pose7=pose.astype(np.float32))
    e3.update(10), e3.set_velocity_command(cmd), e3.update(300)
    assert np.abs(e3.joint_states()[0]).max() > 0.008


def test_cable_mapping_runs_on_the_same_state_as_the_others(pkg, oracle, mapping):
    """The three mappings share one HBM layout: the lane-per-cable kernel reads the ring rows of a cable PAIR and writes
    single dwords into them.  Odd cable counts (masked lanes, padding components of the joint rows), travel-limit flags,
    one-step and fused launches, against the oracle."""
    if mapping != "lane_per_cable":
        pytest.skip("lane-per-cable only")
    rng = np.random.default_rng(71)
    full = pkg.eight_cable_model()
    for keep, stages in (([0, 1, 2, 3, 4, 6], 1), ([0, 1, 2, 3, 4, 5, 6], 3), (list(range(8)), 3), ([0, 1, 2], 0), ([0, 1, 2, 3, 4], 0)):
        m = pkg.Model(full.frame_anchors[keep], full.platform_anchors[keep])
        m.travel_lower, m.travel_upper = -0.003, 0.003
        B, n = 77, len(keep)
        cfg = pkg.Config(model=m, batch=B, stages=stages)
        eng, ora = pair(pkg, oracle, cfg, perturbed_poses(m, B, rng, 0.01, 0.03))
        assert eng.mapping == "lane-per-cable"
        eng.update(40), ora.update(40)
        cmd = rng.uniform(-0.02, 0.02, (B, n)).astype(np.float32)
        eng.set_velocity_command(cmd), ora.set_velocity_command(cmd)
        eng.update(90), ora.update(90)
        compare(eng, ora, where=f"lane-per-cable, n={n}, stages={stages}")
        q = ora.joint_states()[0]
        near = (np.abs(np.abs(q) - 0.003) < 2e-5).any(axis=1)
        assert np.array_equal(eng.limit_state()[~near], ora.limit_state()[~near])
        eng.update(30, 10), ora.update(30)
        compare(eng, ora, where=f"lane-per-cable fused, n={n}")
        eng.close()


def test_c_example_matches_the_python_host(pkg, mapping, tmp_path):
    """examples/c_abi_demo.c (plain C99 against include/cdpr.h: config filled field by field, sine Joy, cdpr_update,
    cdpr_get_observables) prints what the Python host gets from the same calls."""
    once(mapping)
    import os
    import subprocess

    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "c_abi_demo"
    libdir = os.path.join(ROOT, "cdpr-simulation_amd")
    r = subprocess.run(["gcc", "-std=c99", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_abi_demo.c"), "-L" + libdir,
                        "-lcdpr_hip", "-lm", "-Wl,-rpath," + libdir, "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe), "3"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.strip().splitlines()
    assert len(lines) == 6 and lines[-1].startswith("t =  3.00 s")
    eng = pkg.Engine(pkg.Config(batch=3), 0)
    for k in range(300):
        eng.set_velocity_command(np.full(4, np.float32(0.05 * np.sin(2.0 * np.pi * 0.1 * (k * 0.01))), dtype=np.float32))
        eng.update(10)
    q, qd, eff, pose, twist = eng.observables()
    words = lines[-1].replace("=", " ").split()
    z, vz, q0, f0 = float(words[words.index("z") + 1]), float(words[words.index("vz") + 1]), float(words[words.index("q") + 1]), float(words[words.index("F") + 1])
    assert abs(z - pose[0, 2]) < 2e-6 and abs(vz - twist[0, 2]) < 2e-6 and abs(q0 - q[0, 0]) < 2e-6 and abs(f0 - eff[0, 0]) < 2e-4
