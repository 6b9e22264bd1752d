"""cdpr_reset_robots, the CPU side: the oracle-side condition of tests/test_gpu_reset_robots.py and the sharded wrapper.

On OracleSim a reset of mask m is the recipe `oracle_reset` of tests/robot_histories.py (the inputs are that module's too).

  1. history independence: two oracles with different 37-step histories (other start poses, other commands, other modes per robot) get
     the recipe with the same mask and poses and then the same commands; the reset robots' pose, twist, q, qdot and effort are EQUAL
     (difference 0.0) at every checkpoint while the other robots differ.  So the recipe leaves nothing of a robot's past behind, which is
     what the engine's reset kernels are compared with.
  2. ShardedEngine.reset_robots slices mask and rows as shard_range says (stub engines, no GPU).
"""
import numpy as np
import pytest

from robot_histories import B, CONFIGS, after_inputs, history_inputs, model_of, oracle_reset, play_after, play_history, reset_mask


@pytest.mark.parametrize("name", list(CONFIGS))
def test_the_recipe_leaves_nothing_of_a_robots_history(pkg, oracle, name):
    n, kw = CONFIGS[name]
    model = model_of(pkg, n)
    cfg = pkg.Config(model=model, batch=B, perRobotCommands=True, **kw)
    sims = [oracle.OracleSim(cfg.to_struct(), oracle.DERIV_EXACT) for _ in range(2)]
    for s, (seed, shift) in zip(sims, ((11, 0), (12, 1))):  # two histories: other poses, other commands, every robot in another mode
        h = history_inputs(model, seed, shift)
        s.set_platform_state(pose7=h["pose"].astype(np.float64))
        play_history([s], h)
    mask = reset_mask()
    m = mask.astype(bool)
    a = after_inputs(model, 13)
    for s in sims:
        oracle_reset(s, mask, a["pose"])
    seen = []

    def check(label):
        xs, ys = (s.platform_state() + s.joint_states() for s in sims)
        for quantity, x, y in zip(("pose", "twist", "q", "qd", "effort"), xs, ys):
            assert np.isfinite(x).all() and np.isfinite(y).all(), (name, label, quantity)
            assert np.array_equal(x[m], y[m]), f"{name}, {label}: {quantity} of the reset robots depends on their history (max difference {np.abs(x[m] - y[m]).max():.3e})"
        seen.append(float(np.abs(xs[0][~m] - ys[0][~m]).max()))

    play_after(sims, a, check)
    assert min(seen) > 1e-3, f"{name}: the two histories do not tell the other robots apart ({seen})"  # (start poses 2 cm apart)
    for s in sims:
        s.close()


def test_recipe_with_home_pose_and_twist(pkg, oracle):
    """pose7 None = the home pose, a twist row is taken as float32; robots outside the mask keep their state to the bit."""
    model = model_of(pkg, 8)
    cfg = pkg.Config(model=model, batch=B, stages=3, perRobotCommands=True)
    ora = oracle.OracleSim(cfg.to_struct(), oracle.DERIV_EXACT)
    h = history_inputs(model, 21)
    ora.set_platform_state(pose7=h["pose"].astype(np.float64))
    play_history([ora], h, 12)
    before = ora.raw_state()
    mask = reset_mask()
    m = mask.astype(bool)
    twist = np.random.default_rng(22).uniform(-0.01, 0.01, (B, 6))
    oracle_reset(ora, mask, None, twist, home=model.home_pose())
    p, t = ora.raw_state()
    assert np.array_equal(p[~m], before[0][~m]) and np.array_equal(t[~m], before[1][~m])
    assert np.array_equal(p[m], np.tile(model.home_pose(), (int(m.sum()), 1))) and np.array_equal(t[m], twist.astype(np.float32).astype(np.float64)[m])
    ora.close()


class StubEngine:
    def __init__(self):
        self.calls = []

    def reset_robots(self, mask, pose7=None, twist6=None):
        self.calls.append((mask, pose7, twist6))


@pytest.mark.parametrize("devices", [1, 3, 4])
def test_sharded_reset_slices_by_shard_range(pkg, devices):
    from cdpr_simulation_amd.sharding import ShardedEngine, shard_range

    sh = object.__new__(ShardedEngine)  # (no GPU: the per-device engines are stubs)
    sh.B, sh.n = B, 8
    sh.spans = [shard_range(i, devices, B) for i in range(devices)]
    sh.engines = [StubEngine() for _ in range(devices)]
    rng = np.random.default_rng(5)
    mask = (rng.random(B) < 0.3).astype(np.uint8)
    pose, twist = rng.uniform(-1, 1, (B, 7)).astype(np.float32), rng.uniform(-1, 1, (B, 6)).astype(np.float32)
    sh.reset_robots(mask, pose, twist)
    sh.reset_robots(mask.astype(bool), pose.ravel())  # a flat pose array, no twist
    sh.reset_robots(mask)
    assert sum(hi - lo for lo, hi in sh.spans) == B
    for e, (lo, hi) in zip(sh.engines, sh.spans):
        assert len(e.calls) == 3
        (m0, p0, t0), (m1, p1, t1), (m2, p2, t2) = e.calls
        for mm in (m0, m1, m2):
            assert mm.dtype == np.uint8 and np.array_equal(mm, mask[lo:hi])
        assert np.array_equal(p0, pose[lo:hi]) and np.array_equal(t0, twist[lo:hi])
        assert np.array_equal(p1, pose[lo:hi]) and t1 is None
        assert p2 is None and t2 is None


def test_a_null_handle_is_refused_without_a_gpu(pkg):
    import ctypes as C

    from cdpr_simulation_amd._native import lib

    mask = np.ones(4, np.uint8)
    assert lib().cdpr_reset_robots(None, mask.ctypes.data_as(C.POINTER(C.c_uint8)), None, None) == pkg._abi.ERR_INVALID
    assert lib().cdpr_reset_robots_device(None, None, None, None) == pkg._abi.ERR_INVALID
