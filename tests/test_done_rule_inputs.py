"""Done rules, the CPU side: the ABI's new struct and symbols, the sharded wrapper, and the conditions on the reference predicate and
on the oracle that tests/test_gpu_done.py relies on (scenarios and predicate: tests/done_rules.py).

  1. cdpr_done_rule_size() is the ctypes mirror's sizeof, the ABI is version 8, a NULL handle is refused without a GPU.
  2. ShardedEngine.evaluate_done concatenates masks and reasons in shard_range order and sums the counts; reset_done_device hands
     every shard its own pointers (stub engines, no GPU).
  3. The static scenario, on the reference alone: every reason bit it enables fires for at least 3 robots and stays clear for at
     least 3, some robot carries two bits, robots on the box are inside and one value past it outside (float32 and float64), and no
     tilt / speed / rate metric lies within 1e-5 relative of its threshold.
  4. The closed loop, on the oracle alone (ri.oracle_reset driven by done_reference): resets happen at 3 or more of the 8 evaluation
     points and, at every evaluation point, no robot's metric lies within 100 x the parity tolerance of that quantity of its threshold
     - the condition under which an fp32 engine within TOL of the oracle, and an fp64 engine within TOL64, must take the oracle's
     decisions.  No robot is left out.
"""
import ctypes as C

import numpy as np
import pytest

import done_rules as dr
import robot_histories as ri
from parity import TOL, TOL64

B = dr.B


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
def test_rule_struct_and_abi_version(pkg):
    from cdpr_simulation_amd._native import lib

    assert lib().cdpr_done_rule_size() == C.sizeof(pkg._abi.DoneRuleStruct) == 56
    assert lib().cdpr_abi_version() == 8 == pkg._abi.ABI_VERSION
    s = pkg.DoneRule().to_struct()
    assert s.struct_size == 56 and s.enable == 0  # the defaults enable nothing
    assert [getattr(pkg._abi, "DONE_" + n.upper()) for n in dr.BIT_NAMES] == [1 << k for k in range(9)] and pkg._abi.DONE_COUNTS == dr.COUNTS


def test_a_null_handle_is_refused_without_a_gpu(pkg):
    from cdpr_simulation_amd._native import lib

    rule = pkg.DoneRule(enable=dr.WORKSPACE).to_struct()
    mask, words = np.zeros(4, np.uint8), np.zeros(16, np.uint32)
    u8, u32 = mask.ctypes.data_as(C.POINTER(C.c_uint8)), words.ctypes.data_as(C.POINTER(C.c_uint32))
    assert lib().cdpr_evaluate_done(None, C.byref(rule), u8, u32, u32) == pkg._abi.ERR_INVALID
    assert lib().cdpr_evaluate_done_device(None, C.byref(rule), None, None, None) == pkg._abi.ERR_INVALID
    assert lib().cdpr_reset_done_device(None, C.byref(rule), None, None, None) == pkg._abi.ERR_INVALID
    assert lib().cdpr_get_episode_start(None, u32) == pkg._abi.ERR_INVALID
    assert not mask.any() and not words.any()


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
class StubEngine:
    def __init__(self, lo, hi, rng):
        n = hi - lo
        self.reason = rng.integers(0, 1 << 9, n).astype(np.uint32) * (rng.random(n) < 0.4)
        self.reason = self.reason.astype(np.uint32)
        self.start = rng.integers(0, 1000, n).astype(np.uint32)
        self.calls = []

    def evaluate_done(self, rule):
        counts = np.zeros(dr.COUNTS, np.uint32)
        counts[0] = (self.reason != 0).sum()
        for k in range(dr.COUNTS - 1):
            counts[1 + k] = ((self.reason >> np.uint32(k)) & np.uint32(1)).sum()
        return (self.reason != 0).astype(np.uint8), self.reason, counts

    def reset_done_device(self, rule, d_pose7=0, d_twist6=0, d_counts=0):
        self.calls.append((rule, d_pose7, d_twist6, d_counts))

    def episode_start(self):
        return self.start


@pytest.mark.parametrize("devices", [1, 3, 4])
def test_sharded_evaluate_done_slices_and_sums_by_shard_range(pkg, devices):
    from cdpr_simulation_amd.sharding import ShardedEngine, shard_range

    rng = np.random.default_rng(6)
    sh = object.__new__(ShardedEngine)  # (no GPU: the per-device engines are stubs)
    sh.B, sh.n = B, 8
    sh.spans = [shard_range(i, devices, B) for i in range(devices)]
    sh.engines = [StubEngine(lo, hi, rng) for lo, hi in sh.spans]
    rule = pkg.DoneRule(enable=0x1FF)
    mask, reason, counts = sh.evaluate_done(rule)
    assert mask.shape == (B,) and mask.dtype == np.uint8 and reason.shape == (B,) and reason.dtype == np.uint32
    assert counts.shape == (dr.COUNTS,) and counts.dtype == np.uint32
    for e, (lo, hi) in zip(sh.engines, sh.spans):
        assert np.array_equal(reason[lo:hi], e.reason) and np.array_equal(mask[lo:hi], (e.reason != 0).astype(np.uint8))
        assert np.array_equal(sh.episode_start()[lo:hi], e.start)
    assert counts[0] == (reason != 0).sum() and counts[0] > 0
    for k in range(dr.COUNTS - 1):
        assert counts[1 + k] == ((reason >> np.uint32(k)) & np.uint32(1)).sum()
    # per-shard pointers; None = home pose / zero twist / no counts everywhere
    sh.reset_done_device(rule)
    poses, counts_ptrs = [1000 + i for i in range(devices)], [2000 + i for i in range(devices)]
    sh.reset_done_device(rule, d_pose7=poses, d_counts=counts_ptrs)
    for i, e in enumerate(sh.engines):
        assert e.calls == [(rule, 0, 0, 0), (rule, poses[i], 0, counts_ptrs[i])]
    with pytest.raises(ValueError):
        sh.reset_done_device(rule, d_pose7=[1] * (devices + 1))


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True], ids=["float32", "float64"])
@pytest.mark.parametrize("n", [4, 8, 12])
def test_the_static_scenario_exercises_every_bit(pkg, n, f64):
    model = ri.model_of(pkg, n)
    rule, pose, twist = dr.static_scenario(pkg, model, f64)
    assert pose.dtype == twist.dtype == (np.float64 if f64 else np.float32)
    zero = np.zeros(B, np.uint32)
    mask, reason, counts = dr.done_reference(rule, pose, twist, None, None, None, zero, 0, f64)
    assert np.array_equal(mask, (reason != 0).astype(np.uint8)) and set(np.unique(mask)) == {0, 1}
    assert counts[0] == mask.sum() and not (reason & ~np.uint32(rule.enable)).any()
    for k, name in enumerate(dr.BIT_NAMES):
        fired = int(((reason >> np.uint32(k)) & np.uint32(1)).sum())
        assert counts[1 + k] == fired
        if (rule.enable >> k) & 1:
            assert fired >= 3 and B - fired >= 3, (name, fired)
        else:
            assert fired == 0, name
    assert (np.array([bin(int(r)).count("1") for r in reason]) >= 2).sum() >= 1  # some robot carries two bits
    # on the box: inside; one value past it: outside
    for k in dr.ON_LO + dr.ON_HI:
        assert not reason[k] & dr.WORKSPACE, k
    for k in dr.BELOW_LO + dr.ABOVE_HI:
        assert reason[k] == dr.WORKSPACE, k
    assert reason[dr.NAN_POSITION] == dr.NONFINITE and reason[dr.NAN_QUATERNION] == dr.NONFINITE  # ordinary comparisons are false on NaN
    assert reason[dr.INF_TWIST] == dr.NONFINITE | dr.SPEED and reason[dr.NEG_INF_POSITION] == dr.NONFINITE | dr.WORKSPACE
    for k in dr.TILTED:
        assert reason[k] == dr.TILT, k
    for k in dr.UPRIGHT_SCALED:
        assert reason[k] == 0, k
    for k in dr.FAST_AND_OUT:
        assert reason[k] == dr.SPEED | dr.WORKSPACE, k
    for name, d in dr.metric_margins(rule, pose, twist).items():
        assert d.min() > 1e-5, f"{name}: a robot's metric is within 1e-5 relative of its threshold ({d.min():.3e})"


def test_the_timeout_is_wrap_safe_and_disabled_bits_stay_clear(pkg):
    model = ri.model_of(pkg, 8)
    pose, twist = np.tile(np.asarray(model.home_pose()), (4, 1)), np.zeros((4, 6))
    rule = pkg.DoneRule(enable=dr.TIMEOUT, max_steps=10)  # (the box of the defaults is a point at the origin: WORKSPACE is not enabled)
    start = np.array([0xFFFFFFFB, 0xFFFFFFFC, 5, 6], np.uint32)
    step = (1 << 32) + 5  # low word 5: ages 10, 9, 0 and 2^32 - 1
    _, reason, counts = dr.done_reference(rule, pose, twist, None, None, None, start, step, False)
    assert reason.tolist() == [dr.TIMEOUT, 0, 0, dr.TIMEOUT] and counts[0] == 2 and counts[1 + 8] == 2


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
LOOP_CONFIGS = {  # the three per-robot record layouts of tests/test_gpu_reset_robots.py, as the oracle sees them
    "fast_n8": (dict(stages=3), TOL),
    "general_lean_hot": (dict(stages=3, velocityEpsilon=ri.EPS), TOL),
    "fp64_hold_n8": (dict(stages=3, precision=64, velocityEpsilon=ri.EPS), TOL64),
}


@pytest.mark.parametrize("kind", list(LOOP_CONFIGS))
def test_the_closed_loop_keeps_clear_of_its_thresholds_on_the_oracle(pkg, oracle, kind):
    kw, _ = LOOP_CONFIGS[kind]
    model = ri.model_of(pkg, 8)
    cfg = pkg.Config(model=model, batch=B, perRobotCommands=True, **kw)
    rule = dr.loop_rule(pkg, model)
    h, respawn = dr.loop_inputs(model)
    ora = oracle.OracleSim(cfg.to_struct(), oracle.DERIV_EXACT)
    ora.set_platform_state(pose7=h["pose"].astype(np.float64))
    worst = {}
    seen = []

    def check(j, mask, reason, counts, p, t):
        assert np.isfinite(p).all() and np.isfinite(t).all()
        m = dr.loop_margins(rule, p, t, TOL)  # (TOL is the wider of the two: the condition then holds for the fp64 handles as well)
        for name, v in m.items():
            worst[name] = min(worst.get(name, np.inf), v)
            assert v >= 100.0, f"{kind}, evaluation {j}: a robot's {name} metric is {v:.1f} parity tolerances from its threshold"
        seen.append(counts.copy())

    verdicts = dr.run_loop([], ora, rule, h, respawn, check=check)
    ora.close()
    resets = [int(c[0]) for c in seen]
    print(f"done rules, closed loop on the oracle, {kind}: robots reset per evaluation point {resets}; smallest margins (parity tolerances) "
          + "  ".join(f"{k} {v:.0f}" for k, v in worst.items()))
    assert sum(r > 0 for r in resets) >= 3 and len(verdicts) == dr.LOOP_STEPS // dr.LOOP_EVERY
    total = np.sum(seen, axis=0)
    for bit in (dr.WORKSPACE, dr.TILT, dr.TIMEOUT):  # each of the three live conditions decides somewhere in the loop
        assert total[1 + bit.bit_length() - 1] > 0, bit
    assert total[1 + 0] == 0 and total[1 + 3] == 0  # NONFINITE and SPEED are enabled and stay clear
    assert any(0 < r < B for r in resets)  # ... and it is a choice: some robots, not all
