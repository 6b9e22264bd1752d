"""The environment view, the CPU side: the ABI's new struct and symbols, the width arithmetic, the reward's closed forms and the footing
of the tolerance tests/test_gpu_env_view.py compares rewards at (references and scenario: tests/env_view.py).

  1. cdpr_env_spec_size() is the ctypes mirror's sizeof, the ABI number is unchanged, a NULL handle is refused without a GPU.
  2. The packed width for n = 1, 4, 8, 12: every single field, all fields, an unknown bit.
  3. Closed forms: at the target the reward is `alive`; a pure yaw of 0.2 rad gives ori = sin^2(0.1); a weight of exactly 0 hides a NaN,
     a weight that is not shows it.
  4. The bound, on the scenario of the GPU test: the float32 restatement of the formula lies inside 64 * 2^-24 * M of the float64
     reference for every finite robot (so an fp32 handle that computes the formula can meet it), and the bound tells a wrong formula
     from the right one: with two weights swapped, or with the effort term dropped, the reward leaves it for at least half of the
     robots.
  5. ShardedEngine.observe / env_evaluate concatenate in shard_range order and sum the counts (stub engines, no GPU).
"""
import ctypes as C

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import done_rules as dr
import env_view as ev
import robot_histories as ri

B = dr.B


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
def test_spec_struct_and_abi_version(pkg):
    from cdpr_simulation_amd._native import lib

    assert lib().cdpr_env_spec_size() == C.sizeof(pkg._abi.EnvSpec) == 48 + C.sizeof(pkg._abi.DoneRuleStruct)
    assert lib().cdpr_abi_version() == pkg._abi.ABI_VERSION
    s = pkg.EnvSpec()
    assert s.struct_size == C.sizeof(pkg._abi.EnvSpec) and s.fields == 0 and s.done.struct_size == C.sizeof(pkg._abi.DoneRuleStruct) and s.done.enable == 0
    s = pkg.EnvSpec(done=pkg.DoneRule(enable=dr.TILT, min_up=0.5), fields=ev.POSE, w_speed=0.25)
    assert s.done.enable == dr.TILT and s.done.min_up == 0.5 and s.w_speed == 0.25 and s.fields == 1
    assert [getattr(pkg._abi, "OBS_" + n.upper()) for n in ev.FIELD_NAMES] == [1 << k for k in range(8)] and pkg._abi.OBS_ALL == ev.ALL
    assert tuple(pkg._abi.EnvSpec.WEIGHTS) == ev.WEIGHTS


def test_a_null_handle_is_refused_without_a_gpu(pkg):
    from cdpr_simulation_amd._native import lib

    spec = pkg.EnvSpec(fields=ev.POSE)
    w = C.c_uint32(77)
    assert lib().cdpr_observation_width(None, ev.POSE, C.byref(w)) == pkg._abi.ERR_INVALID and w.value == 77
    assert lib().cdpr_observe_device(None, ev.POSE, 0, None, None) == pkg._abi.ERR_INVALID
    assert lib().cdpr_env_evaluate_device(None, C.byref(spec), None, None, None, None, None, None) == pkg._abi.ERR_INVALID


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4, 8, 12])
def test_width_arithmetic(pkg, n):
    for k, w in enumerate(ev.field_widths(n)):
        assert pkg.observation_width(1 << k, n) == w, (n, ev.FIELD_NAMES[k])
    assert pkg.observation_width(ev.ALL, n) == 3 * n + 22 and pkg.observation_width(0, n) == 0
    assert pkg.observation_width(ev.POSE | ev.EFFORT | ev.AGE, n) == 8 + n
    with pytest.raises(ValueError):
        pkg.observation_width(0x100, n)
    # the reference lays the columns out in bit order
    g = dict(pose=np.full((2, 7), 1), twist=np.full((2, 6), 2), joint_position=np.full((2, n), 3), joint_velocity=np.full((2, n), 4), effort=np.full((2, n), 5),
             fk_pose=np.full((2, 7), 6), fk_residual=np.full(2, 7), start=np.array([3, 2 ** 32 - 2 ** 20 + 2], np.uint32), step_count=2 ** 32 + 2)
    g = {k: np.asarray(v, dtype=np.float32) if k not in ("start", "step_count") else v for k, v in g.items()}
    obs = ev.observation_reference(ev.ALL, **g)
    want = sum(([float(k + 1)] * w for k, w in enumerate(ev.field_widths(n)[:7])), [])
    assert obs.shape == (2, 3 * n + 22) and obs[0, :-1].tolist() == want
    assert obs[:, -1].tolist() == [float(2 ** 32), float(2 ** 20)]  # the age wraps with the low word: 2^32 - 1 (rounded to float32) and 2^20


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
def closed_form_inputs(n=8):
    home = np.array([0.125, -0.25, 0.75, 0.0, 0.0, 0.0, 1.0])  # (float32 values: a NULL target is the home pose as a float buffer holds it)
    pose = np.tile(home, (4, 1))
    return home, pose, np.zeros((4, 6)), np.zeros((4, n)), np.zeros(4, np.float32), np.zeros(4, np.uint32)


def test_closed_forms(pkg):
    home, pose, twist, effort, res, reason = closed_form_inputs()
    spec = pkg.EnvSpec(w_position=40.0, w_orientation=3.0, w_speed=0.5, w_rate=0.25, w_effort=0.002, w_fk_residual=7.0, alive=1.5, done_penalty=5.0)
    for fn in (ev.reward_reference, ev.reward_f32):
        # at the target (the home pose, target None): the reward is `alive`, whatever the quaternion's sign and length
        pose[1, 3:] *= -1.0
        pose[2, 3:] *= 2.0
        r = fn(spec, pose, twist, effort, res, reason, None, home)
        r = r[0] if isinstance(r, tuple) else r
        assert np.array_equal(np.asarray(r, dtype=np.float64), np.full(4, 1.5)), fn.__name__
        pose[:, 3:] = home[3:]
    # a pure yaw of 0.2 rad: ori = sin^2(0.1)
    only_ori = pkg.EnvSpec(w_orientation=1.0)
    yaw = pose.copy()
    yaw[:, 3:] = Rotation.from_rotvec([0.0, 0.0, 0.2]).as_quat()
    r, M = ev.reward_reference(only_ori, yaw, twist, effort, res, reason, None, home)
    assert np.allclose(-r, np.sin(0.1) ** 2, rtol=0, atol=1e-15) and np.array_equal(M, np.ones(4))
    assert ev.inside(ev.reward_f32(only_ori, yaw, twist, effort, res, reason, None, home), r, M, False).all()
    # the done penalty reaches the robots with a reason word, and only them
    r, _ = ev.reward_reference(spec, pose, twist, effort, res, np.array([0, 4, 0, 1], np.uint32), None, home)
    assert r.tolist() == [1.5, -3.5, 1.5, -3.5]


def test_a_zero_weight_hides_a_nan(pkg):
    home, pose, twist, effort, res, reason = closed_form_inputs()
    twist[1, 4] = np.nan   # behind w_rate
    effort[2, 3] = np.inf  # behind w_effort
    pose[3, 1] = np.nan    # behind w_position; the quaternion stays finite
    for fn in (ev.reward_reference, ev.reward_f32):
        get = lambda spec: np.asarray((lambda r: r[0] if isinstance(r, tuple) else r)(fn(spec, pose, twist, effort, res, reason, None, home)), dtype=np.float64)  # noqa: E731
        assert np.array_equal(get(pkg.EnvSpec(w_orientation=2.0, w_speed=1.0, alive=1.0)), np.ones(4)), fn.__name__
        r = get(pkg.EnvSpec(w_orientation=2.0, w_rate=1.0, alive=1.0))
        assert np.isnan(r[1]) and np.array_equal(r[[0, 2, 3]], np.ones(3))
        r = get(pkg.EnvSpec(w_effort=1.0, w_position=1.0, alive=1.0))
        assert r[2] == -np.inf and np.isnan(r[3]) and np.array_equal(r[:2], np.ones(2))


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 8, 12])
def test_the_bound_is_reachable_and_tight(pkg, n):
    model = ri.model_of(pkg, n)
    cfg = pkg.Config(model=model, batch=B, stages=3 if n >= 6 else 0)
    rule, weights, pose, twist, target = ev.scenario(pkg, model, False)
    effort, res = ev.stand_in_efforts(n, False)
    if n < 6:
        res = None
    spec = ev.spec_of(pkg, cfg, rule, weights)
    assert len({w for w in ev.weights_of(spec) if w != 0.0}) == (6 if n >= 6 else 5)  # all distinct
    g = dict(pose=pose, twist=twist, fk_residual=res, infeasible=None, limit_mask=None, start=np.zeros(B, np.uint32), step_count=0, f64=False)
    reason = dr.done_reference(rule, **g)[1]
    home = model.home_pose()
    r, M = ev.reward_reference(spec, pose, twist, effort, res, reason, target, home)
    finite = np.isfinite(r)
    assert finite.sum() == B - len(dr.NONFINITE_ROBOTS) and not finite[list(dr.NONFINITE_ROBOTS)].any()
    r32 = ev.reward_f32(spec, pose, twist, effort, res, reason, target, home)
    err = np.abs(r32.astype(np.float64)[finite] - r[finite]) / (2.0 ** -24 * M[finite])
    print(f"env view, n = {n}: the float32 restatement is within {err.max():.2f} x 2^-24 M of the float64 reference (bound 64)")
    assert ev.inside(r32, r, M, False)[finite].all() and np.array_equal(np.isnan(r32), np.isnan(r))
    # the robot at its target: no position or orientation term beyond rounding
    terms = ev.reward_terms(pose, twist, effort, res, target, lambda a, b, c: a * b + c, np.float64)
    assert terms[0][ev.AT_TARGET] == 0.0 and abs(terms[1][ev.AT_TARGET]) < 1e-15
    # a wrong formula leaves the bound: two weights swapped, the effort term dropped
    swapped = ev.spec_of(pkg, cfg, rule, dict(weights, w_speed=weights["w_rate"], w_rate=weights["w_speed"]))
    dropped = ev.spec_of(pkg, cfg, rule, dict(weights, w_effort=0.0))
    other = ev.spec_of(pkg, cfg, rule, dict(weights, w_position=weights["w_orientation"], w_orientation=weights["w_position"]))
    for name, wrong in (("speed and rate swapped", swapped), ("effort dropped", dropped), ("position and orientation swapped", other)):
        out = ~ev.inside(ev.reward_f32(wrong, pose, twist, effort, res, reason, target, home), r, M, False)[finite]
        print(f"env view, n = {n}: {name}: {int(out.sum())} of {int(finite.sum())} robots leave the bound")
        assert out.sum() >= B // 2, name
    # the penalty is visible on exactly the done robots
    free = ev.spec_of(pkg, cfg, rule, weights, done_penalty=0.0)
    diff = ev.reward_reference(free, pose, twist, effort, res, reason, target, home)[0][finite] - r[finite]
    assert np.array_equal(diff != 0.0, (reason != 0)[finite]) and np.allclose(diff[(reason != 0)[finite]], 5.0, rtol=0, atol=1e-12)


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
class StubEngine:
    def __init__(self, lo, hi):
        self.lo, self.hi, self.targets = lo, hi, []

    def observe(self, fields):
        return np.arange(self.lo, self.hi, dtype=np.float32)[:, None] * np.ones((1, 3), np.float32)

    def env_evaluate(self, spec, target7=None):
        self.targets.append(target7)
        k = np.arange(self.lo, self.hi)
        counts = np.zeros(dr.COUNTS, np.uint32)
        counts[0] = counts[1 + 8] = (k % 2).sum()
        return None if spec.fields == 0 else self.observe(spec.fields), k.astype(np.float32), (k % 2).astype(np.uint8), ((k % 2) * dr.TIMEOUT).astype(np.uint32), counts


@pytest.mark.parametrize("devices", [1, 3])
def test_sharded_view_concatenates_and_sums(pkg, devices):
    from cdpr_simulation_amd.sharding import ShardedEngine, shard_range

    sh = object.__new__(ShardedEngine)  # (no GPU: the per-device engines are stubs)
    sh.B, sh.n = B, 8
    sh.spans = [shard_range(i, devices, B) for i in range(devices)]
    sh.engines = [StubEngine(lo, hi) for lo, hi in sh.spans]
    k = np.arange(B)
    assert np.array_equal(sh.observe(ev.POSE)[:, 0], k.astype(np.float32))
    target = np.random.default_rng(3).uniform(-1, 1, (B, 7)).astype(np.float32)
    obs, reward, mask, reason, counts = sh.env_evaluate(pkg.EnvSpec(fields=ev.POSE), target)
    assert np.array_equal(obs[:, 2], k) and np.array_equal(reward, k) and np.array_equal(mask, k % 2) and np.array_equal(reason, (k % 2) * dr.TIMEOUT)
    assert counts.dtype == np.uint32 and counts[0] == B // 2 == counts[9] and counts.sum() == 2 * (B // 2)
    for e, (lo, hi) in zip(sh.engines, sh.spans):
        assert np.array_equal(e.targets[0], target[lo:hi])
    obs, *_ = sh.env_evaluate(pkg.EnvSpec())
    assert obs is None and all(e.targets[1] is None for e in sh.engines)
