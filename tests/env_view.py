"""The environment view (cdpr_observe_device, cdpr_env_evaluate_device): the observation tensor and the reward in numpy, and the
scenario shared by tests/test_env_view_inputs.py (CPU) and tests/test_gpu_env_view.py (GPU), and the comparisons of an engine with them
that tests/test_gpu_env_view.py and tests/test_gpu_padded_stride.py make.  A plain module: no fixtures, no hooks.

Both references take only what the engine's getters return (include/cdpr.h specifies the view as a function of them):
`observation_reference` concatenates getter outputs, so the comparison with the device tensor is bit for bit; `reward_reference` is
the header's formula in float64, `reward_f32` the same formula in float32 in the header's order, every fma as one rounding of the
exact float64 product-sum (a float32 product is exact in float64; the double rounding that remains differs from a true fma in far less
than one case in 2^20).

The bound of the reward comparison, from the formats and not from any result: with M = |alive| + |done_penalty| + sum |w_k| m_k (m_k
the term's float64 value; 1 for the orientation term, which is 1 minus a quotient near 1), an fp32 handle's reward lies within 64 *
2^-24 * M of the float64 value: the longest chain - twelve efforts, then the six weighted terms and the penalty - has fewer than 32
roundings, each relative 2^-24 of a non-negative partial sum bounded by M, and a factor two covers the terms' own roundings.  A
precision = 64 handle computes in double and rounds once at the store: 2^-24 |r| + 64 * 2^-53 * M.
"""
import numpy as np
from scipy.spatial.transform import Rotation

import done_handles as gd
import done_rules as dr

FIELD_NAMES = ("pose", "twist", "joint_position", "joint_velocity", "effort", "fk_pose", "fk_residual", "age")
POSE, TWIST, JOINT_POSITION, JOINT_VELOCITY, EFFORT, FK_POSE, FK_RESIDUAL, AGE = (1 << k for k in range(8))
ALL, NEED_FK = 0xFF, FK_POSE | FK_RESIDUAL
WEIGHTS = ("w_position", "w_orientation", "w_speed", "w_rate", "w_effort", "w_fk_residual")
AT_TARGET = 100  # the robot of the scenario that sits exactly at its target


def field_widths(n):
    return (7, 6, n, n, n, 7, 1, 1)


def fields_of(cfg):
    """every field the handle serves"""
    return ALL if cfg.stages & 1 else ALL & ~NEED_FK


def view_getters(eng, cfg):
    """What the observation is a function of, as the FLOAT getters hand it out (on a precision = 64 handle they round once)."""
    pose, twist = eng.raw_state()
    q, qd, effort = eng.joint_states()
    fk = eng.fk_state() if cfg.stages & 1 else (None, None, None)
    return dict(pose=pose, twist=twist, joint_position=q, joint_velocity=qd, effort=effort, fk_pose=fk[0], fk_residual=fk[1],
                start=eng.episode_start(), step_count=eng.step_count)


def observation_reference(fields, pose, twist, joint_position, joint_velocity, effort, fk_pose, fk_residual, start, step_count):
    """float32[B, width]: the getters' arrays side by side, the fields of `fields` in bit order."""
    age = (np.uint32(int(step_count) & 0xFFFFFFFF) - np.asarray(start, dtype=np.uint32)).astype(np.uint32).astype(np.float32)
    parts = (pose, twist, joint_position, joint_velocity, effort, fk_pose, None if fk_residual is None else np.asarray(fk_residual)[:, None], age[:, None])
    cols = [np.asarray(p, dtype=np.float32) for k, p in enumerate(parts) if (fields >> k) & 1]
    assert all(c.dtype == np.float32 for c in cols)
    return np.concatenate(cols, axis=1) if cols else np.zeros((len(age), 0), np.float32)


def reward_getters(eng, cfg):
    """What the reward is a function of, in the handle's precision: raw_state, the effort of the last published step, the FK residual
    as fk_state hands it out (float32 on every handle)."""
    f64 = cfg.precision == 64
    pose, twist = eng.raw_state_f64() if f64 else eng.raw_state()
    effort = eng.observables_f64()[2] if f64 else eng.joint_states()[2]
    return dict(pose=pose, twist=twist, effort=effort, fk_residual=eng.fk_state()[1] if cfg.stages & 1 else None)


def weights_of(spec):
    return [float(getattr(spec, w)) for w in WEIGHTS]  # (float32 values, as the struct holds them)


def reward_terms(pose, twist, effort, fk_residual, target7, fma, T):
    """the six terms in the header's order of operations, in T; fma(a, b, c) supplied by the caller"""
    p, t, g = np.asarray(pose).astype(T), np.asarray(twist).astype(T), np.asarray(target7, dtype=np.float32).astype(T)
    e = np.asarray(effort).astype(T)
    res = np.zeros(len(p), T) if fk_residual is None else np.asarray(fk_residual, dtype=np.float32).astype(T)
    with np.errstate(all="ignore"):
        d = p[:, :3] - g[:, :3]
        pos = fma(d[:, 2], d[:, 2], fma(d[:, 1], d[:, 1], d[:, 0] * d[:, 0]))
        dot = lambda a, b: fma(a[:, 6], b[:, 6], fma(a[:, 5], b[:, 5], fma(a[:, 4], b[:, 4], a[:, 3] * b[:, 3])))  # noqa: E731
        c, qq, tt = dot(p, g), dot(p, p), dot(g, g)
        ori = T(1) - (c * c) / (qq * tt)
        vv = fma(t[:, 2], t[:, 2], fma(t[:, 1], t[:, 1], t[:, 0] * t[:, 0]))
        ww = fma(t[:, 5], t[:, 5], fma(t[:, 4], t[:, 4], t[:, 3] * t[:, 3]))
        ee = np.zeros(len(p), T)
        for i in range(e.shape[1]):
            ee = fma(e[:, i], e[:, i], ee)
    return [pos, ori, vv, ww, ee, res]


def _combine(spec, terms, reason, fma, T):
    r = np.full(len(terms[0]), T(spec.alive))
    with np.errstate(all="ignore"):
        for w, term in zip(weights_of(spec), terms):
            if w != 0.0:  # a weight of exactly 0 selects its term out
                r = fma(np.full_like(r, -T(w)), term, r)
        r = np.where(np.asarray(reason) != 0, r - T(spec.done_penalty), r)
    return r


def target_or_home(target7, home, batch):
    return np.tile(np.asarray(home, dtype=np.float32), (batch, 1)) if target7 is None else np.asarray(target7, dtype=np.float32).reshape(batch, 7)


def reward_reference(spec, pose, twist, effort, fk_residual, reason, target7, home):
    """(r, M) in float64: the reward of include/cdpr.h and the magnitude the bound is stated in."""
    g = target_or_home(target7, home, len(pose))
    plain = lambda a, b, c: a * b + c  # noqa: E731
    terms = reward_terms(pose, twist, effort, fk_residual, g, plain, np.float64)
    r = _combine(spec, terms, reason, plain, np.float64)
    m = [terms[0], np.ones_like(terms[1]), terms[2], terms[3], terms[4], terms[5]]
    with np.errstate(all="ignore"):
        M = abs(float(spec.alive)) + abs(float(spec.done_penalty)) + sum(abs(w) * mk for w, mk in zip(weights_of(spec), m) if w != 0.0)
    return r, M * np.ones(len(r))


def fma32(a, b, c):
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)


def reward_f32(spec, pose, twist, effort, fk_residual, reason, target7, home):
    """The same in float32, operation by operation as the header states it (what an fp32 handle computes)."""
    g = target_or_home(target7, home, len(pose))
    return _combine(spec, reward_terms(pose, twist, effort, fk_residual, g, fma32, np.float32), reason, fma32, np.float32)


def reward_bound(r, M, f64):
    return 2.0 ** -24 * np.abs(r) + 64 * 2.0 ** -53 * M if f64 else 64 * 2.0 ** -24 * M


def inside(got, r, M, f64):
    """bool[B]: |got - r| within the bound (robots whose reference is not finite: False)"""
    with np.errstate(all="ignore"):
        return np.abs(np.asarray(got, dtype=np.float64) - r) <= reward_bound(r, M, f64)


# ---- the scenario ------------------------------------------------------------------------------------------------------------------
def scenario(pkg, model, f64):
    """(rule, spec kwargs, pose, twist, target7): dr.static_scenario's batch - NaN and Inf robots included - with per-robot targets spread
    over the workspace (+-0.05 m, tilts to 0.3 rad), robot AT_TARGET exactly at its target (its pose rounded to float32, which a target
    can hold), and weights that are all distinct."""
    rule, pose, twist = dr.static_scenario(pkg, model, f64)
    rng = np.random.default_rng(2031)
    home = np.asarray(model.home_pose(), dtype=np.float64)
    target = np.tile(home, (dr.B, 1))
    target[:, :3] += rng.uniform(-0.05, 0.05, (dr.B, 3))
    axis = rng.normal(size=(dr.B, 3))
    axis /= np.linalg.norm(axis, axis=1)[:, None]
    target[:, 3:] = Rotation.from_rotvec(axis * rng.uniform(0.0, 0.3, (dr.B, 1))).as_quat()
    target = target.astype(np.float32)
    pose[AT_TARGET] = pose[AT_TARGET].astype(np.float32)
    target[AT_TARGET] = pose[AT_TARGET].astype(np.float32)
    weights = dict(w_position=40.0, w_orientation=3.0, w_speed=0.5, w_rate=0.25, w_effort=0.002, w_fk_residual=7.0, alive=1.0, done_penalty=5.0)
    return rule, weights, pose, twist, target


def spec_of(pkg, cfg, rule, weights, fields=0, ld=0, **over):
    """an EnvSpec for the handle: the FK residual's weight only where the handle has the stage"""
    kw = dict(weights, **over)
    if not cfg.stages & 1:
        kw["w_fk_residual"] = 0.0
    return pkg.EnvSpec(done=rule, fields=fields, ld=ld, **kw)


# ---- the comparisons on an engine (tests/test_gpu_env_view.py, tests/test_gpu_padded_stride.py) -----------------------------------
SENTINEL = np.float32(-77.25)


class Buffers:
    """device buffers of a test, freed together"""

    def __init__(self, eng):
        self.eng, self.ptrs = eng, []

    def upload(self, array):
        self.ptrs.append(self.eng.device_upload(array))
        return self.ptrs[-1]

    def free(self):
        self.eng.synchronize()
        for p in self.ptrs:
            self.eng.device_free(p)
        self.ptrs = []


def observe_padded(eng, bufs, fields, ld, batch, d_row_mask=0, rows=None):
    """observe_device into a sentinel-filled float[rows][ld] (rows > B): the whole buffer back"""
    rows = rows or batch + 7
    d = bufs.upload(np.full((rows, ld), SENTINEL, np.float32))
    eng.observe_device(fields, d, ld, d_row_mask)
    return eng.device_download(d, (rows, ld), np.float32)


def check_observation(eng, cfg, bufs, where, batch=dr.B):
    """case 1 at the engine's present state: every single field and all fields, ld = width and width + 3"""
    g = view_getters(eng, cfg)
    every = fields_of(cfg)
    for fields in [1 << k for k in range(8) if (every >> k) & 1] + [every]:
        want = observation_reference(fields, **g)
        width = want.shape[1]
        assert eng.observation_width(fields) == width == observation_reference(fields, **g).shape[1], f"{where}, fields {fields:#x}: the width"
        for ld in (width, width + 3):
            got = observe_padded(eng, bufs, fields, ld, batch)
            assert np.array_equal(got[:batch, :width], want, equal_nan=True), f"{where}, fields {fields:#x}, ld {ld}: columns differ from the getters at {np.argwhere(~((got[:batch, :width] == want) | (np.isnan(want) & np.isnan(got[:batch, :width]))))[:6].tolist()}"
            assert (got[batch:] == SENTINEL).all() and (got[:, width:] == SENTINEL).all(), f"{where}, fields {fields:#x}, ld {ld}: written past row B or past the width"
    assert np.array_equal(eng.observe(every), observation_reference(every, **g), equal_nan=True), f"{where}: Engine.observe"
    return g


def check_reward_and_verdict(pkg, eng, cfg, rule, weights, target, where, nan_robots=(), batch=dr.B):
    """cases 3 and 4 at the engine's present state; returns (spec, reward, reason)"""
    f64 = cfg.precision == 64
    every = fields_of(cfg)
    spec = spec_of(pkg, cfg, rule, weights, fields=every)
    want_verdict = eng.evaluate_done(rule)
    obs, reward, mask, reason, counts = eng.env_evaluate(spec, target)
    gd.assert_verdict((mask, reason, counts), want_verdict, f"{where}, verdict")
    assert np.array_equal(obs, eng.observe(every), equal_nan=True), f"{where}: the observation of env_evaluate"
    rg = reward_getters(eng, cfg)
    home = cfg.model.home_pose()
    r, M = reward_reference(spec, reason=reason, target7=target, home=home, **rg)
    finite = np.isfinite(r)
    with np.errstate(all="ignore"):
        worst = float((np.abs(reward.astype(np.float64) - r)[finite] / reward_bound(r, M, f64)[finite]).max())
    print(f"env view, {where}: reward within {worst:.3f} of the bound, {int((reason != 0).sum())} robots done")
    assert reward.dtype == np.float32 and inside(reward, r, M, f64)[finite].all(), f"{where}: the reward leaves the bound ({worst:.2f} x) for robots {np.nonzero(finite & ~inside(reward, r, M, f64))[0][:8]}"
    assert np.array_equal(np.nonzero(~finite)[0], np.sort(np.asarray(nan_robots, dtype=np.int64))), f"{where}: the reference is not finite for robots {np.nonzero(~finite)[0]}"
    assert np.array_equal(reward[~finite].astype(np.float64), r[~finite], equal_nan=True), f"{where}: NaN / Inf rewards differ from the reference's"
    # the bound separates this formula from a wrong one on these very inputs (both weights are live here)
    swapped = spec_of(pkg, cfg, rule, dict(weights, w_position=weights["w_orientation"], w_orientation=weights["w_position"]))
    assert (~inside(reward, *reward_reference(swapped, reason=reason, target7=target, home=home, **rg), f64)[finite]).sum() >= batch // 2, f"{where}: swapped weights stay inside the bound"
    # the penalty is visible on exactly the done robots
    free = eng.env_evaluate(spec_of(pkg, cfg, rule, weights, done_penalty=0.0), target)[1]
    with np.errstate(all="ignore"):
        assert np.array_equal((free != reward)[finite], (reason != 0)[finite]) and np.allclose((free - reward)[finite & (reason != 0)], weights["done_penalty"], rtol=0, atol=1e-3), f"{where}: the done penalty"
    return spec, reward, reason


def stand_in_efforts(n, f64):
    """Efforts and FK residuals of the size real steps leave (a few newtons per cable, residuals of 1e-5 .. 1e-3 m), for the CPU checks
    of the bound: the static scenario itself has published nothing, its efforts are zero."""
    rng = np.random.default_rng(2032)
    T = np.float64 if f64 else np.float32
    return rng.uniform(2.0, 9.0, (dr.B, n)).astype(T), (10.0 ** rng.uniform(-5, -3, dr.B)).astype(np.float32)
