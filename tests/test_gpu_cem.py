"""cdpr_cem_sample_device / cdpr_cem_update_device: the command batch of the MPC rollout sampled around a mean plan with a sigma plan on
the device, and both plans refitted there to every robot's best samples.  Held to the numpy restatement of the definition
(tests/cem_oracle.py): the sampler as in tests/test_gpu_mppi.py (normals within 4e-6, so a command within that times its sigma plus
half an ulp, exact entries to the bit, a constant sigma plan bit for bit the MPPI sampler's batch); the update's elites, best sample and
status words exactly, mean, sigma and action within twice the a-priori bounds the restatement returns with every value.

  1  the sampler on bare handles: the shapes of mo.SAMPLE_SHAPES with a random sigma plan that has zeros, the constant plan against
     mppi_sample_device, every flag combination, an unaligned buffer, two calls, the poisoned pad.
  2  the update's matrix: co.UPDATE_SHAPES x co.PATTERNS x co.SMOOTHINGS, with and without CDPR_CEM_SHIFT; NULL outputs; two calls; more
     samples than the kernel keeps in LDS.
  3  the closed loop without a host read on a per-robot FK + TD handle and a uniform one, against a twin on the host conveniences.
  4  every refusal, the handle untouched.  5  two shards on one device.  6  one handle per record layout.
"""
import ctypes as C

import numpy as np
import pytest

import cem_oracle as co
import mppi_oracle as mo
from parity import sliced_twelve
from per_robot_kinds import LAYOUTS, clean_env, config_of  # noqa: F401  (clean_env: autouse here too)

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
Z_TOL = 4e-6  # (tests/test_gpu_mppi.py: twice what 1 ulp each of logf, sqrtf and sincospif give at |z| <= 5.65)
WORST = {"mean": 0.0, "sigma": 0.0, "action": 0.0}
SEED = 0x9E3779B97F4A7C15


@pytest.fixture(scope="module")
def bare(pkg):
    """bare(B, n): a uniform handle of B robots with n cables, no FK or TD - neither call reads robot state; one per (B, n)"""
    made = {}

    def get(B, n):
        if (B, n) not in made:
            made[(B, n)] = pkg.Engine(pkg.Config(model=sliced_twelve(pkg, n), batch=B, stages=0), 0)
        return made[(B, n)]

    yield get
    for e in made.values():
        e.close()


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
def check_sample(got, U, G, S, flags, lo, hi, iteration, seed, offset, where):
    """the downloaded batch float32[B, H, S, n] against the restatement"""
    want, noisy, z = co.sample(U, G, S, flags, lo, hi, iteration, seed & 0xFFFFFFFF, seed >> 32, offset)
    assert got.shape == want.shape and np.isfinite(got).all(), where
    sig = np.broadcast_to(G.astype(np.float64)[:, :, None, :], want.shape)
    tol = Z_TOL * sig + 0.5 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    exact = ~noisy | (sig == 0.0)  # entries without noise are the mean (clamped) to the bit
    assert np.array_equal(got[exact], want[exact].astype(np.float32)), f"{where}: an entry without noise is not the mean"
    if flags & co.CLAMP:
        lo32, hi32 = np.float32(lo), np.float32(hi)
        raw = np.where(noisy, sig * z + U.astype(np.float64)[:, :, None, :], want)
        assert (got >= lo32).all() and (got <= hi32).all(), f"{where}: a command outside the bounds"
        assert (got[raw > float(hi32) + tol] == hi32).all() and (got[raw < float(lo32) - tol] == lo32).all(), f"{where}: a clamped entry is not the bound"
    d = np.abs(got.astype(np.float64) - want)
    assert (d <= tol).all(), f"{where}: command off by {d.max():.3e} at {np.unravel_index(d.argmax(), d.shape)} (allowed {tol.ravel()[d.argmax()]:.3e})"


def run_sample(eng, spec, iteration, U, G, pad=64, shift_floats=0, mppi=False):
    """one call into a poisoned buffer with `pad` floats around [0, B E), the batch `shift_floats` floats further on (alignment);
    mppi: cdpr_mppi_sample_device with `spec` an MppiSpec instead (G unused)"""
    B, H, n = U.shape
    total = B * H * spec.samples * n
    d_u, d_g = eng.device_upload(U), eng.device_upload(G)
    d_v = eng.device_upload(np.full(total + 2 * pad + shift_floats, POISON, np.uint32))
    if mppi:
        eng.mppi_sample_device(spec, iteration, d_u, d_v + 4 * (pad + shift_floats))
    else:
        eng.cem_sample_device(spec, iteration, d_u, d_g, d_v + 4 * (pad + shift_floats))
    raw = eng.device_download(d_v, total + 2 * pad + shift_floats, np.uint32)
    for d in (d_u, d_g, d_v):
        eng.device_free(d)
    body = raw[pad + shift_floats:pad + shift_floats + total]
    assert (raw[:pad + shift_floats] == POISON).all() and (raw[pad + shift_floats + total:] == POISON).all(), "written outside [0, B E)"
    return body.view(np.float32).reshape(B, H, spec.samples, n).copy()


@pytest.mark.parametrize("shape", mo.SAMPLE_SHAPES, ids=str)
def test_sample_matrix(pkg, bare, shape):
    B, H, S, n = shape
    eng = bare(B, n)
    rng = np.random.default_rng([1, B, H, S, n])
    U = rng.uniform(-0.05, 0.05, (B, H, n)).astype(np.float32)
    G = rng.uniform(0.0, 0.03, (B, H, n)).astype(np.float32)
    G[rng.random(G.shape) < 0.25] = 0.0
    G.reshape(-1)[0] = 0.0
    lo, hi = -0.055, 0.06
    for flags in (0, co.NOMINAL_FIRST, co.CLAMP, co.NOMINAL_FIRST | co.CLAMP, co.NOMINAL_FIRST | co.CLAMP | co.SHIFT):  # (SHIFT is the update's)
        kw = dict(samples=S, horizon=H, flags=flags, cmd_min=lo, cmd_max=hi, seed=SEED, robot_offset=3)
        spec = pkg.CemSpec(elites=1, **kw)
        got = run_sample(eng, spec, 7, U, G)
        check_sample(got, U, G, S, flags, lo, hi, 7, SEED, 3, f"{shape}, flags {flags}")
        assert np.array_equal(bits(got), bits(run_sample(eng, spec, 7, U, G))), f"{shape}: two calls differ"
        assert np.array_equal(bits(got), bits(run_sample(eng, spec, 7, U, G, shift_floats=1))), f"{shape}: the unaligned buffer differs"
        # a constant plan: the MPPI sampler's batch, bit for bit (aligned and not)
        for shift_floats in (0, 1):
            a = run_sample(eng, spec, 7, U, np.full_like(U, 0.02), shift_floats=shift_floats)
            b = run_sample(eng, pkg.MppiSpec(sigma=0.02, **kw), 7, U, G, shift_floats=shift_floats, mppi=True)
            assert np.array_equal(bits(a), bits(b)), f"{shape}, flags {flags}: a constant sigma plan is not the MPPI sampler's batch"
    # sigma 0 everywhere: the mean to the bit; a NaN sigma: a NaN, cmd_min under the clamp
    got = run_sample(eng, pkg.CemSpec(samples=S, horizon=H, seed=SEED), 1, U, np.zeros_like(U))
    assert np.array_equal(bits(got), bits(np.broadcast_to(U[:, :, None, :], got.shape)))
    N = G.copy()
    N[0, 0, 0] = np.nan
    got = run_sample(eng, pkg.CemSpec(samples=S, horizon=H, seed=SEED), 1, U, N)
    assert np.isnan(got[0, 0, :, 0]).all() and np.isfinite(np.delete(got.reshape(B * H, S, n), 0, axis=0)).all() and np.isfinite(got[0, 0, :, 1:]).all()
    got = run_sample(eng, pkg.CemSpec(samples=S, horizon=H, flags=co.CLAMP, cmd_min=lo, cmd_max=hi, seed=SEED), 1, U, N)
    assert (got[0, 0, :, 0] == np.float32(lo)).all() and np.isfinite(got).all()
    # another key, another iteration, another robot: other commands
    G1 = np.full_like(U, 0.02)
    base = run_sample(eng, pkg.CemSpec(samples=S, horizon=H, seed=SEED), 0, U, G1)
    for kw, iteration in ((dict(seed=SEED + 1), 0), (dict(seed=SEED + (1 << 32)), 0), (dict(seed=SEED), 1), (dict(seed=SEED, robot_offset=1), 0)):
        assert not np.array_equal(base, run_sample(eng, pkg.CemSpec(samples=S, horizon=H, **kw), iteration, U, G1))


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
def check_update(got, want, where):
    """(mean, sigma, action, elite, best, status) of the GPU against the restatement's dict"""
    assert np.array_equal(got[3], want["elite"]) and got[3].dtype == np.float32, f"{where}: the elite sets differ"
    assert np.array_equal(got[4], want["best"]) and got[4].dtype == np.int32, f"{where}: best {got[4]} / {want['best']}"
    assert np.array_equal(got[5], want["status"]), f"{where}: status {got[5]} / {want['status']}"
    for name, g in zip(("mean", "sigma", "action"), got):
        w, bound = want[name], want[name + "_bound"]
        assert g.shape == w.shape and g.dtype == np.float32, (where, name)
        d = np.abs(g.astype(np.float64) - w)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(d > 0, d / bound, 0.0)
        WORST[name] = max(WORST[name], float(ratio.max()))
        print(f"[cem] {where}: {name} max |gpu - definition| = {d.max():.3e}, {ratio.max():.3f} bounds")
        ok = d <= 2 * bound
        assert ok.all(), f"{where}: {name} off by {d[~ok].max():.3e} at {np.argwhere(~ok)[0]} (bound {bound[~ok].max():.3e})"


def run_matrix(pkg, eng, shape, patterns):
    S, K, H, n, B = shape
    for pattern in patterns:
        cost, V, U, G = co.update_inputs(pattern, *shape)
        for alpha, smin, smax in co.SMOOTHINGS:
            for shift in (False, True):
                where = f"{shape}, {pattern}, alpha {alpha}, shift {shift}"
                spec = pkg.CemSpec(samples=S, horizon=H, flags=co.SHIFT if shift else 0, elites=K, alpha=alpha, sigma_min=smin, sigma_max=smax)
                got = eng.cem_update(cost, V, U, G, spec)
                want = co.update(cost, V, U, G, K, alpha, smin, smax, shift)
                check_update(got, want, where)
                rows = np.minimum(np.arange(H) + 1, H - 1) if shift else np.arange(H)
                dead = ~np.isfinite(cost).any(axis=1)
                if dead.any():  # the old plans to the bit (one row on under SHIFT, in place)
                    assert np.array_equal(bits(got[0][dead]), bits(U[dead][:, rows])) and np.array_equal(bits(got[1][dead]), bits(G[dead][:, rows])), f"{where}: a degenerate robot's plans moved"
                    assert np.array_equal(bits(got[2][dead]), bits(U[dead][:, 0])) and (got[3][dead] == 0).all() and (got[4][dead] == -1).all()
                live = ~dead
                assert (got[1][live] >= np.float32(smin)).all() and (got[1][live] <= np.float32(smax)).all(), f"{where}: sigma outside [sigma_min, sigma_max]"
                assert np.isfinite(got[0][live]).all() and np.isfinite(got[1][live]).all(), f"{where}: a non-finite plan"
                if K == 1 and alpha == 1.0:  # the plan IS the best sample's command, sigma is sigma_min
                    rb = np.flatnonzero(live)
                    assert np.array_equal(bits(got[0][rb]), bits(V[rb, :, got[4][rb], :][:, rows])), f"{where}: the plan is not the best sample's command"
                    assert (got[1][rb] == np.float32(smin)).all()
                again = eng.cem_update(cost, V, U, G, spec)
                assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, again)), f"{where}: two calls differ"


@pytest.mark.parametrize("shape", co.UPDATE_SHAPES, ids=str)
def test_update_matrix(pkg, bare, shape):
    run_matrix(pkg, bare(shape[4], shape[3]), shape, co.PATTERNS)


def test_update_more_samples_than_lds(pkg, bare):
    """S past the keys and the list the kernel keeps in LDS: every pass folds the costs again, the fit walks the samples"""
    assert co.PAST_CAP_SHAPE[0] > co.LDS_CAP
    run_matrix(pkg, bare(co.PAST_CAP_SHAPE[4], co.PAST_CAP_SHAPE[3]), co.PAST_CAP_SHAPE, ("ties", "bad_mixed"))


def test_zz_report_measured_ratio():
    print(f"\n[cem] largest |gpu - definition| / bound over the update's matrix: mean {WORST['mean']:.3f}, sigma {WORST['sigma']:.3f}, action {WORST['action']:.3f} (allowed 2)")
    assert WORST["mean"] > 0.0, "the update's matrix did not run"


@pytest.mark.parametrize("shape", [(65, 9, 4, 8, 5), (300, 30, 9, 3, 1)], ids=str)
def test_update_optional_outputs(pkg, bare, shape):
    """NULL for each optional output changes nothing else; nothing is written outside an output's range"""
    S, K, H, n, B = shape
    eng = bare(B, n)
    cost, V, U, G = co.update_inputs("one_robot_all_bad" if B > 1 else "bad_mixed", *shape)
    spec = pkg.CemSpec(samples=S, horizon=H, flags=co.SHIFT, elites=K, alpha=0.7, sigma_min=1e-3, sigma_max=0.027)
    full = eng.cem_update(cost, V, U, G, spec)
    pad = 16
    sizes = (B * n, B * S, B, co.STATUS)
    d_c, d_v = eng.device_upload(cost), eng.device_upload(V)
    for present in ((1, 1, 1, 1), (0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (0, 0, 0, 0)):
        d_u, d_g = eng.device_upload(U), eng.device_upload(G)
        bufs = [eng.device_upload(np.full(k + 2 * pad, POISON, np.uint32)) for k in sizes]
        eng.cem_update_device(spec, d_c, d_v, d_u, d_g, *[(d + 4 * pad) if on else 0 for d, on in zip(bufs, present)])
        assert np.array_equal(bits(eng.device_download(d_u, (B, H, n), np.float32)), bits(full[0])), f"{present}: the mean plan changed"
        assert np.array_equal(bits(eng.device_download(d_g, (B, H, n), np.float32)), bits(full[1])), f"{present}: the sigma plan changed"
        for d, k, on, want in zip(bufs, sizes, present, full[2:]):
            raw = eng.device_download(d, k + 2 * pad, np.uint32)
            assert (raw[:pad] == POISON).all() and (raw[pad + k:] == POISON).all(), f"{present}: written outside an output"
            assert np.array_equal(raw[pad:pad + k], bits(want).ravel()) if on else (raw == POISON).all(), f"{present}: an output changed"
        for d in bufs + [d_u, d_g]:
            eng.device_free(d)
    eng.device_free(d_c), eng.device_free(d_v)


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["per_robot_fk_td", "uniform"])
def test_closed_loop(pkg, kind):
    B, H, S, K, ITER = 8, 6, 64, 8, 3
    if kind == "uniform":
        cfg = pkg.Config(model=pkg.cube_model(), batch=B, stages=0)
    else:
        cfg = pkg.Config(model=pkg.eight_cable_model(), batch=B, stages=pkg._abi.STAGE_FK | pkg._abi.STAGE_TD, perRobotCommands=True)
    n = cfg.n_cables
    rng = np.random.default_rng(41)
    pose = np.tile(cfg.model.home_pose(), (B, 1)).astype(np.float32)
    pose[:, :3] += rng.uniform(-0.02, 0.02, (B, 3)).astype(np.float32)
    ref = (pose[:, :3] + rng.uniform(-0.01, 0.01, (B, 3))).astype(np.float32)
    U0 = rng.uniform(-0.01, 0.01, (B, H, n)).astype(np.float32)
    G0 = np.full((B, H, n), 0.02, np.float32)
    alpha, smin, smax = 0.7, 1e-3, 0.05
    spec = pkg.CemSpec(samples=S, horizon=H, flags=co.NOMINAL_FIRST | co.SHIFT, elites=K, alpha=alpha, sigma_min=smin, sigma_max=smax, seed=77)
    eng, twin = pkg.Engine(cfg, 0), pkg.Engine(cfg, 0)
    for e in (eng, twin):
        e.set_platform_state(pose7=pose)
        e.update(5)
    # the device loop: nothing comes back to the host between the calls (one command, cost and elite buffer per iteration, read afterwards)
    d_u, d_g, d_ref, d_action = eng.device_upload(U0), eng.device_upload(G0), eng.device_upload(ref), eng.device_alloc(4 * B * n)
    d_v = [eng.device_alloc(4 * B * H * S * n) for _ in range(ITER)]
    d_c = [eng.device_alloc(4 * B * S) for _ in range(ITER)]
    d_e = [eng.device_alloc(4 * B * S) for _ in range(ITER)]
    for it in range(ITER):
        eng.cem_sample_device(spec, it, d_u, d_g, d_v[it])
        eng.rollout_velocity_device(d_v[it], S, H, d_ref, d_c[it])
        eng.cem_update_device(spec, d_c[it], d_v[it], d_u, d_g, d_action, d_e[it])
        eng.set_velocity_command_device(d_action, B * n)
        eng.update(1)
    V = [eng.device_download(d, (B, H, S, n), np.float32) for d in d_v]
    cost = [eng.device_download(d, (B, S), np.float32) for d in d_c]
    elite = [eng.device_download(d, (B, S), np.float32) for d in d_e]
    mean_end, sigma_end = eng.device_download(d_u, (B, H, n), np.float32), eng.device_download(d_g, (B, H, n), np.float32)
    # the twin, through the host conveniences: the same bits at every stage, and its sigma plans are the device loop's
    U, G = U0, G0
    means, sigmas = [U0], [G0]
    for it in range(ITER):
        Vh = twin.cem_sample(U, G, spec, it)
        ch = twin.rollout_velocity(Vh, ref)
        U, G, action, eh, _, status = twin.cem_update(ch, Vh, U, G, spec)
        assert np.array_equal(bits(Vh), bits(V[it])) and np.array_equal(bits(ch), bits(cost[it])) and np.array_equal(eh, elite[it]), f"{kind}, iteration {it}"
        assert tuple(status) == (B, 0, 0, 0)
        means.append(U), sigmas.append(G)
        twin.set_velocity_command(action)
        twin.update(1)
    assert np.array_equal(bits(U), bits(mean_end)) and np.array_equal(bits(G), bits(sigma_end))
    # every iteration's update against the restatement, fed with that iteration's downloaded costs and commands
    for it in range(ITER):
        assert np.array_equal(bits(V[it][:, :, 0, :]), bits(means[it]))  # (NOMINAL_FIRST: sample 0 is the mean it was drawn around)
        check_sample(V[it], means[it], sigmas[it], S, co.NOMINAL_FIRST, 0, 0, it, 77, 0, f"{kind}, iteration {it}")
        assert np.isfinite(cost[it]).all() and np.ptp(cost[it], axis=1).min() > 0
        want = co.update(cost[it], V[it], means[it], sigmas[it], K, alpha, smin, smax, shift=True)
        assert np.array_equal(elite[it], want["elite"]), f"{kind}, iteration {it}: the elite sets differ"
        for name, got in (("mean", means[it + 1]), ("sigma", sigmas[it + 1])):
            d = np.abs(got.astype(np.float64) - want[name])
            assert (d <= 2 * want[name + "_bound"]).all(), f"{kind}, iteration {it}: {name} is off by {d.max():.3e}"
        picked = (cost[it] * elite[it]).sum(axis=1) / K
        assert (elite[it].sum(axis=1) == K).all() and (picked < cost[it].mean(axis=1)).all(), "the costs do not discriminate"
    for a, b in zip(eng.raw_state() + eng.joint_states(), twin.raw_state() + twin.joint_states()):
        assert np.array_equal(a, b), f"{kind}: the robots differ from the twin's"
    assert eng.step_count == twin.step_count == 5 + ITER
    for d in [d_u, d_g, d_ref, d_action] + d_v + d_c + d_e:
        eng.device_free(d)
    eng.close(), twin.close()


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg, bare):
    from cdpr_simulation_amd._native import lib

    L = lib()
    code = {"INVALID": pkg._abi.ERR_INVALID, "UNSUPPORTED": pkg._abi.ERR_UNSUPPORTED}
    B, n, S, H = 5, 8, 16, 3
    eng = bare(B, n)
    eng.update(3)
    state, steps, kernel = eng.raw_state() + eng.joint_states(), eng.step_count, eng.kernel_name
    good = dict(samples=S, horizon=H, elites=4, alpha=0.5, sigma_min=0.01, sigma_max=1.0)
    rng = np.random.default_rng(5)
    U = rng.uniform(-1, 1, (B, H, n)).astype(np.float32)
    G = rng.uniform(0.1, 0.2, (B, H, n)).astype(np.float32)
    cost = rng.uniform(0, 1, (B, S)).astype(np.float32)
    d_u, d_g, d_c = eng.device_upload(U), eng.device_upload(G), eng.device_upload(cost)
    d_v = eng.device_upload(np.full(B * H * S * n, POISON, np.uint32))
    sizes = (B * n, B * S, B, co.STATUS)
    outs = [eng.device_upload(np.full(k, POISON, np.uint32)) for k in sizes]
    vp = lambda x: C.c_void_p(x) if x else None  # noqa: E731

    def sample(spec, h=eng._h, u=d_u, g=d_g, v=d_v):
        return L.cdpr_cem_sample_device(h, C.byref(spec) if spec is not None else None, 0, vp(u), vp(g), vp(v))

    def update(spec, h=eng._h, c=d_c, v=d_v, u=d_u, g=d_g):
        return L.cdpr_cem_update_device(h, C.byref(spec) if spec is not None else None, vp(c), vp(v), vp(u), vp(g), *[vp(o) for o in outs])

    seen = set()
    for words, want, broken in co.REFUSALS:
        seen.add(words)
        rc = code[want]
        if broken is not None:
            for kw in broken(good):
                spec = pkg.CemSpec(**kw)
                assert update(spec) == rc and sample(spec) == rc, (words, kw)
        elif words == "a NULL handle":
            assert sample(pkg.CemSpec(**good), h=None) == rc and update(pkg.CemSpec(**good), h=None) == rc
        elif words == "a NULL spec":
            assert sample(None) == rc and update(None) == rc and b"null spec" in L.cdpr_last_error(eng._h)
        elif words.startswith("a NULL required buffer"):
            spec = pkg.CemSpec(**good)
            assert sample(spec, u=0) == rc and sample(spec, g=0) == rc and sample(spec, v=0) == rc
            assert update(spec, c=0) == rc and update(spec, v=0) == rc and update(spec, u=0) == rc and update(spec, g=0) == rc
            assert b"null" in L.cdpr_last_error(eng._h)
        elif words.startswith("struct_size"):
            spec = pkg.CemSpec(**good)
            spec.struct_size = 48
            assert sample(spec) == rc and update(spec) == rc and b"struct_size" in L.cdpr_last_error(eng._h)
        elif words == "a reserved word != 0":
            for k in range(3):
                spec = pkg.CemSpec(**good)
                spec.reserved[k] = 1
                assert sample(spec) == rc and update(spec) == rc and b"reserved" in L.cdpr_last_error(eng._h)
        else:
            raise AssertionError(f"no case for the refusal '{words}'")
    assert len(seen) == len(co.REFUSALS)
    # what is allowed at the edges: alpha 1, sigma_min == sigma_max, sigma_max +inf, elites == samples - on a buffer of their own
    d_w = eng.device_alloc(4 * B * H * S * n)
    for kw in (dict(good, alpha=1.0), dict(good, sigma_min=0.5, sigma_max=0.5), dict(good, sigma_min=0.0, sigma_max=float("inf")), dict(good, elites=S)):
        assert sample(pkg.CemSpec(**kw), v=d_w) == 0, kw
    eng.device_free(d_w)
    # a refused call queued nothing: every buffer is as it was, and so is the handle
    assert (eng.device_download(d_v, B * H * S * n, np.uint32) == POISON).all(), "a refused call wrote commands"
    assert np.array_equal(eng.device_download(d_u, (B, H, n), np.float32), U) and np.array_equal(eng.device_download(d_g, (B, H, n), np.float32), G), "a refused call wrote a plan"
    for o, k in zip(outs, sizes):
        assert (eng.device_download(o, k, np.uint32) == POISON).all(), "a refused call wrote an output"
    assert all(np.array_equal(a, b) for a, b in zip(eng.raw_state() + eng.joint_states(), state)) and eng.step_count == steps
    # ... and the calls themselves are no step launches
    spec = pkg.CemSpec(**good)
    eng.profile_begin()
    assert sample(spec) == 0 and update(spec) == 0
    assert eng.profile_end()[1] == 0 and eng.kernel_name == kernel and eng.step_count == steps
    assert all(np.array_equal(a, b) for a, b in zip(eng.raw_state() + eng.joint_states(), state))
    for d in [d_u, d_g, d_c, d_v] + outs:
        eng.device_free(d)


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
def test_sharded(pkg):
    B, H, S, K, n = 11, 3, 20, 5, 8
    cfg = pkg.Config(model=pkg.eight_cable_model(), batch=B, stages=0)
    one, sh = pkg.Engine(cfg, 0), pkg.ShardedEngine(cfg, devices=[0, 0])
    assert sh.spans == [(0, 6), (6, 11)]
    rng = np.random.default_rng(13)
    U = rng.uniform(-0.05, 0.05, (B, H, n)).astype(np.float32)
    G = rng.uniform(0.01, 0.03, (B, H, n)).astype(np.float32)
    flags = co.NOMINAL_FIRST | co.CLAMP | co.SHIFT
    spec = pkg.CemSpec(samples=S, horizon=H, flags=flags, elites=K, alpha=0.7, sigma_min=1e-3, sigma_max=0.027, cmd_min=-0.06, cmd_max=0.06, seed=99, robot_offset=1 << 31)
    V = one.cem_sample(U, G, spec, 4)
    assert np.array_equal(bits(V), bits(sh.cem_sample(U, G, spec, 4))), "two shards sample another batch"
    check_sample(V, U, G, S, co.NOMINAL_FIRST | co.CLAMP, -0.06, 0.06, 4, 99, 1 << 31, "sharded")
    assert not np.array_equal(V[:5], V[6:])  # (a shard without its offset would repeat the first robots)
    cost = rng.uniform(0.0, 1.0, (B, S)).astype(np.float32)
    cost[7] = np.nan
    cost[2, 3] = np.inf
    cost[9, 3:] = -np.inf
    a, b = one.cem_update(cost, V, U, G, spec), sh.cem_update(cost, V, U, G, spec)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b)), "two shards update differently"
    assert tuple(a[5]) == (B - 1, 1, S + 1 + S - 3, 1)
    check_update(a, co.update(cost, V, U, G, K, 0.7, 1e-3, 0.027, shift=True), "sharded")
    one.close(), sh.close()


# ---- 6 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", LAYOUTS)
def test_any_handle(pkg, monkeypatch, kind):
    """per-robot handles of every record layout (register-resident, general path, precision = 64) serve both calls alike"""
    cfg = config_of(pkg, kind, monkeypatch)
    B, n, H, S, K = cfg.batch, cfg.n_cables, 2, 65, 9
    eng = pkg.Engine(cfg, 0)
    eng.update(2)
    name, steps = eng.kernel_name, eng.step_count
    cost, V, U, G = co.update_inputs("bad_mixed", S, K, H, n, B, seed=3)
    spec = pkg.CemSpec(samples=S, horizon=H, elites=K, alpha=0.7, sigma_min=1e-3, sigma_max=0.027, seed=5)
    check_sample(eng.cem_sample(U, G, spec, 2), U, G, S, 0, 0, 0, 2, 5, 0, kind)
    check_update(eng.cem_update(cost, V, U, G, spec), co.update(cost, V, U, G, K, 0.7, 1e-3, 0.027), kind)
    assert eng.kernel_name == name and eng.step_count == steps
    eng.close()
