"""What tests/test_mppi_inputs.py (CPU) and tests/test_gpu_mppi.py (GPU) share: the definition of cdpr_mppi_sample_device and
cdpr_mppi_update_device (include/cdpr.h) restated in numpy, the a-priori error bounds of the update, and the inputs of the tests.

Philox4x32-10 is in uint64 arithmetic (products of two 32-bit words).  Box-Muller and the update are in float64 from the same float32
inputs: they are the VALUE of the definition; the GPU computes it in float32 and is held to bounds worked out here, never to a free
tolerance.

Bounds of the update (u = 2^-24, one float32 rounding; the tests allow twice each):
  w_s     the argument a_s = (c_min - c_s) / T carries two roundings (relative 2 u), which expf turns into |a_s| * 2 u relative; expf
          itself is good to 1 ulp = 2 u and its result is rounded: dw_s = w_s * (|a_s| + 2) * 2^-23, plus 2^-149 (the spacing of float32
          denormals: a result down there has no relative precision, 1 ulp of it is this absolute amount).
  U'      (sum dw_s |v_s| + |U'| sum dw_s) / eta   from the weights and from eta, first order,
          + (ceil(S / 64) + 8) * u * sum w_s |v_s| / eta   for the float sums: a lane adds ceil(S / 64) terms, the butterfly six more,
          eta's own sum and the division the rest.
  ess     eta and sum w^2 are each a lane's ceil(S / 256) additions, six butterfly steps and three across the waves (k = ceil(S/256) + 9
          roundings, every partial sum below the total: relative k u each), ess = eta * eta / sum w^2 two more:
          ess * (2 sum dw / eta + 2 sum (w dw) / sum w^2 + (3 k + 2) u).
"""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
NOMINAL_FIRST, CLAMP, SHIFT = 1, 2, 4
U24 = 2.0 ** -24

KNOWN_ANSWERS = [  # (counter, key, output)
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays (or scalars) of counter words; the four output words as uint64 arrays below 2^32"""
    c = [np.asarray(x, np.uint64) & MASK for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return c


def box_muller(x, y):
    """(z0, z1) in float64 from two arrays of words: u1 = ((x >> 9) + 1) 2^-23, a = (y >> 8) 2^-23, r = sqrt(-2 ln u1)"""
    u1 = ((x >> np.uint64(9)) + np.uint64(1)).astype(np.float64) * 2.0 ** -23
    a = (y >> np.uint64(8)).astype(np.float64) * 2.0 ** -23
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(np.pi * a), r * np.sin(np.pi * a)


def group_words(groups, g, iteration, seed_lo, seed_hi):
    """the words of groups 0 .. groups - 1 of the robot with global index g: uint64[groups, 4]"""
    j = np.arange(groups, dtype=np.uint64)
    return np.stack(philox(j, int(g) & 0xFFFFFFFF, int(iteration) & 0xFFFFFFFF, 0, seed_lo, seed_hi), axis=1)


def normals(E, g, iteration, seed_lo, seed_hi):
    """z float64[E]: the normals of one robot's block"""
    x = group_words((E + 3) // 4, g, iteration, seed_lo, seed_hi)
    z = np.empty((x.shape[0], 4))
    z[:, 0], z[:, 1] = box_muller(x[:, 0], x[:, 1])
    z[:, 2], z[:, 3] = box_muller(x[:, 2], x[:, 3])
    return z.reshape(-1)[:E]


def sample(nominal, S, sigma, flags=0, cmd_min=0.0, cmd_max=0.0, iteration=0, seed_lo=0, seed_hi=0, robot_offset=0):
    """(v float64[B, H, S, n], noisy bool[B, H, S, n], z float64[B, H, S, n]): the command before its rounding to float32 - sigma and the
    bounds as the float32 the spec holds - where noise was added, and the normals.  Entries that are not noisy are exact."""
    U = np.asarray(nominal, np.float32)
    B, H, n = U.shape
    sigma, lo, hi = (np.float64(np.float32(x)) for x in (sigma, cmd_min, cmd_max))
    z = np.stack([normals(H * S * n, robot_offset + b, iteration, seed_lo, seed_hi).reshape(H, S, n) for b in range(B)])
    base = np.broadcast_to(U.astype(np.float64)[:, :, None, :], (B, H, S, n))
    noisy = np.ones((B, H, S, n), bool)
    if flags & NOMINAL_FIRST:
        noisy[:, :, 0, :] = False
    v = np.where(noisy, sigma * z + base, base)
    if flags & CLAMP:
        v = np.fmin(np.fmax(v, lo), hi)
    return v, noisy, z


def update(cost, commands, nominal, temperature, shift=False):
    """The update of one batch.  Returns a dict: plan, action, weights, ess (float64 values), status (uint32[3], exact) and
    plan_bound, action_bound, weights_bound, ess_bound (the a-priori bounds of the module's text; the tests allow twice each).  A
    degenerate robot's plan and action are the old nominal with bound 0."""
    c32, V32, U32 = np.asarray(cost, np.float32), np.asarray(commands, np.float32), np.asarray(nominal, np.float32)
    B, H, S, n = V32.shape
    T = np.float64(np.float32(temperature))
    out = {k: np.zeros(s) for k, s in (("plan", (B, H, n)), ("plan_bound", (B, H, n)), ("weights", (B, S)), ("weights_bound", (B, S)), ("ess", B), ("ess_bound", B))}
    status = np.zeros(3, np.uint32)
    for b in range(B):
        c = c32[b].astype(np.float64)
        ok = np.isfinite(c)
        status[2] += np.count_nonzero(~ok)
        if not ok.any():
            status[1] += 1
            out["plan"][b] = U32[b]
            continue
        status[0] += 1
        with np.errstate(all="ignore"):
            a = np.where(ok, (c[ok].min() - c) / T, -np.inf)
            w = np.where(ok, np.exp(a), 0.0)
        dw = np.where(ok, w * (np.abs(np.where(ok, a, 0.0)) + 2.0) * 2.0 ** -23 + 2.0 ** -149, 0.0)
        eta, sq = w.sum(), (w * w).sum()
        k = -(-S // 256) + 9
        out["weights"][b], out["weights_bound"][b] = w, dw
        out["ess"][b] = eta * eta / sq
        out["ess_bound"][b] = out["ess"][b] * (2 * dw.sum() / eta + 2 * (w * dw).sum() / sq + (3 * k + 2) * U24)
        sel = w.astype(np.float32) != 0  # a weight of exactly 0 is selected out: what is behind it does not reach the plan
        v = V32[b][:, sel, :].astype(np.float64)  # [H, S', n]
        ws, dws = w[sel][None, :, None], dw[sel][None, :, None]
        plan = (ws * v).sum(axis=1) / eta
        out["plan"][b] = plan
        out["plan_bound"][b] = ((dws * np.abs(v)).sum(axis=1) + np.abs(plan) * dw.sum()) / eta + (-(-S // 64) + 8) * U24 * (ws * np.abs(v)).sum(axis=1) / eta
    out["action"], out["action_bound"] = out["plan"][:, 0, :].copy(), out["plan_bound"][:, 0, :].copy()
    if shift:
        rows = np.minimum(np.arange(H) + 1, H - 1)
        out["plan"], out["plan_bound"] = out["plan"][:, rows, :], out["plan_bound"][:, rows, :]
    out["status"] = status
    return out


# ---- the update's inputs ------------------------------------------------------------------------------------------------------
PATTERNS = ("uniform", "heavy_tail", "clear_minimum", "plain_mean", "bad_mixed", "one_robot_all_bad", "nan_behind_zero")
# (S, H, n, B): every S, H, n and B of the matrix at least once, the sizes on both sides of a wave and of a workgroup's stride
UPDATE_SHAPES = [(1, 1, 1, 1), (63, 4, 3, 5), (64, 9, 8, 5), (65, 1, 12, 1), (129, 4, 8, 130), (300, 9, 3, 1), (300, 4, 12, 5), (64, 4, 1, 130)]


def update_inputs(pattern, S, H, n, B, seed=0):
    """(cost float32[B, S], commands float32[B, H, S, n], nominal float32[B, H, n], temperature) of one case"""
    rng = np.random.default_rng([seed, S, H, n, B, PATTERNS.index(pattern)])
    V = rng.uniform(-0.05, 0.05, (B, H, S, n)).astype(np.float32)
    U = rng.uniform(-0.05, 0.05, (B, H, n)).astype(np.float32)
    cost = rng.uniform(0.5, 1.5, (B, S)).astype(np.float32)
    T = 0.25
    if pattern == "heavy_tail":
        cost = (rng.pareto(1.2, (B, S)) * 3.0 + 0.01).astype(np.float32)
        cost[:, ::7] *= np.float32(40.0)  # (weights down to denormals and to 0)
    elif pattern == "clear_minimum":
        cost[np.arange(B), rng.integers(0, S, B)] = np.float32(0.25)
        T = 1e-6  # every other weight underflows to exactly 0: the action IS that sample's command
    elif pattern == "plain_mean":
        T = 1e30  # every weight rounds to exactly 1
    elif pattern in ("bad_mixed", "one_robot_all_bad", "nan_behind_zero"):
        bad = np.array([np.nan, np.inf, -np.inf], np.float32)
        hit = rng.random((B, S)) < 0.3
        if S > 1:
            hit[:, rng.integers(0, S)] = False  # (a usable cost stays)
        else:
            hit[:] = False
        cost[hit] = bad[rng.integers(0, 3, int(hit.sum()))]
        if pattern == "one_robot_all_bad":
            cost[B // 2] = bad[rng.integers(0, 3, S)]
        if pattern == "nan_behind_zero":
            keep = np.argmax(~hit, axis=1)  # (every robot's first usable cost becomes its least)
            far = ~hit & (rng.random((B, S)) < 0.3)
            far[np.arange(B), keep] = False
            cost[far] += np.float32(1e4)  # exp(-4e4) is exactly 0, in float32 and in float64
            cost[np.arange(B), keep] = np.float32(0.4)
            dead = hit | far
            V[np.broadcast_to(dead[:, None, :, None], V.shape) & (rng.random(V.shape) < 0.5)] = np.nan
    return cost, V, U, T


# ---- the sampler's shapes and the refusals ------------------------------------------------------------------------------------
# (B, H, S, n): E = 1 (one partial group), E = 30 (no multiple of 4: the dword-store form), whole groups, S past a wave, many robots
SAMPLE_SHAPES = [(1, 1, 1, 1), (3, 2, 5, 3), (2, 3, 64, 8), (5, 4, 65, 4), (130, 2, 7, 8)]
SAMPLE_LARGE = (512, 8, 128, 8)

# The refusal list of include/cdpr.h, clause by clause: (the header's words, the code, the calls, specs that break it).  `specs` maps a
# dict of good MppiSpec keyword arguments to the list of broken ones; None: the clause is about an argument, not the spec.
NAN, INF = float("nan"), float("inf")
REFUSALS = [
    ("a NULL handle", "INVALID", "both", None),
    ("a NULL spec", "INVALID", "both", None),
    ("a NULL required buffer (sample: d_nominal, d_commands; update: d_cost, d_commands, d_nominal)", "INVALID", "both", None),
    ("struct_size != sizeof(cdpr_mppi_spec_t)", "INVALID", "both", None),
    ("an unknown flag bit", "INVALID", "both", lambda kw: [dict(kw, flags=f) for f in (8, 1 << 31, 7 | 16)]),
    ("reserved != 0", "INVALID", "both", None),
    ("samples == 0", "INVALID", "both", lambda kw: [dict(kw, samples=0)]),
    ("horizon == 0", "INVALID", "both", lambda kw: [dict(kw, horizon=0)]),
    ("a sigma that is negative or not finite", "INVALID", "both", lambda kw: [dict(kw, sigma=s) for s in (-1e-30, -1.0, NAN, INF)]),
    ("a temperature that is not finite or not > 0 (the update)", "INVALID", "update", lambda kw: [dict(kw, temperature=t) for t in (0.0, -1.0, NAN, INF)]),
    ("CDPR_MPPI_CLAMP with bounds that are not finite or with cmd_min > cmd_max", "INVALID", "both",
     lambda kw: [dict(kw, flags=CLAMP, cmd_min=lo, cmd_max=hi) for lo, hi in ((1.0, 0.5), (NAN, 1.0), (0.0, NAN), (-INF, 1.0), (0.0, INF))]),
    ("E > 2^34", "UNSUPPORTED", "both", lambda kw: [dict(kw, samples=1 << 17, horizon=(1 << 17) + 1), dict(kw, samples=3, horizon=1 << 31)]),
    ("B * S > 2^30 (the rollout's own limit)", "UNSUPPORTED", "both", lambda kw: [dict(kw, samples=(1 << 30) + 1, horizon=1)]),
]
