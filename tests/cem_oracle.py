"""What tests/test_cem_inputs.py (CPU) and tests/test_gpu_cem.py (GPU) share: the definition of cdpr_cem_sample_device and
cdpr_cem_update_device (include/cdpr.h) restated in numpy, the a-priori error bounds of the update, and the inputs of the tests.

The sampler is mppi_oracle's with a sigma per entry.  The update's integer part - which costs are usable, their order, the elites, the
best sample, the status words - is exact: the GPU has to equal it.  The fit and the smoothing are in float64 from the same float32
inputs: the VALUE of the definition; the GPU computes it in float32 and is held to twice the bounds worked out here, never to a free
tolerance.

Bounds (u = 2^-24, one float32 rounding; K' elites; c = the most terms one lane adds before the butterfly: ceil(K' / 64) where
S <= LDS_CAP, ceil(S / 64) above - the summation orders include/cdpr.h states):
  m       c additions in the lane, six butterfly steps, one division, every partial sum at most sum |v|:
            dm = (c + 7) u sum |v| / K'
  var     the float d_k = v_k - m is off its value by e_k = dm + u (|d_k| + dm) (m's error, then the subtraction's rounding);
          sum d^2 then moves by at most 2 sum |d_k| e_k + sum e_k^2, and the float sum of the squares (fmaf: one rounding per term,
          c terms, six butterfly steps, the division, with room for two more) is relative (c + 9) u of the perturbed sum:
            dvar = (1 + (c + 9) u) (2 sum |d_k| e_k + sum e_k^2) / K' + (c + 9) u var
  f       |sqrt a - sqrt b| <= min(|a - b| / sqrt b, sqrt |a - b|), sqrtf and its rounding 2 u f:
            df = min(dvar / f, sqrt(dvar)) + 2 u f
  blend   out = fmaf(alpha, fit - old, old): the fit's error and the subtraction's rounding times alpha, then the result's rounding:
            alpha (d + u |fit - old|) + u |out|;   alpha == 1 selects the fit: d alone.
  clamp   min and max move two numbers no further apart: nothing is added.
A degenerate robot's plans are the old ones with bound 0.
"""
import numpy as np

import mppi_oracle as mo

NOMINAL_FIRST, CLAMP, SHIFT = 1, 2, 4
U24 = 2.0 ** -24
LDS_CAP = 4096  # kCemLdsSamples: up to here the kernel sums the elites by rank, above by sample index (include/cdpr.h)
STATUS = 4


def sample(mean, sigma, S, flags=0, cmd_min=0.0, cmd_max=0.0, iteration=0, seed_lo=0, seed_hi=0, robot_offset=0):
    """(v float64[B, H, S, n], noisy bool[B, H, S, n], z float64[B, H, S, n]): mppi_oracle.sample with sigma float32[B, H, n] in the
    scalar's place - the command before its rounding to float32, where noise was added, and the normals."""
    U, G = np.asarray(mean, np.float32), np.asarray(sigma, np.float32)
    B, H, n = U.shape
    assert G.shape == U.shape
    lo, hi = (np.float64(np.float32(x)) for x in (cmd_min, cmd_max))
    z = np.stack([mo.normals(H * S * n, robot_offset + b, iteration, seed_lo, seed_hi).reshape(H, S, n) for b in range(B)])
    base = np.broadcast_to(U.astype(np.float64)[:, :, None, :], (B, H, S, n))
    noisy = np.ones((B, H, S, n), bool)
    if flags & NOMINAL_FIRST:
        noisy[:, :, 0, :] = False
    with np.errstate(invalid="ignore"):
        v = np.where(noisy, G.astype(np.float64)[:, :, None, :] * z + base, base)
    if flags & CLAMP:
        v = np.fmin(np.fmax(v, lo), hi)
    return v, noisy, z


def order(cost_row, variant=None):
    """the indices of the usable costs of one robot in the definition's order: by value with -0 equal to +0, equal values by index"""
    c = np.asarray(cost_row, np.float32)
    idx = np.flatnonzero(np.isfinite(c))
    val = c[idx].astype(np.float64) + 0.0  # (-0 + 0 is +0)
    if variant == "neg_zero_first":
        val = np.where((c[idx] == 0) & np.signbit(c[idx]), -1e-300, val)
    if variant == "ties_high":
        return idx[::-1][np.argsort(val[::-1], kind="stable")]
    return idx[np.argsort(val, kind="stable")]


VARIANTS = ("ties_high", "neg_zero_first", "extra_elite", "var_km1", "no_smoothing", "shift_first")


def update(cost, commands, mean, sigma, K, alpha=1.0, sigma_min=0.0, sigma_max=np.inf, shift=False, variant=None):
    """The update of one batch.  Returns a dict: mean, sigma, action (float64 values), mean_bound, sigma_bound, action_bound (the
    bounds of the module's text; the tests allow twice each), elite float32[B, S], best int32[B], status uint32[4] (exact).  `variant`
    (one of VARIANTS) computes a WRONG definition instead: what the bounds must tell from the right one."""
    c32, V32 = np.asarray(cost, np.float32), np.asarray(commands, np.float32)
    M32, G32 = np.asarray(mean, np.float32), np.asarray(sigma, np.float32)
    B, H, S, n = V32.shape
    al, smin, smax = (np.float64(np.float32(x)) for x in (alpha, sigma_min, sigma_max))
    out = {k: np.zeros((B, H, n)) for k in ("mean", "sigma", "mean_bound", "sigma_bound")}
    elite, best, status = np.zeros((B, S), np.float32), np.full(B, -1, np.int32), np.zeros(STATUS, np.uint32)
    rows = np.minimum(np.arange(H) + 1, H - 1)
    for b in range(B):
        o = order(c32[b], variant)
        status[2] += S - len(o)
        old_m, old_s = M32[b].astype(np.float64), G32[b].astype(np.float64)
        if len(o) == 0:
            status[1] += 1
            out["mean"][b], out["sigma"][b] = old_m, old_s
            continue
        status[0] += 1
        status[3] += len(o) < K
        Kp = min(K + (variant == "extra_elite"), len(o))
        el = np.sort(o[:Kp])
        elite[b, el], best[b] = 1.0, o[0]
        v = V32[b][:, el, :].astype(np.float64)  # [H, K', n]: no other command is read
        cc = -(-Kp // 64) if S <= LDS_CAP else -(-S // 64)
        with np.errstate(all="ignore"):
            m = v.sum(axis=1) / Kp
            d = v - m[:, None, :]
            var = (d * d).sum(axis=1) / (Kp - 1 if variant == "var_km1" else Kp)
            f = np.sqrt(var)
            dm = (cc + 7) * U24 * np.abs(v).sum(axis=1) / Kp
            e = dm[:, None, :] + U24 * (np.abs(d) + dm[:, None, :])
            dvar = (1 + (cc + 9) * U24) * (2 * (np.abs(d) * e).sum(axis=1) + (e * e).sum(axis=1)) / Kp + (cc + 9) * U24 * var
            df = np.fmin(dvar / f, np.sqrt(dvar)) + 2 * U24 * f
            if variant == "shift_first" and shift:
                old_m, old_s = old_m[rows], old_s[rows]
            if al == 1.0 or variant == "no_smoothing":
                new_m, new_s, bm, bs = m, f, dm, df
            else:
                new_m, new_s = al * (m - old_m) + old_m, al * (f - old_s) + old_s
                bm = al * (dm + U24 * np.abs(m - old_m)) + U24 * np.abs(new_m)
                bs = al * (df + U24 * np.abs(f - old_s)) + U24 * np.abs(new_s)
            new_s = np.fmin(np.fmax(new_s, smin), smax)
        out["mean"][b], out["sigma"][b], out["mean_bound"][b], out["sigma_bound"][b] = new_m, new_s, bm, bs
    out["action"], out["action_bound"] = out["mean"][:, 0, :].copy(), out["mean_bound"][:, 0, :].copy()
    if shift:
        dead = best < 0
        for k in ("mean", "sigma", "mean_bound", "sigma_bound"):
            moved = out[k][:, rows, :]
            if variant == "shift_first":  # (the wrong definition moved the OLD plans and blended in place; dead robots move either way)
                moved = np.where(dead[:, None, None], moved, out[k])
            out[k] = moved
    out["elite"], out["best"], out["status"] = elite, best, status
    return out


def tree_sum(x):
    """float32 sum over axis 1 by a binary tree of neighbours (depth ceil(log2 K') <= 6 + c: what the bounds assume of an order)"""
    x = np.asarray(x, np.float32)
    while x.shape[1] > 1:
        if x.shape[1] % 2:
            x = np.concatenate([x, np.zeros_like(x[:, :1])], axis=1)
        x = x[:, 0::2] + x[:, 1::2]
    return x[:, 0]


def update_f32(cost, commands, mean, sigma, K, alpha=1.0, sigma_min=0.0, sigma_max=np.inf, shift=False):
    """(mean, sigma float32[B, H, n]) by the definition in float32 with tree sums over the elites in descending index: ANOTHER summation
    order than the kernel's, which the bounds have to cover just the same"""
    c32, V32 = np.asarray(cost, np.float32), np.asarray(commands, np.float32)
    new_m, new_s = np.array(mean, np.float32), np.array(sigma, np.float32)
    B, H, S, n = V32.shape
    al = np.float32(alpha)
    for b in range(B):
        o = order(c32[b])
        if len(o) == 0:
            continue
        Kp = min(K, len(o))
        v = V32[b][:, np.sort(o[:Kp])[::-1], :]
        with np.errstate(all="ignore"):
            m = tree_sum(v) / np.float32(Kp)
            d = v - m[:, None, :]
            f = np.sqrt(tree_sum(d * d) / np.float32(Kp))
            if al != 1:  # (fmaf: the product and the sum in double, one rounding that counts)
                m = (np.float64(al) * (m - new_m[b]).astype(np.float64) + new_m[b]).astype(np.float32)
                f = (np.float64(al) * (f - new_s[b]).astype(np.float64) + new_s[b]).astype(np.float32)
            new_m[b], new_s[b] = m, np.fmin(np.fmax(f, np.float32(sigma_min)), np.float32(sigma_max))
    if shift:
        rows = np.minimum(np.arange(H) + 1, H - 1)
        new_m, new_s = new_m[:, rows], new_s[:, rows]
    return new_m, new_s


# ---- the update's inputs ------------------------------------------------------------------------------------------------------
PATTERNS = ("distinct", "ties", "bad_mixed", "one_robot_all_bad", "short", "nan_behind_non_elite", "identical_elites")
# (S, K, H, n, B): S and K on both sides of a wave (64) and S of the workgroup's stride (256), K = 1, K = S, every n path (scalar
# loads, one, two and three 16-byte loads), H on both sides of a round of four, more robots than one
UPDATE_SHAPES = [(1, 1, 1, 1, 1), (63, 7, 4, 3, 5), (64, 64, 9, 8, 5), (65, 1, 1, 12, 1), (129, 63, 4, 8, 130), (129, 64, 4, 8, 130),
                 (129, 65, 4, 8, 130), (300, 30, 9, 3, 1), (300, 299, 4, 12, 5), (64, 8, 4, 1, 130)]
PAST_CAP_SHAPE = (LDS_CAP + 5, 410, 2, 3, 1)  # S just past the kernel's LDS cap: costs folded again in every pass, sums by sample index
# (alpha, sigma_min, sigma_max): the fit itself, no upper clamp; a blend whose sigma meets the upper clamp in part
SMOOTHINGS = [(1.0, 1e-4, np.inf), (0.7, 1e-3, 0.027)]
BAD = np.array([np.nan, np.inf, -np.inf], np.float32)


def distinct_costs(rng, B, S):
    """float32[B, S]: a permutation of S distinct magnitudes over 1e-6 .. 1e4 per robot, a quarter of them negative"""
    mag = np.logspace(-6, 4, S).astype(np.float32)
    cost = np.stack([rng.permutation(mag) for _ in range(B)])
    cost[rng.random((B, S)) < 0.25] *= np.float32(-1)
    return cost


def update_inputs(pattern, S, K, H, n, B, seed=0):
    """(cost float32[B, S], commands float32[B, H, S, n], mean float32[B, H, n], sigma float32[B, H, n]) of one case"""
    rng = np.random.default_rng([seed, S, K, H, n, B, PATTERNS.index(pattern)])
    V = rng.uniform(-0.05, 0.05, (B, H, S, n)).astype(np.float32)
    U = rng.uniform(-0.05, 0.05, (B, H, n)).astype(np.float32)
    G = rng.uniform(0.005, 0.03, (B, H, n)).astype(np.float32)
    cost = distinct_costs(rng, B, S)
    if pattern == "ties":  # four values, -0 and +0 among them: a < K costs of -1, then zeros of either sign past the cut, the rest 2
        a = (K - 1) // 2
        for b in range(B):
            zeros = min(S - a, K - a + 1 + int(rng.integers(0, 4)))
            row = np.full(S, 2.0, np.float32)
            row[:a] = -1.0
            row[a:a + zeros] = np.where(np.arange(zeros) % 2 == int(rng.integers(0, 2)), np.float32(-0.0), np.float32(0.0))
            cost[b] = rng.permutation(row)
    elif pattern in ("bad_mixed", "one_robot_all_bad"):
        hit = rng.random((B, S)) < 0.3
        hit[:, rng.integers(0, S)] = False  # (a usable cost stays)
        cost[hit] = BAD[rng.integers(0, 3, int(hit.sum()))]
        if pattern == "one_robot_all_bad":
            cost[B // 2] = BAD[rng.integers(0, 3, S)]
    elif pattern == "short":  # max(1, K / 2) usable costs per robot: short of K wherever K > 1
        for b in range(B):
            dead = rng.permutation(S)[max(1, K // 2):]
            cost[b, dead] = BAD[rng.integers(0, 3, len(dead))]
    elif pattern == "nan_behind_non_elite":
        for b in range(B):
            rest = order(cost[b])[K:]
            V[b][:, rest, :] = np.where(rng.random((H, len(rest), n)) < 0.5, np.float32(np.nan), V[b][:, rest, :])
    elif pattern == "identical_elites":  # even robots: every elite has the same commands (variance 0); odd ones: all but the first
        for b in range(B):
            el = np.sort(order(cost[b])[:K])
            V[b][:, el[b % 2:], :] = V[b][:, el[-1:], :]
    return cost, V, U, G


# ---- the refusals ---------------------------------------------------------------------------------------------------------------
# The refusal list of include/cdpr.h, clause by clause: (the header's words, the code, specs that break it).  `specs` maps a dict of
# good CemSpec keyword arguments to the list of broken ones; None: the clause is about an argument or a field the constructor fills.
NAN, INF = float("nan"), float("inf")
REFUSALS = [
    ("a NULL handle", "INVALID", None),
    ("a NULL spec", "INVALID", None),
    ("a NULL required buffer (sample: d_mean, d_sigma, d_commands; update: d_cost, d_commands, d_mean, d_sigma)", "INVALID", None),
    ("struct_size != sizeof(cdpr_cem_spec_t)", "INVALID", None),
    ("an unknown flag bit", "INVALID", lambda kw: [dict(kw, flags=f) for f in (8, 1 << 31, 7 | 16)]),
    ("a reserved word != 0", "INVALID", None),
    ("samples == 0", "INVALID", lambda kw: [dict(kw, samples=0, elites=1), dict(kw, samples=0, elites=0)]),
    ("horizon == 0", "INVALID", lambda kw: [dict(kw, horizon=0)]),
    ("elites == 0", "INVALID", lambda kw: [dict(kw, elites=0)]),
    ("elites > samples", "INVALID", lambda kw: [dict(kw, elites=kw["samples"] + 1), dict(kw, elites=(1 << 32) - 1)]),
    ("an alpha that is not in (0, 1] or not finite", "INVALID", lambda kw: [dict(kw, alpha=x) for x in (0.0, -0.5, 1.0000001, 2.0, NAN, INF, -INF)]),
    ("a sigma_min that is negative or not finite or greater than sigma_max", "INVALID",
     lambda kw: [dict(kw, sigma_min=lo, sigma_max=hi) for lo, hi in ((-1e-30, 1.0), (-1.0, 1.0), (NAN, 1.0), (INF, INF), (0.5, 0.25), (0.0, -1.0), (0.0, -INF))]),
    ("a sigma_max that is NaN (+inf is allowed: no upper clamp)", "INVALID", lambda kw: [dict(kw, sigma_min=0.0, sigma_max=NAN)]),
    ("CDPR_CEM_CLAMP with bounds that are not finite or with cmd_min > cmd_max", "INVALID",
     lambda kw: [dict(kw, flags=CLAMP, cmd_min=lo, cmd_max=hi) for lo, hi in ((1.0, 0.5), (NAN, 1.0), (0.0, NAN), (-INF, 1.0), (0.0, INF))]),
    ("E > 2^34", "UNSUPPORTED", lambda kw: [dict(kw, samples=1 << 17, horizon=(1 << 17) + 1), dict(kw, samples=3, horizon=1 << 31, elites=3)]),
    ("B * S > 2^30 (the rollout's own limit)", "UNSUPPORTED", lambda kw: [dict(kw, samples=(1 << 30) + 1, horizon=1)]),
]
