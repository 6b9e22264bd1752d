"""What tests/test_resample_inputs.py (CPU) and tests/test_gpu_resample.py (GPU) share: the definition of cdpr_resample_map_device
(include/cdpr.h) restated sequentially - Python integers for everything the definition does in uint64, numpy doubles for the four
operations of ess - the brute-force count of positions the closed form is checked against, and the weight patterns of the tests.

Nothing in the definition depends on the order a sum is taken in, so the GPU is held to this restatement to the bit.
"""
import numpy as np

SCALE = 1 << 30
STATUS = ("copied", "skipped", "resampled", "degenerate", "bad")


def quantise(x):
    """(q list of int, m) of one group's float32 weights; m None: no usable weight"""
    x = np.asarray(x, np.float32)
    ok = np.isfinite(x) & (x > 0)
    if not ok.any():
        return [0] * len(x), None
    m = np.float64(x[ok].max())
    with np.errstate(all="ignore"):
        q = np.floor(x.astype(np.float64) / m * np.float64(SCALE))  # one IEEE double division, then the power of two
    return [int(v) if o else 0 for v, o in zip(q, ok)], m


def ess_of(q):
    Q = sum(q)
    hi = sum((a * a) >> 30 for a in q)
    lo = sum((a * a) & (SCALE - 1) for a in q)
    return (np.float64(Q) * np.float64(Q)) / (np.float64(hi) * np.float64(SCALE) + np.float64(lo))


def offset(Q, word):
    return (Q * int(word)) >> 32


def counts_closed(q, word):
    """c_i = N(P C_i) - N(P C_{i-1}), N(x) = 0 for x <= o, else min(P, (x - o + Q - 1) // Q)"""
    P, Q = len(q), sum(q)
    o = offset(Q, word)
    N = lambda x: 0 if x <= o else min(P, (x - o + Q - 1) // Q)  # noqa: E731
    c, C, below = [], 0, N(0)
    for a in q:
        C += a
        n = N(P * C)
        c.append(n - below)
        below = n
    return c


def counts_brute(q, word):
    """the same by walking the P positions j Q + o through the bounds P C_i"""
    P, Q = len(q), sum(q)
    o = offset(Q, word)
    bounds = np.cumsum([0] + list(q), dtype=object) * P
    c = [0] * P
    i = 0
    for j in range(P):
        pos = j * Q + o
        while not (bounds[i] <= pos < bounds[i + 1]):
            i += 1
        c[i] += 1
    return c


def map_of(c, base):
    """survivors keep their index; the k-th dead robot in index order takes the k-th extra slot in index order"""
    src = np.full(len(c), -1, np.int32)
    slots = [i for i, ci in enumerate(c) for _ in range(max(ci - 1, 0))]
    dead = [i for i, ci in enumerate(c) if ci == 0]
    assert len(slots) == len(dead)
    for d, s in zip(dead, slots):
        src[d] = base + s
    return src


def resample(weights, group_size=0, words=None, ess_gate=2.0):
    """(source int32[B], ess float32[G], status uint32[5]) of cdpr_resample_map_device"""
    w = np.asarray(weights, np.float32).ravel()
    B = len(w)
    P = int(group_size) or B
    assert B % P == 0
    G = B // P
    words = np.full(G, 1 << 31, np.uint64) if words is None else np.asarray(words, np.uint64)
    src, ess, st = np.full(B, -1, np.int32), np.zeros(G, np.float32), dict.fromkeys(STATUS, 0)
    st["bad"] = int((~(np.isfinite(w) & (w >= 0))).sum())
    for g in range(G):
        q, m = quantise(w[g * P:(g + 1) * P])
        if m is None:
            st["degenerate"] += 1
            continue
        e = ess_of(q)
        ess[g] = np.float32(e)
        if not (e < np.float64(np.float32(ess_gate)) * np.float64(P)):
            continue
        st["resampled"] += 1
        part = map_of(counts_closed(q, words[g]), g * P)
        src[g * P:(g + 1) * P] = part
        st["copied"] += int((part >= 0).sum())
    return src, ess, np.array([st[k] for k in STATUS], np.uint32)


def copy_rule_violation(source):
    """None where cdpr_copy_robots accepts the map: every destination's source is in range and is itself left as it is"""
    s = np.asarray(source, np.int64)
    dest = (s >= 0) & (s != np.arange(len(s)))
    if ((s[dest] >= len(s))).any():
        return "a source out of range"
    if dest[s[dest]].any():
        return "a source that is itself a destination"
    return None


# ---- weight patterns: name -> float32[G * P] -----------------------------------------------------------------------------------------
def pattern(name, P, G, seed=0):
    rng = np.random.default_rng([seed, P, G])
    w = np.ones((G, P), np.float32)
    if name == "uniform":
        pass
    elif name in ("one_hot_first", "one_hot_middle", "one_hot_last"):
        w[:] = 0
        w[:, {"one_hot_first": 0, "one_hot_middle": P // 2, "one_hot_last": P - 1}[name]] = 2.5
    elif name == "two_maxima":
        w[:] = rng.random((G, P), np.float32) * 0.5
        w[:, 0] = w[:, P - 1] = 0.75
    elif name == "heavy_tail":
        w[:] = rng.random((G, P), np.float32) ** np.float32(8)
    elif name == "zeros_mixed":  # most weights exactly zero
        w[:] = np.where(rng.random((G, P)) < 0.7, 0, rng.random((G, P), np.float32))
    elif name == "bad_mixed":  # NaN, +-inf, negative, -0 and a denormal among ordinary weights
        w[:] = rng.random((G, P), np.float32) ** np.float32(3)
        bad = np.array([np.nan, np.inf, -np.inf, -1.0, -0.0, 1e-42], np.float32)
        flat = w.reshape(-1)
        at = rng.choice(flat.size, min(flat.size, 2 * len(bad) * G) // 2, replace=False)
        flat[at] = bad[np.arange(len(at)) % len(bad)]
    elif name == "zero_group_next_to_normal":  # even groups all zero (degenerate)
        w[:] = rng.random((G, P), np.float32)
        w[::2] = 0
    elif name == "gate_split":  # even groups nearly uniform (ess ~ P), odd groups one-hot (ess = 1)
        w[:] = 1.0 + 0.01 * rng.random((G, P), np.float32)
        w[1::2] = 0
        w[1::2, P // 3] = 1.0
    else:
        raise KeyError(name)
    return w.reshape(-1)


PATTERNS = ("uniform", "one_hot_first", "one_hot_middle", "one_hot_last", "two_maxima", "heavy_tail", "zeros_mixed", "bad_mixed",
            "zero_group_next_to_normal", "gate_split")
WORDS = (0, 1 << 31, (1 << 32) - 1)
