"""cdpr_resample_map_device / cdpr_resample_device, the CPU side: the definition's own invariants on the sequential restatement
(tests/resample_oracle.py) that tests/test_gpu_resample.py holds the kernels to, the bindings, the sharded wrapper.  No GPU.

  1. the closed form of the offspring counts equals the brute-force walk of the positions; sum c = P; |c_i - P q_i / Q| < 1 -
     P = 1, 2, 3, 64, 65, 130, 257, every weight pattern, the words 0, 2^31, 2^32 - 1 and random ones.
  2. every map the restatement makes passes the rule of cdpr_copy_robots (sources in range and not themselves destinations), the
     destinations are exactly the dead robots and the sources carry exactly their extras.
  3. the degenerate group, the bad weights and the gate behave as defined.
  4. the bindings exist and cdpr_resample_spec_size() is the ctypes mirror's sizeof; a NULL handle is refused without a GPU.
  5. ShardedEngine.resample splits by the spans, re-bases the map, sums the status; a straddling group raises before any shard is called.
"""
import ctypes as C

import numpy as np
import pytest

import resample_oracle as ro

SIZES = (1, 2, 3, 64, 65, 130, 257)


@pytest.mark.parametrize("P", SIZES)
def test_closed_form_is_the_brute_force_count(P):
    rng = np.random.default_rng(P)
    G = 3
    for name in ro.PATTERNS:
        w = ro.pattern(name, P, G, seed=1).reshape(G, P)
        for g in range(G):
            q, m = ro.quantise(w[g])
            if m is None:
                assert not any(q)  # (a degenerate group: no counts to take)
                continue
            assert max(q) == ro.SCALE  # the maximum becomes exactly 2^30
            Q = sum(q)
            for word in ro.WORDS + tuple(int(x) for x in rng.integers(0, 1 << 32, 2, dtype=np.uint64)):
                c = ro.counts_closed(q, word)
                assert c == ro.counts_brute(q, word), (name, P, word)
                assert sum(c) == P
                assert all(abs(ci * Q - P * qi) < Q for ci, qi in zip(c, q)), (name, P, word)  # |c_i - P q_i / Q| < 1, in integers


@pytest.mark.parametrize("P", SIZES)
def test_every_map_passes_the_copy_rule(P):
    G = 4
    for name in ro.PATTERNS:
        w = ro.pattern(name, P, G, seed=2)
        for word in ro.WORDS:
            src, ess, st = ro.resample(w, P, np.full(G, word, np.uint64))
            assert ro.copy_rule_violation(src) is None, (name, P, word)
            dest = src >= 0
            assert st[0] == dest.sum() and st[1] == 0
            assert ((src[dest] // P) == (np.flatnonzero(dest) // P)).all()  # a source is of the destination's own group
            for g in range(G):
                q, m = ro.quantise(w[g * P:(g + 1) * P])
                if m is None:
                    assert not dest[g * P:(g + 1) * P].any() and ess[g] == 0
                    continue
                c = np.array(ro.counts_closed(q, word))
                part = src[g * P:(g + 1) * P]
                assert ((part >= 0) == (c == 0)).all()
                assert (np.bincount(part[part >= 0] - g * P, minlength=P) == np.maximum(c - 1, 0)).all()
                assert 1.0 - 1e-6 <= ess[g] <= P * (1 + 1e-6)


def test_uniform_weights_are_the_identity_and_word_zero_sits_on_the_bounds():
    for P in SIZES:
        for word in ro.WORDS:  # (word 0: every position j Q lies exactly on the bound P C_{j-1})
            src, ess, st = ro.resample(np.full(2 * P, 0.3, np.float32), P, [word, word])
            assert (src == -1).all() and (ess == P).all() and list(st) == [0, 0, 2, 0, 0]


def test_degenerate_groups_bad_weights_and_the_gate():
    P = 65
    w = ro.pattern("bad_mixed", P, 2)
    w[:P] = [np.nan, -np.inf, -2.0, -0.0, 0.0] * (P // 5)  # no usable weight: 3 of 5 are bad, -0 and 0 are zeros
    src, ess, st = ro.resample(w, P)
    bad = int((~(np.isfinite(w) & (w >= 0))).sum())
    assert (src[:P] == -1).all() and ess[0] == 0 and st[3] == 1 and st[2] == 1 and st[4] == bad and bad > 3 * (P // 5)
    w = ro.pattern("gate_split", P, 4)
    src, ess, st = ro.resample(w, P, ess_gate=0.5)
    assert (ess[0::2] > 0.99 * P).all() and (ess[1::2] == 1).all()
    assert st[2] == 2 and (src.reshape(4, P)[0::2] == -1).all() and ((src.reshape(4, P)[1::2] >= 0).sum(axis=1) == P - 1).all()
    assert ro.resample(w, P, ess_gate=0.0)[2][2] == 0 and ro.resample(w, P, ess_gate=2.0)[2][2] == 4
    one = ro.resample(np.float32([1.0, 0.0, 0.0, 0.0]), 0)  # group_size 0: the whole batch
    assert list(one[0]) == [-1, 0, 0, 0] and one[1][0] == 1 and list(one[2]) == [3, 0, 1, 0, 0]


def test_bindings(pkg):
    from cdpr_simulation_amd._native import EXPORTS, lib

    assert {"cdpr_resample_spec_size", "cdpr_resample_map_device", "cdpr_resample_device"} <= set(EXPORTS)
    assert lib().cdpr_resample_spec_size() == C.sizeof(pkg._abi.ResampleSpec) == 16
    assert lib().cdpr_abi_version() == 8
    s = pkg.ResampleSpec()
    assert (s.struct_size, s.group_size, s.ess_gate, s.flags) == (16, 0, 2.0, 0)
    s = pkg.ResampleSpec(group_size=65, ess_gate=0.5)
    assert (s.struct_size, s.group_size, s.ess_gate, s.flags) == (16, 65, 0.5, 0)
    assert lib().cdpr_resample_map_device(None, C.byref(s), None, None, None, None, None) == pkg._abi.ERR_INVALID
    assert lib().cdpr_resample_device(None, C.byref(s), None, None, None, None, None) == pkg._abi.ERR_INVALID
    for name in ("resample_map_device", "resample_device", "resample"):
        assert hasattr(pkg.Engine, name)
    assert hasattr(pkg.ShardedEngine, "resample") and pkg._abi.RESAMPLE_STATUS == len(ro.STATUS)


class StubEngine:
    """an Engine.resample that answers from the restatement and records what it was asked"""

    def __init__(self):
        self.calls = []

    def resample(self, weights, words=None, group_size=0, ess_gate=2.0, copy=True):
        self.calls.append((np.array(weights), None if words is None else np.array(words), group_size, ess_gate, copy))
        return ro.resample(weights, group_size, words, ess_gate)


def sharded(pkg, B, devices):
    from cdpr_simulation_amd.sharding import ShardedEngine, shard_range

    sh = object.__new__(ShardedEngine)  # (no GPU: the per-device engines are stubs)
    sh.B, sh.n = B, 8
    sh.spans = [shard_range(i, devices, B) for i in range(devices)]
    sh.engines = [StubEngine() for _ in range(devices)]
    return sh


def test_sharded_resample_splits_and_rebases(pkg):
    P, G = 13, 6
    w = ro.pattern("heavy_tail", P, G, seed=3)
    words = np.random.default_rng(4).integers(0, 1 << 32, G, dtype=np.uint64).astype(np.uint32)
    for devices in (1, 2, 3):
        sh = sharded(pkg, P * G, devices)
        got = sh.resample(w, words, P, 1.5, copy=False)
        want = ro.resample(w, P, words, 1.5)
        assert all(np.array_equal(g, x) for g, x in zip(got, want)), devices
        assert got[0].dtype == np.int32 and got[2].dtype == np.uint32 and want[2][0] > 0
        for e, (lo, hi) in zip(sh.engines, sh.spans):
            (pw, pu, p, gate, copy), = e.calls
            assert np.array_equal(pw, w[lo:hi]) and np.array_equal(pu, words[lo // P:hi // P]) and (p, gate, copy) == (P, 1.5, False)
    sh = sharded(pkg, P * G, 2)
    assert np.array_equal(sh.resample(w, None, P)[0], ro.resample(w, P)[0]) and sh.engines[0].calls[0][1] is None


def test_sharded_resample_refuses_a_straddling_group(pkg):
    sh = sharded(pkg, 130, 2)  # spans [0, 65), [65, 130)
    w = np.ones(130, np.float32)
    for P in (0, 130, 26, 10):
        with pytest.raises(ValueError, match="straddles"):
            sh.resample(w, None, P)
    with pytest.raises(ValueError, match="whole number"):
        sh.resample(w, None, 7)
    assert not any(e.calls for e in sh.engines)
    sh.resample(w, None, 65), sh.resample(w, None, 13)
    assert all(len(e.calls) == 2 for e in sh.engines)
