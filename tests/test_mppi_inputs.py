"""CPU checks of what tests/test_gpu_mppi.py stands on (tests/mppi_oracle.py): the restated Philox against the known answers, the
statistics of its normals, the independence of streams, the shard rule, the teeth and the size of the update's bounds, and the refusal
table against the text of include/cdpr.h."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mppi_oracle as mo
from cdpr_simulation_amd._abi import MPPI_CLAMP, MPPI_NOMINAL_FIRST, MPPI_SHIFT, MppiSpec  # (the restatement's flags are the ABI's)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_philox_known_answers():
    for counter, key, want in mo.KNOWN_ANSWERS:
        assert tuple(int(x) for x in mo.philox(*counter, *key)) == want
    # ... and vectorised: the same words from arrays of counters
    got = mo.philox(*(np.array([c[k] for c, _, _ in mo.KNOWN_ANSWERS[::2]]) for k in range(4)), 0, 0)
    assert tuple(int(x[0]) for x in got) == mo.KNOWN_ANSWERS[0][2]


def test_normal_statistics():
    N = 1 << 20
    z = mo.normals(N, 5, 3, 0x12345678, 0x9ABCDEF0)
    assert abs(z.mean()) < 4 / np.sqrt(N)
    assert abs(z.var() - 1) < 0.01
    assert abs((z ** 4).mean() - 3) < 0.05
    assert abs(np.corrcoef(z[:-1], z[1:])[0, 1]) < 4 / np.sqrt(N)
    assert np.abs(z).max() <= 5.65
    # the extremes of the definition: u1 = 2^-23 gives the largest radius, u1 = 1 gives 0
    far, _ = mo.box_muller(np.array([0], np.uint64), np.array([0], np.uint64))
    near, _ = mo.box_muller(np.array([0xFFFFFFFF], np.uint64), np.array([0], np.uint64))
    assert 5.64 < far[0] <= 5.65 and near[0] == 0.0


def test_streams_share_no_group():
    groups = 4096
    seen = {}
    for name, (g, it, lo, hi) in {"base": (7, 0, 1, 2), "iteration": (7, 1, 1, 2), "robot": (8, 0, 1, 2), "seed_lo": (7, 0, 3, 2), "seed_hi": (7, 0, 1, 3)}.items():
        words = mo.group_words(groups, g, it, lo, hi)
        seen[name] = {tuple(int(x) for x in row) for row in words}
        assert len(seen[name]) == groups, f"{name}: a group of words repeats within the stream"
    names = list(seen)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert not (seen[a] & seen[b]), f"{a} and {b} share a group of words"


def test_shard_equals_rows_of_the_whole_batch():
    rng = np.random.default_rng(3)
    B, H, S, n = 7, 3, 5, 3
    U = rng.uniform(-0.05, 0.05, (B, H, n)).astype(np.float32)
    whole, _, _ = mo.sample(U, S, 0.01, mo.NOMINAL_FIRST, iteration=9, seed_lo=4, seed_hi=5, robot_offset=100)
    for lo, hi in ((0, 3), (3, 7)):
        part, _, _ = mo.sample(U[lo:hi], S, 0.01, mo.NOMINAL_FIRST, iteration=9, seed_lo=4, seed_hi=5, robot_offset=100 + lo)
        assert np.array_equal(part, whole[lo:hi])
    other, _, _ = mo.sample(U[3:], S, 0.01, mo.NOMINAL_FIRST, iteration=9, seed_lo=4, seed_hi=5, robot_offset=100)
    assert not np.array_equal(other, whole[3:])
    # the global index wraps modulo 2^32
    a, _, _ = mo.sample(U[:1], S, 0.01, robot_offset=(1 << 32) + 5)
    b, _, _ = mo.sample(U[:1], S, 0.01, robot_offset=5)
    assert np.array_equal(a, b)


def cases():
    return [(p, shape) for p in mo.PATTERNS for shape in mo.UPDATE_SHAPES]


@pytest.mark.parametrize("pattern,shape", cases(), ids=lambda v: str(v))
def test_update_bound_has_teeth_and_is_small(pattern, shape):
    """Dropping the heaviest sample, or swapping the costs of the best and the worst usable sample, moves every robot's plan by more than
    four times the bound (the swap: where those two weights differ by more than 1e-3; with equal weights a swap changes nothing, as under
    the huge temperature); and the bound stays under 1e-5 max |v|."""
    cost, V, U, T = mo.update_inputs(pattern, *shape)
    S = shape[0]
    for shift in (False, True):
        ref = mo.update(cost, V, U, T, shift)
        vmax = np.abs(V[np.isfinite(V)]).max()
        assert ref["plan_bound"].max() < 1e-5 * vmax and ref["action_bound"].max() < 1e-5 * vmax
        assert (ref["weights_bound"] <= 1e-5).all()
        assert np.isfinite(ref["plan"]).all() and np.isfinite(ref["ess"]).all()
        W = ref["weights"]
        alive = np.isfinite(cost).any(axis=1)
        # drop the heaviest sample: its cost becomes NaN (weight 0 by definition)
        dropped = cost.copy()
        dropped[np.arange(len(cost)), W.argmax(axis=1)] = np.nan
        got = mo.update(dropped, V, U, T, shift)
        moved = np.abs(got["plan"] - ref["plan"]).max(axis=(1, 2))
        assert (moved[alive] > 4 * ref["plan_bound"].max(axis=(1, 2))[alive]).all(), f"{pattern} {shape}: dropping a sample hides inside the bound"
        # swap the costs of the best and the worst usable sample
        if S > 1:
            masked = np.where(np.isfinite(cost), W, np.inf)
            best, worst = W.argmax(axis=1), masked.argmin(axis=1)
            rows = np.arange(len(cost))
            differ = alive & (W[rows, best] - W[rows, worst] > 1e-3)
            swapped = cost.copy()
            swapped[rows, best], swapped[rows, worst] = cost[rows, worst], cost[rows, best]
            got = mo.update(swapped, V, U, T, shift)
            moved = np.abs(got["plan"] - ref["plan"]).max(axis=(1, 2))
            # (a NaN command that the swap brings into the plan counts as moved)
            assert not (moved[differ] <= 4 * ref["plan_bound"].max(axis=(1, 2))[differ]).any(), f"{pattern} {shape}: swapping two costs hides inside the bound"
            assert differ.any() or pattern in ("plain_mean", "one_robot_all_bad")


def test_update_patterns_are_what_they_claim():
    S, H, n, B = 129, 4, 8, 130
    cost, V, U, T = mo.update_inputs("clear_minimum", S, H, n, B)
    r = mo.update(cost, V, U, T)
    best = cost.argmin(axis=1)
    assert np.array_equal(r["action"].astype(np.float32), V[np.arange(B), 0, best, :]) and (r["ess"] == 1).all()
    cost, V, U, T = mo.update_inputs("plain_mean", S, H, n, B)
    assert (mo.update(cost, V, U, T)["weights"].astype(np.float32) == 1).all()
    cost, V, U, T = mo.update_inputs("one_robot_all_bad", S, H, n, B)
    r = mo.update(cost, V, U, T, shift=True)
    assert r["status"][1] == 1 and np.array_equal(r["plan"][B // 2, :-1], U[B // 2, 1:]) and np.array_equal(r["plan"][B // 2, -1], U[B // 2, -1])
    cost, V, U, T = mo.update_inputs("nan_behind_zero", S, H, n, B)
    r = mo.update(cost, V, U, T)
    assert np.isnan(V).any() and np.isfinite(r["plan"]).all()
    assert (r["weights"].astype(np.float32)[np.isnan(V).any(axis=(1, 3))] == 0).all()
    cost, V, U, T = mo.update_inputs("heavy_tail", S, H, n, B)
    w = mo.update(cost, V, U, T)["weights"].astype(np.float32)
    assert (w == 0).any() and ((w > 0) & (w < 1e-30)).any() and (w == 1).any()


def refusal_paragraph():
    text = open(os.path.join(ROOT, "include", "cdpr.h")).read()
    m = re.search(r"MPPI on the device:.*?Refusals \(a refused call queues nothing\):(.*?)\*/", text, flags=re.S)
    assert m, "the MPPI refusals are not in include/cdpr.h"
    return re.sub(r"\s*\n \*\s*", " ", m.group(1)).strip()


def test_refusal_table_is_the_headers():
    """Every clause of the header's refusal list is in mo.REFUSALS with its code, and nothing else is in the text."""
    text = refusal_paragraph()
    invalid, unsupported = re.fullmatch(r"CDPR_ERR_INVALID for (.*); CDPR_ERR_UNSUPPORTED for (.*)\.", text).groups()
    rest = {"INVALID": invalid, "UNSUPPORTED": unsupported}
    for words, code, calls, _ in mo.REFUSALS:
        assert words in rest[code], f"'{words}' is not among the header's {code} refusals"
        rest[code] = rest[code].replace(words, "", 1)
        assert calls in ("both", "update")
    for code, left in rest.items():
        assert not re.sub(r"[,\s]", "", left), f"the header refuses more than the table ({code}): {left!r}"


def test_spec_layout(pkg):
    from cdpr_simulation_amd._native import lib

    assert lib().cdpr_mppi_spec_size() == C.sizeof(pkg._abi.MppiSpec) == 48
    s = pkg.MppiSpec(samples=3, horizon=2, flags=pkg._abi.MPPI_CLAMP | pkg._abi.MPPI_SHIFT, sigma=0.5, cmd_min=-1, cmd_max=1, temperature=2, seed=(7 << 32) | 9, robot_offset=11)
    assert (s.struct_size, s.samples, s.horizon, s.flags, s.seed_lo, s.seed_hi, s.robot_offset, s.reserved) == (48, 3, 2, 6, 9, 7, 11, 0)
    t = s.with_offset((1 << 32) - 1)
    assert t.robot_offset == 10 and s.robot_offset == 11 and t.samples == 3
    assert (mo.NOMINAL_FIRST, mo.CLAMP, mo.SHIFT) == (MPPI_NOMINAL_FIRST, MPPI_CLAMP, MPPI_SHIFT) and pkg.MppiSpec is MppiSpec
    # no device is needed to be refused: a NULL handle
    assert lib().cdpr_mppi_sample_device(None, C.byref(s), 0, None, None) == pkg._abi.ERR_INVALID
    assert lib().cdpr_mppi_update_device(None, C.byref(s), None, None, None, None, None, None, None) == pkg._abi.ERR_INVALID
