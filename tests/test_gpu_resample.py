"""cdpr_resample_map_device / cdpr_resample_device: systematic resampling per group of P consecutive robots on the device, float weights
to the int32 source map of cdpr_copy_robots_device.  In every case the map, the bits of ess and all five status words EQUAL the
sequential restatement of the definition (tests/resample_oracle.py): nothing in the definition depends on the order of a sum, so
there is no tolerance anywhere in this file.

Group sizes.  The kernel has three forms (csrc/cdpr_resample.hpp) and the host one more switch; the sizes sit on both sides of each:
  P <= 64            a wave per group, four groups per workgroup                       63, 64 | 65
  P <= 1 024         a workgroup per group, weights in registers (4 robots per lane)   1 024 | 1 025
  P <= 65 536        the workgroup walks chunks of 1 024 with carries                  2 048 | 2 049: a whole number of chunks or not
  2 P > 64 KiB       the launch asks for its dynamic LDS by attribute                  32 768 | 32 769
and 1, 2, 130 (one group, and 2 x 65), 256, 257, 1 040, and 65 536 once.  G runs from 1 to counts that take several workgroups, with
spare waves in the last workgroup of the wave form (G = 9: three workgroups, three spare waves).

  1  the matrix: every weight pattern x the words NULL, 0, 2^31, 2^32 - 1 and random ones, on bare handles without FK (map form).
  2  the gate: groups clearly under and clearly over ess_gate * P in one call.
  3  the caller's buffers: only [0, B) of the map and [0, G) of ess are written; a NULL d_ess or d_status changes nothing else.
  4  the fused form on one handle per record layout, B = 130, P = 65, after a history: against copy_robots(the restatement's map) on a
     twin, every getter to the bit right after and after more steps; the handle's own map buffer.
  5  refusals.  6  two shards on one device, and the straddling group.
"""
import ctypes as C

import numpy as np
import pytest

import resample_oracle as ro
import robot_histories as ri
from parity import engines, equal_rows, every_getter
from per_robot_kinds import LAYOUTS, clean_env, config_of  # noqa: F401  (clean_env: autouse here too)

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
SMALL = [(1, 1), (1, 300), (2, 5), (63, 5), (64, 4), (64, 9), (65, 2), (130, 1), (256, 3), (257, 2), (1024, 2), (1025, 1), (1040, 2)]
LARGE = [(2048, 1), (2049, 2), (32768, 1), (32769, 1), (65536, 1)]


@pytest.fixture(scope="module")
def bare(pkg):
    """bare(B): a uniform four-cable handle without FK or TD of B robots - the map form reads no robot state; one per batch size"""
    made = {}

    def get(B):
        if B not in made:
            made[B] = pkg.Engine(pkg.Config(model=pkg.cube_model(), batch=B, stages=0), 0)
        return made[B]

    yield get
    for e in made.values():
        e.close()


def agree(got, want, where):
    for name, g, w in zip(("map", "ess", "status"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (where, name)
        same = np.array_equal(g.view(np.uint32), w.view(np.uint32))  # (ess: the bits)
        assert same, f"{where}: {name} differs from the restatement at {np.flatnonzero(g.view(np.uint32) != w.view(np.uint32))[:8]}: {g.ravel()[:8]} / {w.ravel()[:8]}"


def word_sets(G, seed):
    rng = np.random.default_rng(seed)
    return [None] + [np.full(G, x, np.uint32) for x in ro.WORDS] + [rng.integers(0, 1 << 32, G, dtype=np.uint64).astype(np.uint32)]


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,G", SMALL)
def test_matrix(bare, P, G):
    eng = bare(P * G)
    for name in ro.PATTERNS:
        w = ro.pattern(name, P, G, seed=5)
        for k, words in enumerate(word_sets(G, P + G)):
            agree(eng.resample(w, words, P, copy=False), ro.resample(w, P, words), f"P {P}, G {G}, {name}, words {k}")
    # NULL words are 2^31; group_size 0 is the whole batch
    w = ro.pattern("heavy_tail", P, G, seed=6)
    agree(eng.resample(w, None, P, copy=False), ro.resample(w, P, np.full(G, 1 << 31, np.uint32)), f"P {P}: NULL words")
    agree(eng.resample(w, None, 0, copy=False), ro.resample(w, P * G), f"P {P}: group_size 0")


@pytest.mark.parametrize("P,G", LARGE)
def test_large_groups(bare, P, G):
    eng = bare(P * G)
    rng = np.random.default_rng(P)
    for name in ("heavy_tail", "one_hot_last", "bad_mixed", "uniform"):
        w = ro.pattern(name, P, G, seed=7)
        words = rng.integers(0, 1 << 32, G, dtype=np.uint64).astype(np.uint32) if name != "uniform" else np.zeros(G, np.uint32)
        want = ro.resample(w, P, words)
        agree(eng.resample(w, words, P, copy=False), want, f"P {P}, G {G}, {name}")
        assert name != "one_hot_last" or want[2][0] == G * (P - 1)


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,G", [(3, 4), (65, 4), (1040, 2), (2049, 2)])  # (a one-hot group has ess 1: under 0.5 P from P = 3 on)
def test_gate(bare, P, G):
    eng = bare(P * G)
    w = ro.pattern("gate_split", P, G)
    for gate in (0.5, 0.0, 2.0, 1.0):
        want = ro.resample(w, P, None, gate)
        agree(eng.resample(w, None, P, gate, copy=False), want, f"P {P}, gate {gate}")
    want = ro.resample(w, P, None, 0.5)
    assert want[2][2] == G // 2 and (want[1][0::2] > 0.99 * P).all() and (want[1][1::2] == 1).all()  # (one under, one over, in one call)


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,G", [(5, 7), (65, 2), (1040, 1), (2049, 1)])
def test_callers_buffers(pkg, bare, P, G):
    B, pad = P * G, 64
    eng = bare(B)
    w = ro.pattern("heavy_tail", P, G, seed=8)
    words = np.random.default_rng(9).integers(0, 1 << 32, G, dtype=np.uint64).astype(np.uint32)
    want = ro.resample(w, P, words)
    spec = pkg.ResampleSpec(P)
    d_w, d_u = eng.device_upload(w), eng.device_upload(words)
    d_map, d_ess = eng.device_upload(np.full(B + 2 * pad, POISON, np.uint32)), eng.device_upload(np.full(G + 2 * pad, POISON, np.uint32))
    d_status = eng.device_upload(np.full(5 + 2 * pad, POISON, np.uint32))
    eng.resample_map_device(spec, d_w, d_map + 4 * pad, d_u, d_ess + 4 * pad, d_status + 4 * pad)
    got_map, got_ess, got_status = (eng.device_download(d, n + 2 * pad, np.uint32) for d, n in ((d_map, B), (d_ess, G), (d_status, 5)))
    for name, got, n in (("map", got_map, B), ("ess", got_ess, G), ("status", got_status, 5)):
        assert (got[:pad] == POISON).all() and (got[pad + n:] == POISON).all(), f"P {P}: {name} written outside its range"
    agree((got_map[pad:pad + B].view(np.int32), got_ess[pad:pad + G].view(np.float32), got_status[pad:pad + 5]), want, f"P {P}, offset buffers")
    # NULL d_ess, NULL d_status, both: the map is the same and the other output too
    for with_ess, with_status in ((False, True), (True, False), (False, False)):
        eng.device_upload_into(d_map, np.full(B + 2 * pad, POISON, np.uint32))
        eng.device_upload_into(d_ess, np.full(G + 2 * pad, POISON, np.uint32))
        eng.device_upload_into(d_status, np.full(5 + 2 * pad, POISON, np.uint32))
        eng.resample_map_device(spec, d_w, d_map + 4 * pad, d_u, d_ess + 4 * pad if with_ess else 0, d_status + 4 * pad if with_status else 0)
        assert np.array_equal(eng.device_download(d_map + 4 * pad, B, np.int32), want[0])
        got_ess, got_status = eng.device_download(d_ess + 4 * pad, G, np.float32), eng.device_download(d_status + 4 * pad, 5, np.uint32)
        assert np.array_equal(got_ess.view(np.uint32), want[1].view(np.uint32)) if with_ess else (got_ess.view(np.uint32) == POISON).all()
        assert np.array_equal(got_status, want[2]) if with_status else (got_status == POISON).all()
    for d in (d_w, d_u, d_map, d_ess, d_status):
        eng.device_free(d)


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", LAYOUTS)
def test_fused(pkg, monkeypatch, kind):
    cfg = config_of(pkg, kind, monkeypatch)
    B, P = cfg.batch, 65
    assert B == 130
    h = ri.history_inputs(cfg.model, 191)
    eng, own, twin = engines(pkg, cfg, h["pose"], 3)
    ri.play_history([eng, own, twin], h, 12)
    w = ro.pattern("heavy_tail", P, 2, seed=10)
    w[3], w[70] = np.nan, -1.0
    words = np.array([123456789, 4000000000], np.uint32)
    want = ro.resample(w, P, words)
    assert want[2][0] > 20 and ro.copy_rule_violation(want[0]) is None
    got = eng.resample(w, words, P)  # the fused form: map, then the copy kernel's own counts in [0] and [1]
    agree(got, want, f"{kind}: fused")
    assert got[2][1] == 0
    # the handle's own map buffer, no ess, the status
    d_w, d_u, d_status = own.device_upload(w), own.device_upload(words), own.device_upload(np.full(5, POISON, np.uint32))
    own.resample_device(pkg.ResampleSpec(P), d_w, 0, d_u, 0, d_status)
    assert np.array_equal(own.device_download(d_status, 5, np.uint32), want[2])
    twin.copy_robots(want[0])
    for label, steps in (("right after the call", 0), ("4 steps on", 4), ("9 steps on", 5)):
        for e in (eng, own, twin):
            e.update(steps) if steps else None
        ref = every_getter(twin, cfg, pkg)
        for name, e in (("resample", eng), ("resample_device, own map", own)):
            assert equal_rows(every_getter(e, cfg, pkg), ref, slice(None), slice(None)), f"{kind}, {name}, {label}: differs from copy_robots(the restatement's map)"
    dest = want[0] >= 0
    assert equal_rows(ref, ref, dest, want[0][dest])  # (and a destination still is its source: same commands since)
    for d in (d_w, d_u, d_status):
        own.device_free(d)
    for e in (eng, own, twin):
        e.close()


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg, monkeypatch, bare):
    from cdpr_simulation_amd._native import lib

    L, INVALID, UNSUPPORTED = lib(), pkg._abi.ERR_INVALID, pkg._abi.ERR_UNSUPPORTED
    B = 130
    w = ro.pattern("heavy_tail", 65, 2)

    def refusals_of(call, eng, d_w, d_map):
        """every refusal of the list through `call` (one of the two exports); the map buffer stays poisoned"""
        vp = lambda x: C.c_void_p(x) if x else None  # noqa: E731
        good = pkg.ResampleSpec(65)
        go = lambda spec, dw=d_w, dm=d_map: call(eng._h, C.byref(spec) if spec is not None else None, vp(dw), None, vp(dm), None, None)  # noqa: E731
        assert call(None, C.byref(good), vp(d_w), None, vp(d_map), None, None) == INVALID
        assert go(None) == INVALID and b"null spec" in L.cdpr_last_error(eng._h)
        assert go(good, 0) == INVALID and b"null weights" in L.cdpr_last_error(eng._h)
        wrong = pkg.ResampleSpec(65)
        wrong.struct_size = 12
        assert go(wrong) == INVALID and b"struct_size" in L.cdpr_last_error(eng._h)
        assert go(pkg.ResampleSpec(65, flags=1)) == INVALID and b"flags" in L.cdpr_last_error(eng._h)
        for P in (7, 131, 260, 1 << 20):
            assert go(pkg.ResampleSpec(P)) == INVALID and b"whole number" in L.cdpr_last_error(eng._h)
        for gate in (float("nan"), -1.0, -1e-30):
            assert go(pkg.ResampleSpec(65, gate)) == INVALID and b"ess_gate" in L.cdpr_last_error(eng._h)
        assert (eng.device_download(d_map, B, np.uint32) == POISON).all(), "a refused call wrote the map"

    # a uniform handle: the map form works, the fused form is refused
    eng = bare(B)
    d_w, d_map = eng.device_upload(w), eng.device_upload(np.full(B, POISON, np.uint32))
    refusals_of(L.cdpr_resample_map_device, eng, d_w, d_map)
    assert L.cdpr_resample_map_device(eng._h, C.byref(pkg.ResampleSpec(65)), C.c_void_p(d_w), None, None, None, None) == INVALID
    assert b"null source map" in L.cdpr_last_error(eng._h)
    with pytest.raises(pkg.CdprError) as ei:
        eng.resample_device(pkg.ResampleSpec(65), d_w, d_map)
    assert ei.value.code == UNSUPPORTED and "per_robot_commands" in str(ei.value)
    with pytest.raises(pkg.CdprError) as ei:
        eng.resample(w, None, 65)  # (copy=True)
    assert ei.value.code == UNSUPPORTED
    assert (eng.device_download(d_map, B, np.uint32) == POISON).all()
    eng.resample_map_device(pkg.ResampleSpec(65), d_w, d_map)
    assert np.array_equal(eng.device_download(d_map, B, np.int32), ro.resample(w, 65)[0])
    eng.device_free(d_w), eng.device_free(d_map)
    # more than 65 536 robots in a group
    big = bare(1 << 17)
    d_w, d_map = big.device_upload(np.ones(1 << 17, np.float32)), big.device_upload(np.full(1 << 17, POISON, np.uint32))
    for P in (0, 1 << 17):
        with pytest.raises(pkg.CdprError) as ei:
            big.resample_map_device(pkg.ResampleSpec(P), d_w, d_map)
        assert ei.value.code == UNSUPPORTED and "65 536" in str(ei.value)
    assert (big.device_download(d_map, 1 << 17, np.uint32) == POISON).all()
    big.resample_map_device(pkg.ResampleSpec(1 << 16), d_w, d_map)
    assert (big.device_download(d_map, 1 << 17, np.int32) == -1).all()
    big.device_free(d_w), big.device_free(d_map)
    # a per-robot handle: a refused fused call leaves the map and the robots as they were
    cfg = config_of(pkg, "fast_n8", monkeypatch)
    h = ri.history_inputs(cfg.model, 195)
    eng, twin = engines(pkg, cfg, h["pose"], 2)
    ri.play_history([eng, twin], h, 8)
    d_w, d_map = eng.device_upload(w), eng.device_upload(np.full(B, POISON, np.uint32))
    refusals_of(L.cdpr_resample_device, eng, d_w, d_map)
    assert equal_rows(every_getter(eng, cfg, pkg), every_getter(twin, cfg, pkg), slice(None), slice(None)), "a refused call changed a robot"
    eng.update(3), twin.update(3)
    assert equal_rows(every_getter(eng, cfg, pkg), every_getter(twin, cfg, pkg), slice(None), slice(None))
    eng.device_free(d_w), eng.device_free(d_map)
    eng.close(), twin.close()


# ---- 6 -------------------------------------------------------------------------------------------------------------------------
def test_sharded(pkg, monkeypatch):
    cfg = config_of(pkg, "fast_n8", monkeypatch)
    h = ri.history_inputs(cfg.model, 197)
    one = pkg.Engine(cfg, 0)
    sh = pkg.ShardedEngine(cfg, devices=[0, 0])
    assert [hi - lo for lo, hi in sh.spans] == [65, 65]
    one.set_platform_state(pose7=h["pose"]), sh.set_platform_state(pose7=h["pose"])
    ri.play_history([one, sh], h, 6)
    rng = np.random.default_rng(11)
    for P in (13, 65):
        w = ro.pattern("heavy_tail", P, 130 // P, seed=P)
        words = rng.integers(0, 1 << 32, 130 // P, dtype=np.uint64).astype(np.uint32)
        want = ro.resample(w, P, words)
        agree(sh.resample(w, words, P), want, f"two shards on one device, P {P}")
        agree(one.resample(w, words, P), want, f"one engine, P {P}")
        assert want[2][0] > 0
        one.update(2), sh.update(2)
        assert all(np.array_equal(a, b) for a, b in zip(sh.raw_state() + sh.joint_states(), one.raw_state() + one.joint_states()))
    before = sh.raw_state()
    for P in (0, 130, 26):
        with pytest.raises(ValueError, match="straddles"):
            sh.resample(np.ones(130, np.float32), None, P)
    assert all(np.array_equal(a, b) for a, b in zip(sh.raw_state(), before))
    sh.close(), one.close()
