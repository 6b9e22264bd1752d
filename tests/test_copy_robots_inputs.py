"""cdpr_copy_robots, the CPU side: the oracle-side condition of tests/test_gpu_copy_robots.py, the test map, the sharded wrapper.

The oracle has no copy and needs none: its robots are index-independent.  An oracle whose input rows of destination d (start pose, the
three commands, mode group) are those of its source s FROM THE START holds in robot d, at every step, what robot s of the plain oracle
holds - to the bit.  This "twin from birth" is what a copied engine is compared with on the GPU; here it is established as a yardstick.

  1. twin from birth = source, to the bit, on n8_fk_td, n8_fk_td_hold and n4, through the 37-step history and the script behind it.
  2. copy_map(): the properties the GPU tests rely on; validate_map accepts it and refuses a chain and an index >= B.
  3. ShardedEngine.copy_robots slices and re-bases the map as shard_range says; a cross-shard source raises before any shard is called.
  4. both exports are in the prototype table; a null handle is refused without a GPU.
"""
import ctypes as C

import numpy as np
import pytest

import copy_robots as cr
import robot_histories as ri

B = ri.B


@pytest.mark.parametrize("name", list(ri.CONFIGS))
def test_the_oracles_robots_are_index_independent(pkg, oracle, name):
    n, kw = ri.CONFIGS[name]
    model = ri.model_of(pkg, n)
    cfg = pkg.Config(model=model, batch=B, perRobotCommands=True, **kw)
    source = cr.copy_map()
    dest = cr.destinations_of(source)
    h, a = ri.history_inputs(model, 111), ri.after_inputs(model, 112)
    plain, twin = (oracle.OracleSim(cfg.to_struct(), oracle.DERIV_EXACT) for _ in range(2))
    runs = ((plain, h, a), (twin, cr.twin_rows(h, source), cr.twin_rows(a, source)))
    for sim, hh, _ in runs:
        sim.set_platform_state(pose7=hh["pose"].astype(np.float64))
        ri.play_history([sim], hh)
    checkpoints = {}

    def record(sim):
        def check(label):
            checkpoints.setdefault(label, []).append(sim.raw_state() + sim.platform_state() + sim.joint_states())
        return check

    for sim, _, aa in runs:
        record(sim)("after the history")
        ri.play_after([sim], aa, record(sim))
    assert len(checkpoints) == 5
    for label, (x, y) in checkpoints.items():
        for quantity, p, t in zip(("raw pose", "raw twist", "pose", "twist", "q", "qd", "effort"), x, y):
            assert np.isfinite(p).all() and np.isfinite(t).all(), (name, label, quantity)
            assert np.array_equal(t[dest], p[source[dest]]), f"{name}, {label}: {quantity} of a twin differs from its source"
            assert np.array_equal(t[~dest], p[~dest]), f"{name}, {label}: {quantity} of a robot that is no destination moved"
        assert not np.array_equal(x[0][dest], x[0][source[dest]]), (name, label)  # (the plain oracle does tell them apart)
    plain.close(), twin.close()


def test_the_test_map():
    source = cr.copy_map()
    mask = ri.reset_mask().astype(bool)
    dest = cr.destinations_of(source)
    assert source.dtype == np.int32 and source.shape == (B,)
    assert np.array_equal(dest, mask)
    assert (source[~dest] == -1).all()
    s = source[dest]
    d = np.flatnonzero(dest)
    assert ((s >= 0) & (s < B)).all() and not mask[s].any()
    assert (s // 64 != d // 64).any(), "no source in another wavefront than its destination"
    assert (np.bincount(s, minlength=B) >= 2).any(), "no source feeds two destinations"
    assert (s % 3 != d % 3).all(), "a destination keeps its mode group"
    assert cr.validate_map(source) is None
    # the wave-aligned map of the general path's bit-equality scenario
    al = cr.aligned_map()
    assert cr.validate_map(al) is None and np.array_equal(np.flatnonzero(cr.destinations_of(al)), np.arange(64, 128))
    # "leave me" in both spellings
    assert cr.validate_map(np.full(B, -1)) is None and cr.validate_map(np.arange(B)) is None
    # a chain: robot 1 (a source of the map) becomes a destination itself
    chain = source.copy()
    chain[1] = 3
    bad = cr.validate_map(chain)
    assert 1 in source[dest] and bad is not None and bad[1] == "chain" and chain[bad[0]] == 1
    # an index >= B
    far = source.copy()
    far[8] = B
    assert cr.validate_map(far) == (8, "out of range")


class StubEngine:
    def __init__(self):
        self.calls = []

    def copy_robots(self, source):
        self.calls.append(source)


def sharded(devices):
    from cdpr_simulation_amd.sharding import ShardedEngine, shard_range

    sh = object.__new__(ShardedEngine)  # (no GPU: the per-device engines are stubs)
    sh.B, sh.n = B, 8
    sh.spans = [shard_range(i, devices, B) for i in range(devices)]
    sh.engines = [StubEngine() for _ in range(devices)]
    return sh


@pytest.mark.parametrize("devices", [1, 3, 4])
def test_sharded_copy_slices_and_rebases(pkg, devices):
    sh = sharded(devices)
    rng = np.random.default_rng(7)
    source = np.full(B, -1, dtype=np.int32)
    for lo, hi in sh.spans:  # within every shard: its even robots take a random odd robot of the same shard, one robot names itself
        odd = np.arange(lo, hi)[np.arange(lo, hi) % 2 == 1]
        for r in range(lo + lo % 2, hi, 2):
            source[r] = rng.choice(odd)
        source[odd[0]] = odd[0]
    assert cr.validate_map(source) is None
    sh.copy_robots(source)
    sh.copy_robots(source.astype(np.int64).tolist())
    for e, (lo, hi) in zip(sh.engines, sh.spans):
        assert len(e.calls) == 2
        for part in e.calls:
            assert part.dtype == np.int32 and part.shape == (hi - lo,)
            d = cr.destinations_of(part)
            assert np.array_equal(d, cr.destinations_of(source)[lo:hi])
            assert np.array_equal(part[d] + lo, source[lo:hi][d]) and (part[~d] == -1).all()
            assert cr.validate_map(part) is None


def test_sharded_copy_refuses_before_any_shard_is_touched(pkg):
    sh = sharded(3)
    (lo0, hi0), (lo1, hi1) = sh.spans[0], sh.spans[1]
    source = np.full(B, -1, dtype=np.int32)
    source[lo0] = lo0 + 1     # fine, shard 0
    source[hi1 - 1] = lo0 + 1  # shard 1 takes a robot of shard 0
    with pytest.raises(ValueError, match="another shard"):
        sh.copy_robots(source)
    for bad in ((lo1, B), (lo1, lo0)):  # out of range; a chain (lo0 is a destination)
        m = source.copy()
        m[hi1 - 1] = -1
        m[bad[0]] = bad[1]
        assert cr.validate_map(m) is not None
        with pytest.raises(ValueError):
            sh.copy_robots(m)
    assert all(not e.calls for e in sh.engines)


def test_exports_and_a_null_handle(pkg):
    from cdpr_simulation_amd._native import EXPORTS, lib

    assert "cdpr_copy_robots" in EXPORTS and "cdpr_copy_robots_device" in EXPORTS
    source = np.full(4, -1, np.int32)
    assert lib().cdpr_copy_robots(None, source.ctypes.data_as(C.POINTER(C.c_int32))) == pkg._abi.ERR_INVALID
    assert lib().cdpr_copy_robots_device(None, None, None) == pkg._abi.ERR_INVALID
    assert hasattr(pkg.Engine, "copy_robots") and hasattr(pkg.Engine, "copy_robots_device")
