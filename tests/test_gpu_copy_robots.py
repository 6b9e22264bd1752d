"""cdpr_copy_robots / cdpr_copy_robots_device: robots of a per-robot handle continue from where other robots of the handle are now - on
every record layout (register-resident per-robot records, the general path's record buffer with its hot rows, the precision = 64 rows),
against the fp64 oracle at the tolerances of tests/parity.py (TOL, TOL64).  On the oracle a copy is
the "twin from birth" of tests/test_copy_robots_inputs.py: an oracle whose destination rows were those of the sources from the start.

  1  right after the copy, every kind: every getter returns for a destination its source's row to the bit; a twin engine that ran the
     same history without the call is equal to the bit on every robot that is not a destination.
  2  against the oracle, every kind: the plain oracle before the copy, the twin from birth at every checkpoint of play_after.
  3  destination = source to the bit at every checkpoint: register-resident and precision = 64 kinds with the scattered map, general
     path with the wave-aligned map (64 .. 127 take 0 .. 63); general path with the scattered map: within TOL, exactness printed.
  4  hot rows (general_lean_hot): destinations / sources that a velocity Joy took out of the hot rows three steps before the copy.
  5  forms.  6  refusals.  7  a pending command survives.  8  a copy in front of every step.  9  the environment view.

B = 130: two full wavefronts and a ragged one, stride 192.
"""
import numpy as np
import pytest

import copy_robots as cr
import parity
import robot_histories as ri
from parity import NAMES, TOL, TOL64, engines, equal_rows, every_getter, observed, oracle_at
from per_robot_kinds import ALL, LAYOUTS, clean_env, config_of, named, state_of  # noqa: F401  (clean_env: autouse here too)

pytestmark = pytest.mark.gpu

B = ri.B
GENERAL = ["general_n8", "general_lean_hot", "general_long"]  # per-wave tier decisions (gen_controller): exact only lane for lane


def against_the_oracle(eng, ora, cfg, where):
    parity.against_the_oracle(eng, ora, cfg.precision == 64, where, printed="copy_robots")


# ---- 1, 2, 3, 4 ----------------------------------------------------------------------------------------------------------------
def run_scenario(pkg, oracle, monkeypatch, kind, source, seed, exact, kicked=None, more_stages=0, with_oracle=True):
    """History on an engine, its no-copy twin engine and the plain oracle; the copy; play_after with the destinations' input rows equal
    to their sources', against the twin-from-birth oracle.  exact: destination = source to the bit at every checkpoint, else within
    TOL.  kicked: uint8[B], robots that get a velocity Joy three steps before the copy (4).  Returns whether the bits were equal."""
    cfg = config_of(pkg, kind, monkeypatch, more_stages=more_stages)
    f64 = cfg.precision == 64
    tol = TOL64 if f64 else TOL
    dest = cr.destinations_of(source)
    src = source[dest]
    h, a = ri.history_inputs(cfg.model, seed), ri.after_inputs(cfg.model, seed + 1)
    ht, at = cr.twin_rows(h, source), cr.twin_rows(a, source)
    eng, twin = engines(pkg, cfg, h["pose"], 2)
    plain, born = (oracle_at(oracle, cfg, hh["pose"]) for hh in (h, ht)) if with_oracle else (None, None)
    oracles = [plain, born] if with_oracle else []
    if kicked is None:
        ri.play_history([eng, twin] + oracles[:1], h)
        ri.play_history(oracles[1:], ht)
    else:
        kick = dict(v=a["v"], m=kicked)
        kick_t = cr.twin_rows(kick, source)
        for sims, hh, kk in (([eng, twin] + oracles[:1], h, kick), (oracles[1:], ht, kick_t)):
            ri.play_history(sims, hh, ri.HISTORY - 3)
            for s in sims:
                assert s.set_velocity_command(kk["v"], mask=kk["m"]) == 0
                s.update(3)
    named(eng, kind)
    if with_oracle:
        against_the_oracle(eng, plain, cfg, f"{kind}, before the copy")
    steps = eng.step_count
    before = every_getter(eng, cfg, pkg)
    eng.copy_robots(source)
    after = every_getter(eng, cfg, pkg)
    assert eng.step_count == steps
    for k, (x, y) in enumerate(zip(before, after)):
        assert np.array_equal(y[dest], x[src]), f"{kind}: getter {k} of a destination is not its source's row right after the copy"
        assert np.array_equal(y[~dest], x[~dest]), f"{kind}: getter {k} of a robot that is no destination changed"
    assert not equal_rows(before, before, dest, src)  # (the history does tell them apart)
    assert equal_rows(after, every_getter(twin, cfg, pkg), ~dest, ~dest), f"{kind}: the copy changed a robot that is no destination (twin engine)"
    bits = []

    def check(label):
        if with_oracle:
            against_the_oracle(eng, born, cfg, f"{kind}, {label}")
        got = every_getter(eng, cfg, pkg)
        assert equal_rows(got, every_getter(twin, cfg, pkg), ~dest, ~dest), f"{kind}, {label}: a robot that is no destination differs from the twin engine's"
        bits.append(equal_rows(got, got, dest, src))
        if exact:
            assert bits[-1], f"{kind}, {label}: destination and source have parted"
        for name, x in zip(NAMES, observed(eng, cfg.precision == 64)):
            err = float(np.abs(x[dest] - x[src]).max())
            assert err <= tol[name], f"{kind}, {label}: {name} of destination and source differ by {err:.3e}"

    ri.play_after([eng, twin] + oracles[1:], at, check)
    named(eng, kind)
    print(f"copy_robots, {kind}: destination = source to the bit at the checkpoints: {bits}")
    for s in [eng, twin] + oracles:
        s.close()
    return bits


@pytest.mark.parametrize("kind", ALL)
def test_copy_on_every_kind(pkg, oracle, monkeypatch, kind):
    """1, 2, 3 with the scattered map: exact on the register-resident and precision = 64 kinds, within TOL on the general path."""
    run_scenario(pkg, oracle, monkeypatch, kind, cr.copy_map(), 131, exact=kind not in GENERAL)


@pytest.mark.parametrize("kind", GENERAL)
def test_a_wave_aligned_copy_is_exact_on_the_general_path(pkg, oracle, monkeypatch, kind):
    run_scenario(pkg, oracle, monkeypatch, kind, cr.aligned_map(), 141, exact=True)


@pytest.mark.parametrize("shape", ["scattered", "aligned"])
def test_hot_rows_travel_with_the_records(pkg, oracle, monkeypatch, shape):
    """Half of the destinations get a masked velocity Joy three steps before the copy (they have left the hot rows, their sources are in
    them); for the other half the sources get it.  62 steps later all of them are back in the steady state: the oracle says so."""
    source = cr.copy_map() if shape == "scattered" else cr.aligned_map()
    d = np.flatnonzero(cr.destinations_of(source))
    kicked = np.zeros(B, np.uint8)
    kicked[d[::2]] = 1
    kicked[source[d[1::2]]] = 1
    assert kicked[d].any() and not kicked[d].all() and kicked[source[d]].any() and not kicked[source[d]].all()
    run_scenario(pkg, oracle, monkeypatch, "general_lean_hot", source, 151, exact=shape == "aligned", kicked=kicked)


@pytest.mark.parametrize("kind", ALL)
def test_the_pid_topic_travels(pkg, oracle, monkeypatch, kind):
    """the `pid` debug row (1 with CDPR_STAGE_PID_DEBUG; such a handle need not run the kernel HANDLES names)"""
    cfg = config_of(pkg, kind, monkeypatch, more_stages=pkg._abi.STAGE_PID_DEBUG)
    source = cr.copy_map()
    dest = cr.destinations_of(source)
    h = ri.history_inputs(cfg.model, 161)
    (eng,) = engines(pkg, cfg, h["pose"], 1)
    ri.play_history([eng], h, 15)
    before = every_getter(eng, cfg, pkg)
    assert before[-1][dest].any() and not np.array_equal(before[-1][dest], before[-1][source[dest]])
    eng.copy_robots(source)
    after = every_getter(eng, cfg, pkg)
    for x, y in zip(before, after):
        assert np.array_equal(y[dest], x[source[dest]]) and np.array_equal(y[~dest], x[~dest]), kind
    eng.update(5)
    now = eng.pid_debug()
    if kind not in GENERAL:
        assert np.array_equal(now[dest], now[source[dest]]), kind
    eng.close()


@pytest.mark.parametrize("kind", LAYOUTS)
def test_the_episode_clock_travels(pkg, oracle, monkeypatch, kind):
    """Sources that were reset at world step 5: their destinations take the episode start 5 and the age the environment view shows."""
    cfg = config_of(pkg, kind, monkeypatch)
    source = cr.copy_map()
    dest = cr.destinations_of(source)
    sources = np.zeros(B, np.uint8)
    sources[source[dest]] = 1
    h = ri.history_inputs(cfg.model, 165)
    (eng,) = engines(pkg, cfg, h["pose"], 1)
    eng.update(5)
    eng.reset_robots(sources, h["pose"])
    eng.update(7)
    start = eng.episode_start()
    assert np.array_equal(start, 5 * sources.astype(np.uint32))
    eng.copy_robots(source)
    want = start.copy()
    want[dest] = 5
    assert np.array_equal(eng.episode_start(), want), kind
    age = eng.observe(pkg._abi.OBS_AGE)[:, 0]
    assert np.array_equal(age, (12 - want).astype(np.float32)), kind
    eng.close()


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", LAYOUTS)
def test_forms(pkg, oracle, monkeypatch, kind):
    cfg = config_of(pkg, kind, monkeypatch)
    h = ri.history_inputs(cfg.model, 171)
    source = cr.copy_map()
    host, dev, nothing, twin = engines(pkg, cfg, h["pose"], 4)
    ri.play_history([host, dev, nothing, twin], h)
    # host form = device form; the status words; a NULL status
    host.copy_robots(source)
    d_source, d_status = dev.device_upload(source), dev.device_upload(np.array([7, 7], np.uint32))
    dev.copy_robots_device(d_source, d_status)
    assert np.array_equal(dev.device_download(d_status, (2,), np.uint32), [int(cr.destinations_of(source).sum()), 0]), kind
    for e in (host, dev):
        e.update(3)
    assert equal_rows(every_getter(host, cfg, pkg), every_getter(dev, cfg, pkg), slice(None), slice(None)), f"{kind}: the device form differs from the host form"
    host.copy_robots(source), dev.copy_robots_device(d_source)  # (again: the destinations have moved three steps on; no status)
    for e in (host, dev):
        e.update(2)
    assert equal_rows(every_getter(host, cfg, pkg), every_getter(dev, cfg, pkg), slice(None), slice(None)), kind
    # "leave me" in both spellings changes nothing; the counts say so
    nothing.copy_robots(np.full(B, -1, np.int32))
    nothing.copy_robots(np.arange(B, dtype=np.int32))
    nothing_status = nothing.device_upload(np.array([7, 7], np.uint32))
    d_same = nothing.device_upload(np.arange(B, dtype=np.int32))
    nothing.copy_robots_device(d_same, nothing_status)
    assert np.array_equal(nothing.device_download(nothing_status, (2,), np.uint32), [0, 0]), kind
    assert equal_rows(every_getter(nothing, cfg, pkg), every_getter(twin, cfg, pkg), slice(None), slice(None)), f"{kind}: an empty map changed something"
    nothing.update(4), twin.update(4)
    assert equal_rows(every_getter(nothing, cfg, pkg), every_getter(twin, cfg, pkg), slice(None), slice(None)), f"{kind}: an empty map changed something"
    dev.synchronize(), nothing.synchronize()
    dev.device_free(d_source), dev.device_free(d_status), nothing.device_free(nothing_status), nothing.device_free(d_same)
    for e in (host, dev, nothing, twin):
        e.close()


# ---- 6 -------------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg, oracle, monkeypatch):
    # a uniform handle: the reset call's refusal, nothing changed
    cfg = config_of(pkg, "fast_n8", monkeypatch, per_robot=False)
    h = ri.history_inputs(cfg.model, 181)
    source = cr.copy_map()
    eng, twin = engines(pkg, cfg, h["pose"], 2)
    for s in (eng, twin):
        s.set_velocity_command(h["v"])
        s.update(20)
    d = eng.device_upload(source)
    with pytest.raises(pkg.CdprError) as reset_refusal:
        eng.reset_robots(np.ones(B, np.uint8))
    for call in (lambda: eng.copy_robots(source), lambda: eng.copy_robots_device(d)):
        with pytest.raises(pkg.CdprError) as ei:
            call()
        assert ei.value.code == reset_refusal.value.code == pkg._abi.ERR_UNSUPPORTED and "per_robot_commands" in str(ei.value)
    eng.device_free(d)
    eng.update(5), twin.update(5)
    assert equal_rows(state_of(eng, cfg), state_of(twin, cfg), slice(None), slice(None))
    eng.close(), twin.close()
    # a chain and an out-of-range entry
    chain, far = source.copy(), source.copy()
    chain[1] = 3  # robot 1 is the source of robot 63
    far[8] = B
    both = chain.copy()
    both[8] = B
    assert cr.validate_map(chain) == (63, "chain") and cr.validate_map(far) == (8, "out of range")
    valid = both.copy()
    valid[[63, 8]] = -1  # what the device form is left with
    assert cr.validate_map(valid) is None
    for kind in LAYOUTS:
        cfg = config_of(pkg, kind, monkeypatch)
        eng, dev, want, twin = engines(pkg, cfg, h["pose"], 4)
        ri.play_history([eng, dev, want, twin], h)
        for bad in (chain, far, both):
            with pytest.raises(pkg.CdprError) as ei:
                eng.copy_robots(bad)
            assert ei.value.code == pkg._abi.ERR_INVALID, kind
        with pytest.raises(pkg.CdprError) as ei:
            eng.copy_robots_device(0)
        assert ei.value.code == pkg._abi.ERR_INVALID
        assert equal_rows(every_getter(eng, cfg, pkg), every_getter(twin, cfg, pkg), slice(None), slice(None)), f"{kind}: a refused map changed something"
        d_source, d_status = dev.device_upload(both), dev.device_upload(np.zeros(2, np.uint32))
        dev.copy_robots_device(d_source, d_status)
        want.copy_robots(valid)
        assert np.array_equal(dev.device_download(d_status, (2,), np.uint32), [int(cr.destinations_of(valid).sum()), 2]), kind
        got = every_getter(dev, cfg, pkg)
        assert equal_rows(got, every_getter(want, cfg, pkg), slice(None), slice(None)), f"{kind}: the device form did not copy exactly the valid entries"
        untouched = ~cr.destinations_of(valid)
        assert untouched[63] and untouched[8]
        assert equal_rows(got, every_getter(twin, cfg, pkg), untouched, untouched), f"{kind}: a skipped or untouched robot changed"
        dev.device_free(d_source), dev.device_free(d_status)
        for e in (eng, dev, want, twin):
            e.close()


# ---- 7 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fast_n8", "general_n8", "fp64_n8"])
def test_a_pending_command_stays_with_its_index(pkg, oracle, monkeypatch, kind):
    """A masked velocity Joy set BEFORE the copy, for a destination (0) and for a source (2) among others: it is latched at the next step
    onto the index it was addressed to - the destination gets its own row, not its source's, and robot 4 (same source, not addressed)
    goes on as its source did before the Joy."""
    cfg = config_of(pkg, kind, monkeypatch)
    source = cr.copy_map()
    h, a = ri.history_inputs(cfg.model, 191), ri.after_inputs(cfg.model, 192)
    (eng,) = engines(pkg, cfg, h["pose"], 1)
    born = oracle_at(oracle, cfg, cr.twin_rows(h, source)["pose"])
    ri.play_history([eng], h)
    ri.play_history([born], cr.twin_rows(h, source))
    joy_mask = (np.arange(B) % 8 < 3).astype(np.uint8)  # 0 (destination), 2 (its source), 8, 16 ... (destinations), 1, 9 ... (others)
    assert joy_mask[0] and joy_mask[2] and not joy_mask[4] and source[0] == source[4] == 2
    assert eng.set_velocity_command(a["v"], mask=joy_mask) == 0
    eng.copy_robots(source)
    assert born.set_velocity_command(a["v"], mask=joy_mask) == 0  # by index: NOT the twinned rows
    eng.update(1), born.update(1)
    against_the_oracle(eng, born, cfg, f"{kind}, pending velocity Joy, 1 step")
    eng.update(20), born.update(20)
    against_the_oracle(eng, born, cfg, f"{kind}, pending velocity Joy, 21 steps")
    q = observed(eng, cfg.precision == 64)[2]
    assert not np.array_equal(q[0], q[2]) and not np.array_equal(q[0], q[4])
    eng.close(), born.close()


# ---- 8 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fast_n8", "general_n8"])
def test_a_copy_in_front_of_every_step(pkg, oracle, monkeypatch, kind):
    """25 steps, each behind a device-form copy, two maps taking turns; twice an update(10) in between, so that graph replays sit between
    the copies.  An engine doing the same through the host form holds the same bits.  The second map's destinations are robots the
    first leaves alone (index mod 4 = 1, no source of the first map), each taking its right neighbour: the union of the two is a valid
    map, and with no new command after the first copy the end state is that union's twin from birth."""
    cfg = config_of(pkg, kind, monkeypatch)
    first = cr.copy_map()
    second = np.full(B, -1, np.int32)
    for r in range(1, B - 1, 4):
        if r not in set(first[first >= 0]):
            second[r] = r + 1
    union = np.where(first >= 0, first, second).astype(np.int32)
    assert cr.validate_map(second) is None and cr.validate_map(union) is None and cr.destinations_of(second).sum() > 10
    h = ri.history_inputs(cfg.model, 201)
    dev, host = engines(pkg, cfg, h["pose"], 2)
    born = oracle_at(oracle, cfg, cr.twin_rows(h, union)["pose"])
    ri.play_history([dev, host], h)
    ri.play_history([born], cr.twin_rows(h, union))
    d_maps = [dev.device_upload(m) for m in (first, second)]
    d_status = dev.device_upload(np.zeros(2, np.uint32))
    for step in range(25):
        dev.copy_robots_device(d_maps[step % 2], d_status)
        host.copy_robots((first, second)[step % 2])
        for s in (dev, host, born):
            s.update(1)
        if step in (8, 17):
            for s in (dev, host, born):
                s.update(10)
    assert np.array_equal(dev.device_download(d_status, (2,), np.uint32), [int(cr.destinations_of(first).sum()), 0])  # (step 24: the first map)
    assert equal_rows(every_getter(dev, cfg, pkg), every_getter(host, cfg, pkg), slice(None), slice(None)), f"{kind}: host and device form have parted"
    against_the_oracle(dev, born, cfg, f"{kind}, a copy before every step, the end")
    named(dev, kind)
    dev.synchronize()
    for d in d_maps + [d_status]:
        dev.device_free(d)
    dev.close(), host.close(), born.close()


# ---- 9 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fast_n8", "fp64_hold_n8"])
def test_the_environment_view_shows_the_sources(pkg, oracle, monkeypatch, kind):
    """observe_device with the destination set as row mask: the destinations' rows are their sources', the columns behind the packed
    width (robot-indexed by the caller) and every other row stay as the caller left them."""
    cfg = config_of(pkg, kind, monkeypatch)
    source = cr.copy_map()
    dest = cr.destinations_of(source)
    h = ri.history_inputs(cfg.model, 211)
    (eng,) = engines(pkg, cfg, h["pose"], 1)
    ri.play_history([eng], h)
    fields = pkg._abi.OBS_ALL
    width = eng.observation_width(fields)
    before = eng.observe(fields)
    assert not np.array_equal(before[dest], before[source[dest]])
    ld = width + 2
    mine = np.tile(np.arange(B, dtype=np.float32)[:, None] + 1000.0, (1, ld))
    d_obs, d_rows = eng.device_upload(mine), eng.device_upload(dest.astype(np.uint8))
    eng.copy_robots(source)
    eng.observe_device(fields, d_obs, ld, d_rows)
    got = eng.device_download(d_obs, (B, ld), np.float32)
    assert np.array_equal(got[dest, :width], before[source[dest]]), kind
    assert np.array_equal(got[:, width:], mine[:, width:]) and np.array_equal(got[~dest], mine[~dest]), kind
    assert np.array_equal(eng.observe(fields)[~dest], before[~dest])
    eng.device_free(d_obs), eng.device_free(d_rows)
    eng.close()
