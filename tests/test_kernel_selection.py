"""What CDPR_MAP_AUTO picks, as a table: the routing rules of cdpr-simulation_amd/csrc/cdpr_select.hpp are
pure functions of the configuration, exposed without a GPU through cdpr_plan_kernel (include/cdpr.h), and every cell of
  cables {1 .. 12} x stages {none, FK, TD, FK + TD} x batch {1, 4 096, 32 768, 65 536, 131 072, 524 288}
  x handle {uniform, per-robot, general (hold branch live), precision = 64} x launch {1 step, 10 steps, MPC rollout}
(FK / TD from six cables on; a refused combination is pinned as its return code and reason) is pinned to the kernel name in tests/golden/kernel_selection.json (regenerate: python tests/test_kernel_selection.py --write,
and review the diff: a changed cell is a changed routing decision).  The engine takes its kernels from the same function
(planned_kernel names one instantiation; its label and its entry point are read from that descriptor alone, csrc/cdpr_kernels.hpp), and
tests/test_gpu_full_size.py checks on the GPU that the kernel a handle really launched (cdpr_kernel_name) is the planned one.  Whether
an instantiation stands behind every cell, and a different one exactly where the name differs, is checked here without a GPU
(cdpr_debug_plan_entry)."""
import ctypes as C
import json
import os
import sys
from dataclasses import replace

from parity import ROUTING_OVERRIDES, clean_env_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_selection.json")
CABLES, BATCHES = tuple(range(1, 13)), (1, 4096, 32768, 65536, 131072, 524288)
STAGES = {"none": 0, "fk": 1, "td": 2, "fk+td": 3}
HANDLES = ("uniform", "per_robot", "general", "fp64")
FIRST, SCHEDULED, ROLLOUT, NOT_STEADY = 1, 2, 4, 8


def model_of(pkg, n):
    if n == 4:
        return pkg.cube_model()
    full = pkg.eight_cable_model() if n <= 8 else pkg.twelve_cable_model()
    return replace(full, frame_anchors=full.frame_anchors[:n], platform_anchors=full.platform_anchors[:n])


def plan(pkg, cfg, steps=1, flags=0):
    from cdpr_simulation_amd._native import lib

    buf = C.create_string_buffer(256)
    s = cfg.to_struct()
    rc = lib().cdpr_plan_kernel(C.byref(s), steps, flags, buf, 256)
    return rc, buf.value.decode()


def plan_entry(cfg, steps=1, flags=0):
    """(1 = an instantiation behind every variant of the planned kernel | 0 | the refusal's code, the entry point's address)."""
    from cdpr_simulation_amd._native import lib

    s = cfg.to_struct()
    return lib().cdpr_debug_plan_entry(C.byref(s), steps, flags), lib().cdpr_debug_plan_entry_address(C.byref(s), steps, flags)


def cells(pkg):
    """(cell name, Config, steps per launch, flags) of the matrix."""
    for n in CABLES:
        for sname, stages in STAGES.items():
            if stages and n < 6:
                continue  # (refused by validate_config: FK / TD need six cables)
            for batch in BATCHES:
                for handle in HANDLES:
                    kw = dict(model=model_of(pkg, n), batch=batch, stages=stages)
                    if handle == "per_robot":
                        kw["perRobotCommands"] = True
                    elif handle == "general":
                        kw["velocityEpsilon"] = 0.001
                    elif handle == "fp64":
                        kw["precision"] = 64
                    for steps, flags, cell in ((1, 0, "k1"), (10, 0, "k10"), (10, ROLLOUT, "rollout")):
                        yield f"n{n} {sname} b{batch} {handle} {cell}", pkg.Config(**kw), steps, flags


def table(pkg):
    out = {}
    for key, cfg, steps, flags in cells(pkg):
        rc, name = plan(pkg, cfg, steps, flags)
        out[key] = name if rc == 0 else f"rc {rc}: {name}"
    return out


clean_env = clean_env_fixture()


def test_auto_routing_table_is_pinned(pkg, clean_env):
    got = table(pkg)
    want = json.load(open(GOLDEN))
    assert set(got) == set(want)
    diff = {k: (want[k], got[k]) for k in got if got[k] != want[k]}
    assert not diff, f"{len(diff)} routing decisions changed, e.g. {list(diff.items())[:5]}"
    # the cells BASELINE.json's configs land in
    assert got["n8 fk+td b65536 uniform k1"] == "cdpr_split_kernel<8, false>"           # config 3: the headline
    assert got["n4 none b4096 uniform k10"] == "cdpr_pair_stream_kernel<4>"              # config 2, scheduled / fused
    assert got["n4 none b4096 uniform k1"] == "cdpr_step_kernel_pair<4, false, false, true>"
    assert got["n8 fk+td b524288 uniform k1"] == "cdpr_step_kernel<8, true, true, SINGLE, LOWREG>"  # config 4 on one GPU
    assert got["n8 fk+td b65536 general k1"].startswith("cdpr_gen_lean_kernel<8>")
    assert got["n8 fk+td b65536 fp64 k1"] == "cdpr_split_kernel_f64<8, LEAN>"
    # a precision = 64 rollout runs on the handle's one-wave kernel with the rings in memory (rollout_enqueue_f64), whatever
    # the step launches of the same handle run on
    assert got["n8 fk+td b1 fp64 k1"] == "cdpr_split_kernel_f64<8>" and got["n8 fk+td b1 fp64 rollout"] == "cdpr_step_kernel_f64<8>"
    assert got["n8 none b1 fp64 k10"] == "cdpr_step_kernel_f64<8, RING_LDS, JCACHE>" and got["n8 none b1 fp64 rollout"] == "cdpr_step_kernel_f64<8>"
    assert got["n8 fk+td b4096 uniform rollout"] == "cdpr_step_kernel<8, true, true, ROLLOUT>"  # config 5
    assert got["n12 none b1 general k1"].startswith("rc -3: more than 8 cables")  # (refused by name, not served by another path)


def test_every_selectable_cell_has_a_kernel(pkg, clean_env):
    """Every cell the golden names a kernel for has an instantiation behind it - in both modes and, for the role-split kernel, in its
    steady-state form (cdpr_debug_plan_entry tries them) - and a refused cell is refused with the golden's code.  Over the matrix a
    kernel name and an entry point stand for each other: two cells share the entry exactly where they share the name."""
    want = json.load(open(GOLDEN))
    by_name, by_entry, entry_of = {}, {}, {}
    for key, cfg, steps, flags in cells(pkg):
        ok, address = plan_entry(cfg, steps, flags)
        if want[key].startswith("rc "):
            assert ok == int(want[key][3:].split(":")[0]) and not address, (key, ok)
            continue
        assert ok == 1 and address, (key, want[key], ok)
        by_name.setdefault(want[key], set()).add(address)
        by_entry.setdefault(address, set()).add(want[key])
        entry_of[key] = address
    assert all(len(v) == 1 for v in by_name.values()), [k for k, v in by_name.items() if len(v) != 1]
    assert all(len(v) == 1 for v in by_entry.values()), [v for v in by_entry.values() if len(v) != 1]
    assert len(by_name) > 150  # (the matrix reaches that many instantiations)
    # only the batch differs, within one regime: the same code
    assert entry_of["n8 fk+td b4096 uniform k1"] == entry_of["n8 fk+td b65536 uniform k1"]      # the role-split kernel
    assert entry_of["n8 fk+td b1 fp64 k1"] == entry_of["n8 fk+td b4096 fp64 k1"]                # cdpr_split_kernel_f64<8>
    assert entry_of["n8 fk+td b1 general k1"] == entry_of["n8 fk+td b32768 general k1"]         # cdpr_gen_split_kernel<8>
    assert entry_of["n4 none b1 uniform k10"] == entry_of["n4 none b65536 uniform k10"]         # cdpr_pair_stream_kernel<4>
    # ... and where the name differs, so does the code: across a routing threshold, the launch form, the stages, the cable count
    assert entry_of["n8 fk+td b65536 uniform k1"] != entry_of["n8 fk+td b131072 uniform k1"]    # role-split -> LOWREG
    assert entry_of["n8 fk+td b4096 fp64 k1"] != entry_of["n8 fk+td b65536 fp64 k1"]            # -> LEAN
    assert entry_of["n8 fk+td b32768 general k1"] != entry_of["n8 fk+td b65536 general k1"]     # role-split -> lean
    assert entry_of["n8 fk+td b65536 uniform k1"] != entry_of["n8 fk+td b65536 uniform k10"] != entry_of["n8 fk+td b65536 uniform rollout"]
    assert entry_of["n8 fk b65536 uniform k1"] != entry_of["n8 fk+td b65536 uniform k1"] != entry_of["n7 fk+td b65536 uniform k1"]
    assert entry_of["n8 fk+td b65536 uniform k1"] != entry_of["n8 fk+td b65536 per_robot k1"]   # <8, false> / <8, true>
    # the per-launch variants that share a name are instantiations of their own
    c2 = pkg.Config(batch=4096)
    assert plan_entry(c2, 10, NOT_STEADY)[1] != plan_entry(c2, 10)[1] and plan_entry(c2, 10, FIRST)[1] == plan_entry(c2, 10, NOT_STEADY)[1]


def test_launch_flags_and_overrides(pkg, clean_env, monkeypatch):
    c2 = pkg.Config(batch=4096)
    assert plan(pkg, c2, 1000, SCHEDULED) == (0, "cdpr_pair_stream_kernel<4>")
    assert plan(pkg, c2, 1, SCHEDULED) == (0, "cdpr_pair_stream_kernel<4>")  # a schedule of one step still runs the several-steps form
    assert plan(pkg, c2, 1000, SCHEDULED | FIRST) == (0, "cdpr_step_kernel_pair<4, false, false, false>")  # world step 0: a window to fill
    assert plan(pkg, c2, 10, NOT_STEADY) == (0, "cdpr_step_kernel_pair<4, false, false, false>")
    c5 = pkg.Config(model=pkg.eight_cable_model(), batch=512, stages=3)
    assert plan(pkg, c5, 64, ROLLOUT) == (0, "cdpr_step_kernel<8, true, true, ROLLOUT>")  # config 5
    g = pkg.Config(model=pkg.eight_cable_model(), batch=16384, stages=3, velocityEpsilon=0.001)
    assert plan(pkg, g, 1) == (0, "cdpr_gen_split_kernel<8>") and plan(pkg, g, 10) == (0, "cdpr_gen_split_kernel<8>")  # fused runs as one-step launches
    big = pkg.Config(model=pkg.eight_cable_model(), batch=65536, stages=3, velocityEpsilon=0.001)
    assert plan(pkg, big, 1, FIRST)[1] == "cdpr_gen_step_kernel<8, true, true, false, 11, SINGLE>"  # world step 0: the one-wave kernel
    monkeypatch.setenv("CDPR_GEN_SPLIT", "0")  # "the one-wave kernel" (ADVICE r05): the lean kernel stays off with it
    assert plan(pkg, big, 1)[1] == "cdpr_gen_step_kernel<8, true, true, false, 11, SINGLE>"
    monkeypatch.setenv("CDPR_GEN_LEAN", "1")
    assert plan(pkg, big, 1)[1].startswith("cdpr_gen_lean_kernel<8>")
    monkeypatch.delenv("CDPR_GEN_SPLIT"), monkeypatch.delenv("CDPR_GEN_LEAN")
    monkeypatch.setenv("CDPR_PAIR_STREAM", "0")
    assert plan(pkg, c2, 10) == (0, "cdpr_step_kernel_pair<4, false, false, false>")
    monkeypatch.delenv("CDPR_PAIR_STREAM")
    monkeypatch.setenv("CDPR_MAPPING", "1")
    assert plan(pkg, c2, 1) == (0, "cdpr_step_kernel<4, false, false, SINGLE>")


def test_refusals_carry_their_reason(pkg, clean_env):
    lumped = pkg.eight_cable_model()
    lumped.leg_inertia = 0.004
    assert plan(pkg, pkg.Config(model=lumped, batch=4, precision=64)) == (0, "cdpr_step_kernel_f64<8, TSTOP>")  # (in double since round 6)
    # ... and together with per-robot modes and the hold branch (later in round 6)
    assert plan(pkg, pkg.Config(model=lumped, batch=4, precision=64, perRobotCommands=True)) == (0, "cdpr_step_kernel_f64<8, PR, TSTOP>")
    assert plan(pkg, pkg.Config(model=lumped, batch=4, precision=64, perRobotCommands=True, velocityEpsilon=0.01)) == (0, "cdpr_step_kernel_f64<8, PR, HOLD = 1, TSTOP>")
    long_pr = pkg.Config(model=lumped, batch=4, precision=64, perRobotCommands=True)  # ... and windows beyond 11 samples with both
    long_pr.velocityController.dBufferLength = long_pr.positionController.dBufferLength = 20
    assert plan(pkg, long_pr) == (0, "cdpr_step_kernel_f64<8, PR, TSTOP, W = 31>")
    long_hold = pkg.Config(batch=4, precision=64, velocityEpsilon=0.01)  # ... and long windows with the hold branch: Pid records of 32 samples
    long_hold.velocityController.dBufferLength = 20
    assert plan(pkg, long_hold) == (0, "cdpr_step_kernel_f64<4, HOLD = 2, HW = 32>")
    assert plan(pkg, pkg.Config(model=pkg.twelve_cable_model(), batch=4, precision=64)) == (0, "cdpr_step_kernel_f64<12>")  # (end of round 6)
    rc, why = plan(pkg, pkg.Config(model=pkg.twelve_cable_model(), batch=4, precision=64, velocityEpsilon=0.01))  # beyond 8 cables: as in float
    assert rc == pkg._abi.ERR_UNSUPPORTED and "more than 8 cables" in why
    long_w = pkg.Config(batch=4, precision=64)
    long_w.velocityController.dBufferLength = 20
    assert plan(pkg, long_w, 10) == (0, "cdpr_step_kernel_f64<4, W = 31>")
    rc, why = plan(pkg, pkg.Config(batch=4, mapping=pkg._abi.MAP_LANE_PAIR, perRobotCommands=True))
    assert rc == pkg._abi.ERR_UNSUPPORTED and "CDPR_MAP_LANE_PAIR" in why


def test_precision_64_accepts_what_precision_32_accepts(pkg, clean_env):
    """End of round 6: no configuration that cdpr_create takes at precision = 32 is refused at precision = 64 - cable counts 4 / 8 / 12,
    the optional physics, per-robot modes, the hold branch, long windows, cascades, mappings, stages (384 combinations, planned
    without a GPU)."""
    from dataclasses import replace

    models = [pkg.cube_model(), pkg.eight_cable_model(), pkg.twelve_cable_model(),
              replace(pkg.eight_cable_model(), travel_lower=-0.01, travel_upper=0.01, travel_stop=2, leg_inertia=0.004)]
    checked = served = 0
    for m in models:
        for pr in (False, True):
            for eps in (-1.0, 0.004):
                for nbuf in (11, 20):
                    for cas in (0, 1):
                        for mapping in (pkg._abi.MAP_AUTO, pkg._abi.MAP_LANE_PAIR, pkg._abi.MAP_LANE_PER_ROBOT):
                            for stages in (0, 3):
                                def cfg(prec):
                                    c = pkg.Config(model=m, batch=64, stages=stages if m.n_cables >= 6 else 0, precision=prec, perRobotCommands=pr, velocityEpsilon=eps, mapping=mapping)
                                    c.velocityController.dBufferLength, c.velocityController.dDegree, c.velocityController.pFilter.cascade = nbuf, 2, cas
                                    return c
                                rc32, _ = plan(pkg, cfg(32))
                                rc64, why = plan(pkg, cfg(64))
                                checked += 1
                                served += rc32 == 0
                                assert rc32 != 0 or rc64 == 0, (m.n_cables, pr, eps, nbuf, cas, mapping, stages, why)
    assert checked == 384 and served >= 150


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import cdpr_simulation_amd as pkg_

    for k_ in ROUTING_OVERRIDES:
        os.environ.pop(k_, None)
    if "--write" in sys.argv:
        json.dump(table(pkg_), open(GOLDEN, "w"), indent=0, sort_keys=True)
        print("wrote", GOLDEN)
    else:
        print(json.dumps(table(pkg_), indent=0, sort_keys=True))
