"""Every getter against a decoder that owes nothing to the library.

cdpr_get_observables and the separate getters share one gather kernel and one host routine (read_blocks, csrc/cdpr_engine_readout.hip),
so their equality (test_gpu_cable_counts.py) compares one implementation with itself.  Here the last image of update_record is
downloaded as bytes and decoded by tests/readout_layout.py (numpy, written from DESIGN.md section 3); every getter must equal that
decode bit for bit: joint_states, platform_state, observables, fk_state's residual and iteration count, td_state, limit_state, the
library's own cdpr_decode_observables; on precision = 64 handles observables_f64 and cdpr_decode_observables_f64, and the float
getters and the float decoder equal the doubles cast once to float32.  Every cell asserts that its handle stepped on the kernel family
of the layout it is named for.

raw_state[_f64] and the FK pose live in the state.  The C-ABI exports no pointer to the state rows, so they cannot be downloaded and
decoded on the host; they are pinned three ways: (a) set_platform_state[_f64] of random poses and twists followed by raw_state and
fk_state before any update returns those bits; (b) after updates raw_state[_f64] equals, to the bit and in the handle's own number
type, the pose and twist that the NEXT step publishes (a step publishes the state it starts from), decoded from that step's image by
numpy; (c) raw_state and the FK pose equal the environment view's POSE / TWIST / FK_POSE columns (cdpr_observe_device: cdpr_env.hpp
reads the state rows on the device with row constants of its own; floats, so on precision = 64 the FK estimate's doubles are pinned
by (a) alone).

Layouts: one handle kind per record layout of tests/per_robot_kinds.py (register-resident, general path, precision = 64) with the cable
count and the batch varied: B = 1 (one ragged block of the gather), 67 and 130 (several blocks, a ragged last wavefront, strides 128
and 192); n = 4, 5, 8, 12 (one full joint slot, a ragged second one, two and three full slots); FK + TD from six cables on.  Per-robot and general handles stop at eight cables, so n = 12 runs on uniform handles and not on the general path.  The tier
boundaries: where the gathered bytes pass 2 MiB (precision = 64: mapped image -> scratch and one copy per block; fp32: staging image
-> caller arrays) and 256 KiB (fp32: completion word -> staging), at and one robot past each, n = 4 (25 columns).  NULL outputs in
every position of every getter and of both decoders; every read twice in a row (the completion word's epoch)."""
import ctypes as C

import numpy as np
import pytest

import per_robot_kinds as prk
import readout_layout as rl
import robot_histories as ri
from parity import perturbed_poses

pytestmark = pytest.mark.gpu

KINDS = {"fast": "fast_n8", "general": "general_n8", "fp64": "fp64_n8"}  # one kind of tests/per_robot_kinds.py per record layout
BLOCKS = ("position", "velocity", "effort", "pose", "twist")


def engine_of(pkg, layout, n, batch):
    _, kw, env, _ = prk.HANDLES[KINDS[layout]]
    assert not env
    kw = dict(kw, stages=3 if n >= 6 else 0)
    return pkg.Engine(pkg.Config(model=ri.model_of(pkg, n), batch=batch, perRobotCommands=n <= 8, **kw), 0)


def last_image(eng, steps=3, per_launch=2):
    image = eng.observable_image_bytes()
    dptr = eng.device_alloc(image * steps)
    try:
        eng.update_record_device(steps, per_launch, dptr, image * steps)
        return eng.device_download(dptr, (steps, image), dtype=np.uint8)[-1].copy()
    finally:
        eng.device_free(dptr)


def same(got, want, where):
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), where


def with_null_in_every_position(eng, fn, arrays, where, lead=()):
    """fn(handle, *lead, *pointers) with NULL in place of each output in turn: the others come out as `arrays`, nothing else is written"""
    for skip in range(len(arrays)):
        out = [np.full_like(a, 77) for a in arrays]
        args = [None if k == skip else C.cast(o.ctypes.data_as(C.c_void_p), fn.argtypes[1 + len(lead) + k]) for k, o in enumerate(out)]
        assert fn(eng._h, *lead, *args) == 0, where
        for k, (o, a) in enumerate(zip(out, arrays)):
            same(o, a if k != skip else np.full_like(a, 77), f"{where}: output {k} with NULL at {skip}")


def check_against_image(eng, n, fp64, where, nulls=True):
    """every getter of the published step = the numpy decode of the last recorded image (which update_record leaves as the handle's own)"""
    from cdpr_simulation_amd._native import lib

    L = lib()
    raw = last_image(eng)
    dec = rl.decode_image(raw, eng.B, n, fp64)
    as32 = {k: v.astype(np.float32) for k, v in dec.items()}  # (precision = 64: the float getters round once)
    want = [as32[k] for k in BLOCKS]
    image = (raw.ctypes.data_as(C.c_void_p),)
    for k, got in enumerate(eng.decode_observables(raw)):
        same(got, want[k], f"{where}: cdpr_decode_observables {BLOCKS[k]}")
    with_null_in_every_position(eng, L.cdpr_decode_observables, want, f"{where}: cdpr_decode_observables", lead=image)
    if fp64:  # (the all-outputs call is the pass with NULL in no position: every pass fills four of the five)
        with_null_in_every_position(eng, L.cdpr_decode_observables_f64, [dec[k] for k in BLOCKS], f"{where}: cdpr_decode_observables_f64", lead=image)
        full = [np.empty_like(dec[k]) for k in BLOCKS]
        assert L.cdpr_decode_observables_f64(eng._h, *image, *[eng._dp(a) for a in full]) == 0, where
        for k, got in enumerate(full):
            same(got, dec[BLOCKS[k]], f"{where}: cdpr_decode_observables_f64 {BLOCKS[k]}")
    for call in range(2):  # (twice in a row: the completion word's epoch)
        for k, got in enumerate(eng.observables()):
            same(got, want[k], f"{where}: observables {BLOCKS[k]}, call {call}")
        for k, got in enumerate(eng.joint_states() + eng.platform_state()):
            same(got, want[k], f"{where}: separate getters {BLOCKS[k]}, call {call}")
        if fp64:
            for k, got in enumerate(eng.observables_f64()):
                same(got, dec[BLOCKS[k]], f"{where}: observables_f64 {BLOCKS[k]}, call {call}")
    flags = dec["flags"].astype(np.int32)
    same(eng.limit_state(), (flags >> 1).astype(np.uint32), f"{where}: limit_state")
    stages = int(eng.config.stages)
    if stages & 1:
        _, res, it = eng.fk_state()
        same(res, as32["fk_residual"], f"{where}: fk residual")
        same(it, dec["fk_iterations"].astype(np.int32), f"{where}: fk iterations")
    if stages & 2:
        tension, flag = eng.td_state()
        same(tension, as32["effort"], f"{where}: td tension")
        same(flag, flags & 1, f"{where}: td flag")
    if nulls:
        with_null_in_every_position(eng, L.cdpr_get_observables, want, f"{where}: cdpr_get_observables")
        with_null_in_every_position(eng, L.cdpr_get_joint_states, want[:3], f"{where}: cdpr_get_joint_states")
        with_null_in_every_position(eng, L.cdpr_get_platform_state, want[3:], f"{where}: cdpr_get_platform_state")
        with_null_in_every_position(eng, L.cdpr_get_raw_state, list(eng.raw_state()), f"{where}: cdpr_get_raw_state")
        if fp64:
            with_null_in_every_position(eng, L.cdpr_get_observables_f64, [dec[k] for k in BLOCKS], f"{where}: cdpr_get_observables_f64")
            with_null_in_every_position(eng, L.cdpr_get_raw_state_f64, list(eng.raw_state_f64()), f"{where}: cdpr_get_raw_state_f64")
        if stages & 1:
            with_null_in_every_position(eng, L.cdpr_get_fk_state, list(eng.fk_state()), f"{where}: cdpr_get_fk_state")
        if stages & 2:
            with_null_in_every_position(eng, L.cdpr_get_td_state, list(eng.td_state()), f"{where}: cdpr_get_td_state")


def on_its_layout(eng, layout):
    """the last step launch ran on the kernel family of the record layout the cell is named for"""
    name = eng.kernel_name
    family = "fp64" if "f64" in name else "general" if "cdpr_gen_" in name else "fast"
    assert family == layout, (layout, name)


def cells():
    out = []
    for layout in KINDS:
        for n in (4, 5, 8, 12):
            if n > 8 and layout == "general":
                continue  # (the general path stops at eight cables)
            for batch in (1, 67, 130):
                out.append((layout, n, batch))
    return out


@pytest.mark.parametrize("layout,n,batch", cells(), ids=lambda v: str(v))
def test_every_getter_equals_the_numpy_decode(pkg, layout, n, batch):
    fp64 = layout == "fp64"
    where = f"{layout}, n = {n}, B = {batch}"
    rng = np.random.default_rng(1000 * n + batch)
    eng = engine_of(pkg, layout, n, batch)
    pose = perturbed_poses(eng.config.model, batch, rng, dp=0.02, dr=0.05)
    twist = rng.uniform(-0.05, 0.05, (batch, 6))
    fk = bool(int(eng.config.stages) & 1)
    # (a) the state columns before any update: what set_platform_state[_f64] wrote, bit for bit
    p32, t32 = pose.astype(np.float32), twist.astype(np.float32)
    eng.set_platform_state(pose7=p32, twist6=t32)
    for k, (got, want) in enumerate(zip(eng.raw_state(), (p32, t32))):
        same(got, want, f"{where}: raw_state {k} after set_platform_state")
    if fk:
        same(eng.fk_state()[0], p32, f"{where}: the FK seed follows the spawn pose")
    if fp64:
        for k, (got, want) in enumerate(zip(eng.raw_state_f64(), (p32.astype(np.float64), t32.astype(np.float64)))):
            same(got, want, f"{where}: raw_state_f64 {k} after set_platform_state")
        eng.set_platform_state_f64(pose7=pose, twist6=twist)
        for k, (got, want) in enumerate(zip(eng.raw_state_f64(), (pose, twist))):
            same(got, want, f"{where}: raw_state_f64 {k} after set_platform_state_f64")
        for k, (got, want) in enumerate(zip(eng.raw_state(), (pose, twist))):
            same(got, want.astype(np.float32), f"{where}: raw_state {k} rounds the doubles once")
        if fk:
            same(eng.fk_state()[0], p32, f"{where}: the FK seed follows the spawn pose (doubles, rounded once)")
        eng.set_platform_state_f64(twist6=np.zeros((batch, 6)))  # pose only, twist only: the other rows stay
        same(eng.raw_state_f64()[0], pose, f"{where}: a twist alone leaves the pose")
    else:
        eng.set_platform_state(twist6=np.zeros((batch, 6), dtype=np.float32))
        same(eng.raw_state()[0], p32, f"{where}: a twist alone leaves the pose")
    # the published step
    eng.update(2)
    eng.set_velocity_command(rng.uniform(-0.03, 0.03, (batch, n)).astype(np.float32))
    check_against_image(eng, n, fp64, where)
    on_its_layout(eng, layout)
    # (b) the state columns after updates.  A step publishes the pose and twist it STARTS from (PLG.cpp:248-280 publishes in front of the world
    # step), so the raw state read now is, to the bit, the pose and twist in the image of the next step - decoded by numpy, in the handle's
    # own number type
    before = eng.raw_state_f64() if fp64 else eng.raw_state()
    before32 = eng.raw_state()
    nxt = rl.decode_image(last_image(eng, 1, 1), batch, n, fp64)
    for k, key in enumerate(("pose", "twist")):
        same(before[k], nxt[key], f"{where}: raw {key} = the next image's {key}")
        same(before32[k], nxt[key].astype(np.float32), f"{where}: raw_state {key} = the next image's {key}, rounded once")
    # ... and the FK pose, which no image holds: the state columns after updates: the environment view reads them on the device by its own row constants
    A = pkg._abi
    view = eng.observe(A.OBS_POSE | A.OBS_TWIST | (A.OBS_FK_POSE if fk else 0))
    rp, rt = eng.raw_state()
    same(rp, view[:, 0:7], f"{where}: raw pose against the environment view")
    same(rt, view[:, 7:13], f"{where}: raw twist against the environment view")
    if fk:
        same(eng.fk_state()[0], view[:, 13:20], f"{where}: FK pose against the environment view")
    if fp64:
        dp, dt = eng.raw_state_f64()
        same(dp.astype(np.float32), view[:, 0:7], f"{where}: raw_state_f64 pose, rounded once")
        same(dt.astype(np.float32), view[:, 7:13], f"{where}: raw_state_f64 twist, rounded once")
    eng.close()


def boundaries():
    cols = 25  # 3 n + 13 at n = 4
    out = [("fp64", (2 << 20) // (8 * cols)), ("fp64", (2 << 20) // (4 * cols)), ("fast", (256 << 10) // (4 * cols)), ("fast", (2 << 20) // (4 * cols))]
    return [(layout, b + d) for layout, b in out for d in (0, 1)]


@pytest.mark.parametrize("layout,batch", boundaries(), ids=lambda v: str(v))
def test_tier_boundaries_equal_the_numpy_decode(pkg, layout, batch):
    """n = 4: the five arrays are 25 columns.  precision = 64: observables_f64 passes 2 MiB between (2 << 20) // 200 and the next batch, the
    float getters between (2 << 20) // 100 and the next; fp32: the completion-word tier ends at (256 << 10) // 100, the staging tier at
    (2 << 20) // 100.  (The separate getters ask for fewer bytes at the same batch, so each batch also reads through the tier below.)"""
    n, fp64 = 4, layout == "fp64"
    rng = np.random.default_rng(batch)
    eng = engine_of(pkg, layout, n, batch)
    eng.set_platform_state(pose7=perturbed_poses(eng.config.model, batch, rng, dp=0.02, dr=0.05).astype(np.float32))
    eng.set_velocity_command(rng.uniform(-0.03, 0.03, (batch, n)).astype(np.float32))
    eng.update(2)
    check_against_image(eng, n, fp64, f"{layout}, B = {batch}", nulls=False)
    on_its_layout(eng, layout)
    eng.close()
