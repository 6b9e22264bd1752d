"""What tests/test_padded_stride_inputs.py (CPU) and tests/test_gpu_padded_stride.py (GPU) share: handles on a padded row stride.

Every per-robot buffer of a handle is addressed row * stride + r.  cdpr_create sets stride = round_up(batch, 64) and adds 128 columns
where that would be a multiple of 131 072 (HBM channel aliasing: csrc/cdpr_engine.hip, profiles/r04_stride_padding.txt), so
stride != round_up(batch, 64) exactly at 131 072, 262 144 and 524 288 robots.  CDPR_STRIDE_PAD=<columns> forces a pad at any batch:
`create` sets it around the create call alone (cdpr_create is the only reader), so the padded layout runs at B = 130 in seconds.

PADS: 64 is the narrowest pad the create rule accepts, narrower than a 128-thread workgroup; 128 is the production pad.  At B = 130 the
strides are 256 and 320 against 192.  The pad columns hold home-state rows that are not robots.

The stride is an internal layout: robot r sits in the same lane either way, so a padded handle equals its unpadded twin to the bit on
everything a caller can read (`state_everything`, `assert_same`), and is held to the same references at the same tolerances as the
unpadded handles of the other modules (tests/parity.py, tests/done_rules.py, tests/resample_oracle.py, tests/env_view.py).

pytest rewrites asserts only in test modules, so every assert here carries its message.
"""
from dataclasses import replace

import numpy as np

import copy_robots as cr
import done_handles as gd
import done_rules as dr
import env_view as ev
import parity
import per_robot_kinds as prk
import resample_oracle as ro
import robot_histories as ri
import workspace_poses as wp

ENV = "CDPR_STRIDE_PAD"
PADS = (64, 128)
B = ri.B
EVERY = slice(None)
EDGE_BATCHES = (1, 63, 64, 65, 257)  # a single robot | a ragged wave, a full one, one robot more | two 128-thread workgroups and a robot
OPS_KINDS = prk.ALL                                                # reset, copy, resample: the nine per-robot kinds
VIEW_KINDS = gd.KINDS + [k for k in prk.ALL if k not in gd.KINDS]  # verdicts, view, read-out: three layouts, three uniform, six more
FULL_B = 131072  # the smallest batch cdpr_create pads by itself


def round_up(batch):
    return (int(batch) + 63) & ~63


# ---- the stride of a handle, from the size of its observable image ----------------------------------------------------------------
def row_bytes(n, f64=False, unpadded_image=None, batch=None):
    """Bytes of the observable image per column of the stride.  fp32 handles: n_obs float4 slots of 16 B, n_obs = 4 + 3 ceil(n / 4)
    (DESIGN.md section 3).  precision = 64: worked out from the image of an UNPADDED twin of `batch` robots, whose stride is
    round_up(batch, 64)."""
    if not f64:
        return 16 * (4 + 3 * ((int(n) + 3) // 4))
    assert unpadded_image is not None and batch is not None, "row_bytes: a precision = 64 handle needs its unpadded twin's image"
    stride = round_up(batch)
    assert unpadded_image % stride == 0, f"row_bytes: an image of {unpadded_image} B is no whole number of {stride}-column rows"
    return unpadded_image // stride


def stride_from_image(image_bytes, row):
    assert row > 0 and image_bytes % row == 0, f"stride_from_image: {image_bytes} B is no whole number of {row} B columns"
    return image_bytes // row


def stride_of(eng, cfg, unpadded=None):
    """The row stride of `eng`, in columns; `unpadded`: the unpadded twin a precision = 64 handle needs."""
    f64 = cfg.precision == 64
    row = row_bytes(cfg.n_cables, f64, unpadded.observable_image_bytes() if f64 and unpadded is not None else None, cfg.batch)
    return stride_from_image(eng.observable_image_bytes(), row)


# ---- handles ----------------------------------------------------------------------------------------------------------------------
def create(pkg, cfg, monkeypatch, pad, count=1):
    """`count` engines created with CDPR_STRIDE_PAD=pad, or with it removed where pad is None; the variable is gone again afterwards."""
    with monkeypatch.context() as m:
        if pad is None:
            m.delenv(ENV, raising=False)
        else:
            m.setenv(ENV, str(pad))
        return [pkg.Engine(cfg, 0) for _ in range(count)]


def assert_pad_took(unpadded, padded, cfg, pad, where=""):
    """Without this a test proves nothing: the padded handle's image is exactly stride_padded / stride_unpadded times the twin's."""
    su, sp = round_up(cfg.batch), round_up(cfg.batch) + pad
    iu, ip = unpadded.observable_image_bytes(), padded.observable_image_bytes()
    assert ip * su == iu * sp and ip > iu, f"{where}: the pad of {pad} columns did not take (images {iu} and {ip} B, strides {su} and {sp} expected)"
    assert stride_of(unpadded, cfg, unpadded) == su and stride_of(padded, cfg, unpadded) == sp, f"{where}: stride_of disagrees with the image sizes"


def twins(pkg, cfg, monkeypatch, pad, pose=None, padded=1, where=""):
    """(the unpadded handle, [padded handles]) at `pose`, the pad checked on every padded one."""
    (u,) = create(pkg, cfg, monkeypatch, None)
    ps = create(pkg, cfg, monkeypatch, pad, padded)
    for p in ps:
        assert_pad_took(u, p, cfg, pad, where)
    if pose is not None:
        for e in [u] + ps:
            gd.put(e, cfg, pose)
    return u, ps


def state_everything(eng, cfg):
    """{name: array}: everything the getters return for the handle's stages - raw state (the f64 getters on precision = 64, and the
    float getters of the double rows), joint states and observables (parity.state_of), what the verdict is a function of
    (done_handles.getters: FK residual, infeasible flag, limit bits, episode start, step count), fk_state, td_state, pid_debug."""
    from cdpr_simulation_amd import _abi

    f64 = cfg.precision == 64
    names = ("raw_pose", "raw_twist", "q", "qd", "effort", "pose", "twist") if f64 else \
            ("raw_pose", "raw_twist", "joint_q", "joint_qd", "joint_effort", "q", "qd", "effort", "pose", "twist")
    got = parity.state_of(eng, f64, joint_states=True)
    assert len(got) == len(names), f"state_everything: parity.state_of returned {len(got)} arrays"
    out = dict(zip(names, got))
    if f64:
        out.update(zip(("raw_pose_f32", "raw_twist_f32", "joint_q", "joint_qd", "joint_effort"), eng.raw_state() + eng.joint_states()))
    for k, v in gd.getters(eng, cfg).items():
        if k not in ("pose", "twist", "f64") and v is not None:
            out[k] = np.asarray(v)
    if cfg.stages & _abi.STAGE_FK:
        out.update(zip(("fk_pose", "fk_residual", "fk_iterations"), eng.fk_state()))
    if cfg.stages & _abi.STAGE_TD:
        out.update(zip(("tension", "infeasible"), eng.td_state()))
    if cfg.stages & _abi.STAGE_PID_DEBUG:
        out["pid_debug"] = eng.pid_debug()
    return out


def assert_same(got, want, where, rows=EVERY, rows_want=None):
    """np.array_equal on every entry of two state_everything dicts: rows `rows` of `got` against rows `rows_want` (default: the same)
    of `want`.  No exception of any kind."""
    rows_want = rows if rows_want is None else rows_want
    assert set(got) == set(want), f"{where}: the getters differ ({sorted(set(got) ^ set(want))})"
    for k, x in got.items():
        x, y = np.asarray(x), np.asarray(want[k])
        if x.ndim == 0:
            assert x == y, f"{where}: {k} is {x}, not {y}"
            continue
        x, y = x[rows], y[rows_want]
        if not (x.dtype == y.dtype and np.array_equal(x, y)):
            bad = np.flatnonzero((x != y).reshape(len(x), -1).any(axis=1)) if x.shape == y.shape else "(shapes differ)"
            raise AssertionError(f"{where}: {k} differs to the bit ({x.dtype} / {y.dtype}) on rows {bad[:8] if not isinstance(bad, str) else bad}")


def against_the_oracle(eng, ora, cfg, where, rows=EVERY, ora_rows=None):
    """parity.against_the_oracle (TOL, or TOL64 on precision = 64, every quantity finite) on the robots `rows` of the engine against the
    robots `ora_rows` of the oracle (default: the same rows): before a copy the twin-from-birth oracle holds the sources' rows where the
    engine still holds the destinations' own."""
    f64 = cfg.precision == 64
    if rows is EVERY and ora_rows is None:
        return parity.against_the_oracle(eng, ora, f64, where, printed="padded stride")
    ora_rows = rows if ora_rows is None else ora_rows
    worst = {}
    for name, g, o in zip(parity.NAMES, parity.observed(eng, f64), parity.observed(ora)):
        g, o = np.asarray(g)[rows], np.asarray(o)[ora_rows]
        assert not f64 or g.dtype == np.float64, f"{where}: {name} is {g.dtype}, not float64"
        assert np.isfinite(g).all(), f"{where}: {name} is not finite"
        worst[name] = (float(np.abs(g - o).max()) if g.size else 0.0, 0, 0)
    parity.assert_within(worst, parity.TOL64 if f64 else parity.TOL, where)
    return worst


def assert_record_is_published(rec, state, where):
    """the last image of an update_record (decoded by cdpr_decode_observables[_f64]) is what the getters publish"""
    for key, name in (("position", "q"), ("velocity", "qd"), ("effort", "effort"), ("pose", "pose"), ("twist", "twist")):
        assert rec[key].dtype == state[name].dtype and np.array_equal(rec[key][-1], state[name]), f"{where}: the record's last image is not the published one ({key})"


# ---- configurations ---------------------------------------------------------------------------------------------------------------
def ops_config(pkg, kind, monkeypatch, batch=None):
    """per_robot_kinds.config_of with done_handles.limited travel limits (bits only: travel_stop is 0, the dynamics are those of the
    reset and copy tests), at `batch` robots where given."""
    cfg = prk.config_of(pkg, kind, monkeypatch)
    return replace(cfg, model=gd.limited(cfg.model), **({} if batch is None else dict(batch=batch)))


def view_extras(stages):
    """test_gpu_done's "after real steps": tension bounds of 1 .. 12 N and one FK iteration per step where the handle has the stages"""
    return dict(tdFMin=1.0, tdFMax=12.0, fkMaxIterations=1) if stages == 3 else {}


def view_config(pkg, kind, monkeypatch):
    if kind in gd.KINDS:
        n = gd.UNIFORM[kind][0] if kind in gd.UNIFORM else 8
        return gd.config_of(pkg, kind, monkeypatch, gd.limited, **(view_extras(3) if n >= 6 else {}))
    cfg = prk.config_of(pkg, kind, monkeypatch)
    return replace(cfg, model=gd.limited(cfg.model), **view_extras(cfg.stages))


VIEW_SEED, VIEW_STEPS = 301, ri.HISTORY  # (test_after_real_steps' own)


def view_rule(pkg, cfg, residual):
    """(rule, robot k): TRAVEL and, where the handle has the stages, INFEASIBLE and FK_RESIDUAL with the threshold one value below the
    residual of robot k, a robot with a middle residual: k is done by it, some robots are not (test_after_real_steps' second rule)."""
    enable, k, thr = dr.TRAVEL, 0, 0.0
    if cfg.stages & 2:
        enable |= dr.INFEASIBLE
    if cfg.stages & 1:
        res = np.asarray(residual, dtype=np.float32)
        distinct = np.unique(res)
        assert len(distinct) >= 3, f"view_rule: the FK residuals do not spread ({distinct})"
        k = int(np.nonzero(res == distinct[len(distinct) // 2])[0][0])
        enable, thr = enable | dr.FK_RESIDUAL, float(np.nextafter(res[k], np.float32(-np.inf)))
    return pkg.DoneRule(enable=enable, max_fk_residual=thr), k


def edge_rule(pkg, age):
    """section 4: TRAVEL, and TIMEOUT at the age of the robots that were never reset"""
    return pkg.DoneRule(enable=dr.TRAVEL | dr.TIMEOUT, max_steps=int(age))


def assert_counts_are_live(counts, rule, batch, where):
    """each enabled bit's count strictly between 0 and B: the rule tells the robots apart (a count over the pad columns, which hold the
    home state, or over too few robots cannot hide).  One robot has no `between`: there the count is 0 or 1."""
    for k, name in enumerate(dr.BIT_NAMES):
        if (int(rule.enable) >> k) & 1:
            c = int(counts[1 + k])
            assert (0 < c < batch) if batch > 1 else c in (0, 1), f"{where}: {c} of {batch} robots are done by `{name}`: the rule does not tell the robots apart"


def oracle_getters(ora, cfg, start=None):
    """done_handles.getters of an oracle (float64; the episode clock kept by the caller, default: no reset yet)"""
    pose, twist = ora.raw_state()
    return dict(pose=pose, twist=twist, fk_residual=ora.fk_state()[1] if cfg.stages & 1 else None, infeasible=ora.td_state()[1] if cfg.stages & 2 else None,
                limit_mask=ora.limit_state(), start=np.zeros(cfg.batch, np.uint32) if start is None else start, step_count=ora.step_count, f64=True)


# ---- the margin from the home state -----------------------------------------------------------------------------------------------
def home_margin(observed, home, tol):
    """min over robots of max(|pose - home| / tol[pose], |effort| / tol[eff]): how far, in units of the comparison tolerance, the
    closest robot is from what a pad column holds (the home pose, zero efforts).  Above 1 on the oracle means that a kernel which read a
    pad column for some robot could not pass the comparison with the oracle."""
    pose, eff = np.asarray(observed[0], dtype=np.float64), np.asarray(observed[4], dtype=np.float64)
    d = np.maximum(np.abs(pose - np.asarray(home, dtype=np.float64)).max(axis=1) / tol["pose"], np.abs(eff).max(axis=1) / tol["eff"])
    return float(d.min())


def cell_states_on_the_oracle(pkg, oracle, cell):
    """(cfg, [observed after every segment of wp.SCRIPT]) of a workspace cell on the oracle alone, the cell's own seed and inputs"""
    cfg, _, seed = wp.cell_config(pkg, cell)
    rng = np.random.default_rng(seed)
    pose = wp.start_poses(cfg.model, cfg.batch, rng)
    cmds = wp.script_commands(rng, cfg.batch, cfg.n_cables)
    ora = oracle.OracleSim(cfg.to_struct(), oracle.DERIV_EXACT)
    ora.set_platform_state(pose7=pose.astype(np.float64))
    used, out = {}, []
    for kind, k in wp.SCRIPT:
        cmd = wp.segment_command(kind, cmds, ora, used)
        if cmd is not None:
            getattr(ora, wp.SETTER[kind])(cmd)
        ora.update(k)
        out.append(parity.observed(ora))
    ora.close()
    return cfg, out


# ---- masks and maps ---------------------------------------------------------------------------------------------------------------
def edge_masks(batch):
    """section 4's resets: robot 0, robot B - 1, every third robot"""
    out = [np.zeros(batch, np.uint8) for _ in range(3)]
    out[0][0], out[1][batch - 1] = 1, 1
    out[2][::3] = 1
    return out


def edge_map(batch):
    """Section 4's copy: every third robot but the last is a destination; its source lies half a batch away (in another wavefront from
    65 robots on), is no destination and sits in another `index mod 3` group (the mode changes); robot 0 takes robot B - 1.  One robot:
    nothing to copy."""
    source = np.full(batch, -1, dtype=np.int32)
    if batch == 1:
        return source
    dest = np.zeros(batch, bool)
    dest[0:batch - 1:3] = True
    for d in np.flatnonzero(dest):
        s = (d + batch // 2) % batch
        while dest[s] or s % 3 == d % 3:
            s = (s + 1) % batch
        source[d] = s
    source[0] = batch - 1
    return source


def spread_mask(batch=FULL_B):
    """section 5's reset: every 61st robot (one or two in every wavefront) and robots 0, 65 535, 65 536, B - 1"""
    m = np.zeros(batch, np.uint8)
    m[::61] = 1
    m[[0, batch // 2 - 1, batch // 2, batch - 1]] = 1
    return m


def other_half_map(batch=FULL_B):
    """section 5's copy: every 101st robot that spread_mask leaves alone takes the robot half a batch away (+1 where that one is a
    destination itself); robot 1 takes robot B - 2"""
    m = spread_mask(batch).astype(bool)
    source = np.full(batch, -1, dtype=np.int32)
    dest = np.zeros(batch, bool)
    dest[5::101] = True
    dest &= ~m
    dest[[1]] = True
    for d in np.flatnonzero(dest):
        s = (d + batch // 2) % batch
        while dest[s]:
            s = (s + 1) % batch
        source[d] = s
    source[1] = batch - 2
    assert not dest[batch - 2], "other_half_map: robot B - 2 is a destination"
    return source


def waves_touched(rows, batch):
    """the wavefronts (of 64 robots) that hold a robot of `rows`, and whether all of the batch's are among them"""
    w = set(int(r) // 64 for r in np.flatnonzero(rows))
    return w, w == set(range((batch + 63) // 64))


def twin_inputs(inputs, source):
    """cr.twin_rows where there is a map, else the inputs themselves"""
    return inputs if source is None else cr.twin_rows(inputs, source)


# ---- the chain of sections 4 and 5: history, resets, a copy, on engines and on the twin-from-birth oracle --------------------------
def chain_inputs(model, batch, seed):
    """History and after inputs at `batch` robots, the reset masks and the copy map; `born`: the same with every destination's rows -
    its reset flags too - replaced by its source's, what an oracle that is the twin from birth is driven by."""
    h, a = ri.history_inputs(model, seed, batch=batch), ri.after_inputs(model, seed + 1, batch=batch)
    masks = edge_masks(batch)
    source = edge_map(batch)
    plain = dict(pose=h["pose"], p=h["p"], v=h["v"], f=h["f"], group=h["group"], fresh=a["pose"], v2=a["v"], v2_mask=a["v_mask"],
                 m0=masks[0], m1=masks[1], m2=masks[2])
    return plain, cr.twin_rows(plain, source), source


CHAIN_HISTORY = 12
CHAIN_STEPS = (("m0", 2), ("m1", 2), ("m2", 5))  # (mask, steps behind the reset)


def chain_history(sims, x, steps=CHAIN_HISTORY):
    ri.play_history(sims, dict(p=x["p"], v=x["v"], f=x["f"], group=x["group"]), steps)


def chain_reset_on_the_oracle(ora, x, key):
    if x[key].any():
        ri.oracle_reset(ora, x[key], x["fresh"])


# ---- section 3's ops --------------------------------------------------------------------------------------------------------------
OPS = ("reset", "reset_device", "copy", "copy_device", "resample")
RESAMPLE_P = 65  # (section 4 of tests/test_gpu_resample.py)


def resample_weights():
    w = ro.pattern("heavy_tail", RESAMPLE_P, B // RESAMPLE_P, seed=10)
    w[3], w[70] = np.nan, -1.0
    return w, np.array([123456789, 4000000000], np.uint32)


def ops_inputs(model, op, seed=131):
    """(history, after, their twinned forms for the oracle, mask or None, source map or None, the restatement's resample or None)"""
    h, a = ri.history_inputs(model, seed), ri.after_inputs(model, seed + 1)
    mask = source = want = None
    if op.startswith("reset"):
        mask = ri.reset_mask()
    elif op.startswith("copy"):
        source = cr.copy_map()
    else:
        w, words = resample_weights()
        want = ro.resample(w, RESAMPLE_P, words)
        source = want[0]
    return h, a, twin_inputs(h, source), twin_inputs(a, source), mask, source, want
