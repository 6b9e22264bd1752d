"""Every kernel family and every call over chosen robots on a PADDED row stride (helpers, pads and the reasons: tests/padded_stride.py).

cdpr_create pads the stride only at 131 072, 262 144 and 524 288 robots; CDPR_STRIDE_PAD forces the same layout at B = 130, where the
whole matrix runs in seconds.  Two assertions throughout, on ALL B robots:
  same bits   a padded handle equals its unpadded twin on everything a caller can read (np.array_equal, no exception of any kind):
              robot r sits in the same lane either way, no arithmetic may move;
  reference   the padded handle is held to the reference of the same call at the tolerance the unpadded tests hold: the fp64 oracle at
              TOL / TOL64 (tests/parity.py), done_rules.done_reference, resample_oracle's restatement, the getters for observation
              columns, env_view.reward_reference - the same-bits check would pass if both layouts were wrong in the same way.
Every test first asserts that the pad took (padded_stride.assert_pad_took, on the size of the observable image).

  1  step kernels: the 21 cells of workspace_poses.CELLS over wp.SCRIPT; unpadded one-step launches against pad 128 one-step, pad 128
     update(k, 10) and pad 64 update_record(k, 10); kernel_name = plan_kernel (the pad does not change the routing); FK estimates and
     iteration counts, tensions and flags against the oracle's under test_closed_loop_cell_over_the_wide_box's rule (flags may differ
     only within 2e-2 N of a bound and on at most 1 % of the robots).  test_zy_every_family_ran_on_a_padded_handle.
  2  launch forms behind reset and copy: launch_forms.KINDS x FORMS on pad 128 against form `one` on the unpadded handle, the padded
     `one` against the oracle Player; then rollout_velocity twice (3 samples, then 2: the rollout's record column stride stays at the
     first call's 448, unlike batch x samples = 260 and unlike the handle's 320).  test_zy_every_kind_and_form_ran_on_a_padded_handle.
  3  a. reset_robots[_device], copy_robots[_device] (status words), resample fused (P = 65: map, ess bits, five status words) on the
        nine per-robot kinds at pads 64 and 128, travel limits of +-15 mm so that the limit bits are live: twins equal, destinations equal
        their sources, untouched robots equal their state before, then ri.play_after against the oracle (the recipe; the twin from birth).
     b. evaluate_done[_device], reset_done_device, observe_device and env_evaluate_device (every field, ld = width + 2, a row mask over
        every wave and robot B - 1, sentinels), update_record on done_handles.KINDS and the six other per-robot kinds.
  4  batch edges B = 1, 63, 64, 65, 257 on one kind per record layout, pad 64 against none: resets of robot 0, of robot B - 1, of every
     third robot, the done rule, the observation, a copy across waves with B - 1 onto 0 - one chain, the oracle its twin from birth.
  5  the create rule itself: B = 131 072 pads by itself; against CDPR_STRIDE_PAD=0; three 128-robot slices on the oracle.

Measured on MI355X (173 cases, 8 s; HISTORY.md section 25): every family, form and call was bit equal to the unpadded layout at both pads
and at every batch; no kernel or host routine changed.  Worst error of a padded handle against the oracle: fp32 pose 5.7e-7, twist 8.9e-5,
q 5.1e-7, qd 9.6e-5, effort 4.5e-3 N; fp64 pose 3.2e-15, effort 2.2e-11 N; rollouts within 0.06 (fp32) and 0.11 (fp64) of their tolerance.
With the done kernel's stride taken as round_up(batch, 64) on a scratch build, the 18 fp32 cases of 3b fail (mask differs from
done_reference from robot 0 on) while tests/test_gpu_done.py and tests/test_gpu_env_view.py pass all their 74 cases.
"""
import numpy as np
import pytest

import copy_robots as cr
import done_handles as gd
import done_rules as dr
import env_view as ev
import launch_forms as lf
import padded_stride as ps
import parity
import per_robot_kinds as prk
import robot_histories as ri
import workspace_poses as wp
from parity import TOL

pytestmark = pytest.mark.gpu

clean_env = prk.clean_env  # (autouse here too: clears CDPR_STRIDE_PAD with the routing overrides)

B = ps.B
EVERY = ps.EVERY
FIRST, NOT_STEADY = 1, 8  # CDPR_PLAN_* (include/cdpr.h)
RAN = {}           # section 1: cell -> kernel names that ran on padded handles
FORMS_RAN = set()  # section 2: (kind, form) that ran on a padded handle, every launch on the planned kernel
CANARY8, CANARY32 = 0xA5, 0xDEADBEEF


def state(eng, cfg):
    return ps.state_everything(eng, cfg)


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", list(wp.CELLS))
def test_step_kernels_on_a_padded_stride(pkg, oracle, monkeypatch, cell):
    cfg, env, seed = wp.cell_config(pkg, cell)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    f64, stages = cfg.precision == 64, cfg.stages
    s = cfg.to_struct()
    rng = np.random.default_rng(seed)
    pose = wp.start_poses(cfg.model, cfg.batch, rng)
    cmds = wp.script_commands(rng, cfg.batch, cfg.n_cables)
    # u: unpadded, one step per launch; p1: pad 128, one step per launch; p10: pad 128, fused; prec: pad 64, the trajectory record
    u, (p1, p10) = ps.twins(pkg, cfg, monkeypatch, 128, pose, padded=2, where=cell)
    (prec,) = ps.create(pkg, cfg, monkeypatch, 64)
    ps.assert_pad_took(u, prec, cfg, 64, cell)
    gd.put(prec, cfg, pose)
    ora = parity.oracle_at(oracle, cfg, pose)
    ran = RAN.setdefault(cell, set())
    used = {}
    for kind, k in wp.SCRIPT:
        where = f"{cell}, {kind}"
        cmd = wp.segment_command(kind, cmds, ora, used)
        if cmd is not None:
            for sim in (u, p1, p10, prec, ora):
                getattr(sim, wp.SETTER[kind])(cmd)
        u.update(k), p1.update(k), p10.update(k, 10), ora.update(k)
        rec = prec.update_record(k, 10)
        # the pad does not change the routing (derived as test_closed_loop_cell_over_the_wide_box derives it)
        flags = (FIRST | NOT_STEADY) if kind == "hold" else NOT_STEADY if kind == "force" else 0
        planned = pkg.plan_kernel(cfg, k - 10 * ((k - 1) // 10), flags)
        if kind == "hold" and pkg.plan_kernel(cfg, 10).startswith(("cdpr_gen_split", "cdpr_gen_lean")):
            planned = pkg.plan_kernel(cfg, 1, NOT_STEADY)
        assert u.kernel_name == p1.kernel_name == pkg.plan_kernel(cfg, 1), where
        assert p10.kernel_name == planned == prec.kernel_name, where
        ran.update((p1.kernel_name, p10.kernel_name, prec.kernel_name))
        # same bits
        su = state(u, cfg)
        for e, form in ((p1, "pad 128, one-step"), (p10, "pad 128, fused"), (prec, "pad 64, recorded")):
            ps.assert_same(state(e, cfg), su, f"{where}: {form} against unpadded one-step launches")
        ps.assert_record_is_published(rec, su, where)
        # the oracle
        ps.against_the_oracle(p1, ora, cfg, where)
        if stages & 1:
            fp, _, fi = p1.fk_state()
            op, _, oi = ora.fk_state()
            assert np.array_equal(fi, oi), f"{where}: FK iteration counts"
            assert np.abs(fp - op).max() <= 1e-5, f"{where}: FK estimate differs from the oracle's by {np.abs(fp - op).max():.3e}"
        if stages & 2:
            tt, tf = p1.td_state()
            ot, of = ora.td_state()
            assert np.abs(tt - ot).max() <= TOL["eff"], f"{where}: tensions differ by {np.abs(tt - ot).max():.3e}"
            near = wp.near_bound(ot, float(s.td_f_min), float(s.td_f_max), 2e-2)
            differ = tf != of
            assert not differ[~near].any(), f"{where}: infeasibility flags differ away from the bounds"
            assert differ.mean() <= 0.01, f"{where}: flags differ on {differ.sum()} robots"
    for e in (u, p1, p10, prec, ora):
        e.close()


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,op", [(kind, op) for kind in lf.KINDS for op in ("reset", "copy")])
def test_launch_forms_on_a_padded_stride(pkg, oracle, monkeypatch, kind, op):
    def make(cfg, pose, forms):
        u, padded = ps.twins(pkg, cfg, monkeypatch, 128, pose, padded=len(forms) - 1, where=kind)
        return [u] + padded

    sc = lf.Scenario(pkg, oracle, monkeypatch, kind, op, ("one",) + lf.FORMS, 301, make=make)
    cfg, general = sc.cfg, kind in lf.GENERAL
    one_u, padded, ora = sc.players[0], sc.players[1:], sc.ora.sim
    one_p = padded[0]
    assert [p.form for p in padded] == list(lf.FORMS) and one_p.form == "one"

    def same_bits(label):
        base = state(one_u.sim, cfg)
        for p in padded:
            ps.assert_same(state(p.sim, cfg), base, f"{kind}, {op}, {label}: form {p.form} on the padded handle against `one` on the unpadded")

    same_bits("the end of the history")
    ps.against_the_oracle(one_p.sim, ora, cfg, f"{kind}, {op}, the end of the history", rows=EVERY if op == "reset" else ~sc.touched)
    sc.apply()
    same_bits(f"right after the {op}")

    def check(label, k):
        same_bits(label)
        ps.against_the_oracle(one_p.sim, ora, cfg, f"{kind}, {op}, {label}")

    sc.play_after(check)
    for p in padded:
        assert len(p.launches) == 5, (kind, p.form)
        for last, name in p.launches:
            assert name == pkg.plan_kernel(cfg, last), (kind, p.form, last, name)
        FORMS_RAN.add((kind, p.form))
    # the rollout behind it all, twice: 3 samples, then 2 on record columns that stay as wide as the first call made them
    roll = lf.rollout_inputs(cfg, sc.a["pose"], 331)
    if op != "reset":
        roll = cr.twin_rows(roll, sc.source)
    before = state(one_p.sim, cfg)
    for samples in (lf.SAMPLES, 2):
        cmds, ref = np.ascontiguousarray(roll["cmds"][:, :, :samples]), roll["ref"]
        where = f"{kind}, {op}, rollout of {samples} samples"
        costs = [p.sim.rollout_velocity(cmds, ref) for p in sc.players]
        assert costs[0].shape == (B, samples) and np.isfinite(costs[0]).all(), where
        assert one_p.sim.kernel_name == pkg.plan_kernel(cfg, cmds.shape[1], flags=pkg._abi.PLAN_ROLLOUT), (where, one_p.sim.kernel_name)
        for p, c in zip(padded, costs[1:]):
            assert np.array_equal(c, costs[0]), f"{where}: the costs of form {p.form} on the padded handle differ from the unpadded handle's"
        oc = ora.rollout_velocity(cmds, ref.astype(np.float64))
        err, bound = float(np.abs(costs[1] - oc).max()), lf.rollout_tolerance(cfg, general, oc)
        print(f"padded stride ROLLOUT {where}: max |cost - oracle| {err:.3e} = {err / bound:.3f} x the tolerance")
        assert err <= bound, f"{where}: the costs differ from the oracle's by {err:.3e} (tolerance {bound:.3e})"
    ps.assert_same(state(one_p.sim, cfg), before, f"{kind}, {op}: the rollouts changed what a getter returns")
    sc.close()


# ---- 3a ------------------------------------------------------------------------------------------------------------------------
def apply_op(pkg, eng, op, a, mask, source, want, where):
    """one op of padded_stride.OPS on one engine, its own outputs checked"""
    if op == "reset":
        eng.reset_robots(mask, a["pose"])
    elif op == "reset_device":
        bufs = ev.Buffers(eng)
        eng.reset_robots_device(bufs.upload(mask), bufs.upload(a["pose"]))
        bufs.free()
    elif op == "copy":
        eng.copy_robots(source)
    elif op == "copy_device":
        bufs = ev.Buffers(eng)
        d_status = bufs.upload(np.array([7, 7], np.uint32))
        eng.copy_robots_device(bufs.upload(source), d_status)
        status = eng.device_download(d_status, (2,), np.uint32)
        assert np.array_equal(status, [int(cr.destinations_of(source).sum()), 0]), f"{where}: status words {status}"
        bufs.free()
    else:
        w, words = ps.resample_weights()
        got = eng.resample(w, words, ps.RESAMPLE_P)
        assert want[2][0] > 20 and cr.validate_map(want[0]) is None, where
        for name, g, x in zip(("map", "ess", "status"), got, want):
            assert g.dtype == x.dtype and np.array_equal(g.view(np.uint32), x.view(np.uint32)), f"{where}: {name} differs from the restatement: {g.ravel()[:8]} / {x.ravel()[:8]}"


@pytest.mark.parametrize("pad", ps.PADS)
@pytest.mark.parametrize("op", ps.OPS)
@pytest.mark.parametrize("kind", ps.OPS_KINDS)
def test_robot_ops_on_a_padded_stride(pkg, oracle, monkeypatch, kind, op, pad):
    cfg = ps.ops_config(pkg, kind, monkeypatch)
    h, a, ht, at, mask, source, want = ps.ops_inputs(cfg.model, op)
    touched = mask.astype(bool) if source is None else cr.destinations_of(source)
    where = f"{kind}, {op}, pad {pad}"
    u, (p,) = ps.twins(pkg, cfg, monkeypatch, pad, h["pose"], where=where)
    ora = parity.oracle_at(oracle, cfg, ht["pose"])
    ri.play_history([u, p], h)
    ri.play_history([ora], ht)
    before = state(u, cfg)
    ps.assert_same(state(p, cfg), before, f"{where}, the end of the history")
    assert 0 < (before["limit_mask"] != 0).sum() < B, f"{where}: the travel bits do not tell the robots apart"
    ps.against_the_oracle(p, ora, cfg, f"{where}, the end of the history", rows=~touched)
    steps = p.step_count
    for e in (u, p):
        apply_op(pkg, e, op, a, mask, source, want, where)
    after = state(p, cfg)
    assert p.step_count == steps
    ps.assert_same(after, state(u, cfg), f"{where}, right after")
    ps.assert_same(after, before, f"{where}: a robot the op does not touch changed", rows=~touched)
    if source is None:
        fresh = a["pose"].astype(after["raw_pose"].dtype)
        assert np.array_equal(after["raw_pose"][touched], fresh[touched]) and not after["raw_twist"][touched].any(), f"{where}: a reset robot is not at its fresh pose"
        assert (after["start"][touched] == steps).all() and not after["start"][~touched].any(), f"{where}: the episode clock"
        ri.oracle_reset(ora, mask, a["pose"])
    else:
        assert not np.array_equal(before["raw_pose"][touched], before["raw_pose"][source[touched]]), where  # (the history tells them apart)
        ps.assert_same(after, before, f"{where}: a destination is not its source", rows=touched, rows_want=source[touched])

    def check(label):
        ps.assert_same(state(p, cfg), state(u, cfg), f"{where}, {label}")
        ps.against_the_oracle(p, ora, cfg, f"{where}, {label}")

    ri.play_after([u, p, ora], at, check)
    for e in (u, p, ora):
        e.close()


# ---- 3b ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", ps.PADS)
@pytest.mark.parametrize("kind", ps.VIEW_KINDS)
def test_verdicts_view_and_read_out_on_a_padded_stride(pkg, monkeypatch, kind, pad):
    cfg = ps.view_config(pkg, kind, monkeypatch)
    f64 = cfg.precision == 64
    where = f"{kind}, pad {pad}"
    h = ri.history_inputs(cfg.model, ps.VIEW_SEED)
    u, (p,) = ps.twins(pkg, cfg, monkeypatch, pad, h["pose"], where=where)
    gd.drive([u, p], cfg, h, ps.VIEW_STEPS)
    ps.assert_same(state(p, cfg), state(u, cfg), f"{where}, every getter after {ps.VIEW_STEPS} steps")
    bp, bu = ev.Buffers(p), ev.Buffers(u)
    # the verdict: host form, device form (canaries behind row B and behind the counts), the twin's
    g = gd.getters(p, cfg)
    rule, k = ps.view_rule(pkg, cfg, g["fk_residual"])
    got = p.evaluate_done(rule)
    print(f"padded stride, done, {where}: counts {got[2][:10].tolist()}")
    gd.assert_verdict(got, dr.done_reference(rule, **g), f"{where}, the reference on the padded handle's own getters")
    gd.assert_verdict(got, u.evaluate_done(rule), f"{where}, the unpadded twin's verdict")
    ps.assert_counts_are_live(got[2], rule, B, where)
    assert not cfg.stages & 1 or got[1][k] & dr.FK_RESIDUAL, f"{where}: one value above the threshold is done"
    rows = B + 70
    d_mask, d_reason = bp.upload(np.full(rows, CANARY8, np.uint8)), bp.upload(np.full(rows, CANARY32, np.uint32))
    d_counts = bp.upload(np.full(2 * dr.COUNTS, CANARY32, np.uint32))
    p.evaluate_done_device(rule, d_mask, d_reason, d_counts)
    m, r, c = p.device_download(d_mask, rows, np.uint8), p.device_download(d_reason, rows, np.uint32), p.device_download(d_counts, 2 * dr.COUNTS, np.uint32)
    gd.assert_verdict((m[:B], r[:B], c[:dr.COUNTS]), got, f"{where}, device form")
    assert (m[B:] == CANARY8).all() and (r[B:] == CANARY32).all() and (c[dr.COUNTS:] == CANARY32).all(), f"{where}: the device form wrote past row B"
    # the observation: every field alone and all of them against the getters; a row mask over every wave and robot B - 1
    every = ev.fields_of(cfg)
    want_obs = ev.observation_reference(every, **ev.check_observation(p, cfg, bp, where))
    width = want_obs.shape[1]
    chosen = ri.reset_mask() * np.uint8(3)
    assert ps.waves_touched(chosen, B)[1] and chosen[B - 1] and not chosen.all()
    sel = np.zeros(B + 7, bool)
    sel[:B] = chosen != 0
    tensors = [ev.observe_padded(e, b, every, width + 2, B, b.upload(chosen)) for e, b in ((p, bp), (u, bu))]
    assert np.array_equal(tensors[0][sel, :width], want_obs[chosen != 0]), f"{where}: a chosen row is not the getters' columns"
    assert (tensors[0][~sel] == ev.SENTINEL).all() and (tensors[0][:, width:] == ev.SENTINEL).all(), f"{where}: an unchosen row or a slack column changed"
    assert np.array_equal(tensors[0], tensors[1]), f"{where}: the masked observation differs from the unpadded twin's"
    # observation, reward and verdict in one launch
    _, weights, _, _, target = ev.scenario(pkg, cfg.model, f64)
    spec = ev.spec_of(pkg, cfg, rule, weights, fields=every, ld=width + 2)
    outs = []
    for e, b in ((p, bp), (u, bu)):
        d = [b.upload(np.full((B + 7, width + 2), ev.SENTINEL, np.float32)), b.upload(np.full(B + 7, ev.SENTINEL, np.float32)), b.upload(np.full(B + 7, CANARY8, np.uint8)),
             b.upload(np.full(B + 7, CANARY32, np.uint32)), b.upload(np.full(2 * dr.COUNTS, CANARY32, np.uint32))]
        e.env_evaluate_device(spec, b.upload(target), *d)
        outs.append([e.device_download(x, shape, dt) for x, shape, dt in zip(d, ((B + 7, width + 2), B + 7, B + 7, B + 7, 2 * dr.COUNTS), (np.float32, np.float32, np.uint8, np.uint32, np.uint32))])
    obs, reward, mask, reason, counts = outs[0]
    for name, x, y in zip(("obs", "reward", "mask", "reason", "counts"), *outs):
        assert np.array_equal(x, y), f"{where}: {name} of env_evaluate_device differs from the unpadded twin's"
    assert np.array_equal(obs[:B, :width], want_obs) and (obs[B:] == ev.SENTINEL).all() and (obs[:, width:] == ev.SENTINEL).all(), f"{where}: the observation of env_evaluate_device"
    gd.assert_verdict((mask[:B], reason[:B], counts[:dr.COUNTS]), got, f"{where}, the verdict of env_evaluate_device")
    assert (reward[B:] == ev.SENTINEL).all() and (mask[B:] == CANARY8).all() and (reason[B:] == CANARY32).all() and (counts[dr.COUNTS:] == CANARY32).all(), f"{where}: env_evaluate_device wrote past row B"
    ref, M = ev.reward_reference(spec, reason=reason[:B], target7=target, home=cfg.model.home_pose(), **ev.reward_getters(p, cfg))
    assert np.isfinite(ref).all() and ev.inside(reward[:B], ref, M, f64).all(), f"{where}: the reward leaves the bound for robots {np.nonzero(~ev.inside(reward[:B], ref, M, f64))[0][:8]}"
    if kind in gd.KINDS:  # (test_view_static_and_after_steps' own handles and history: its whole comparison)
        ev.check_reward_and_verdict(pkg, p, cfg, rule, weights, target, where)
    # read-out: the record (cdpr_decode_observables[_f64] of a padded image) against the getters and against the twin's
    rec_p, rec_u = p.update_record(4, 2), u.update_record(4, 2)
    sp = state(p, cfg)
    ps.assert_record_is_published(rec_p, sp, where)
    for key in rec_p:
        assert np.array_equal(rec_p[key], rec_u[key]), f"{where}: the record differs from the unpadded twin's ({key})"
    ps.assert_same(sp, state(u, cfg), f"{where}, behind the record")
    # evaluate and reset in one call
    if cfg.perRobotCommands:
        want = p.evaluate_done(rule)
        done = want[0].astype(bool)
        assert done.any(), where
        for e, b in ((p, bp), (u, bu)):
            d_c = b.upload(np.full(2 * dr.COUNTS, CANARY32, np.uint32))
            e.reset_done_device(rule, 0, 0, d_c)
            cc = e.device_download(d_c, 2 * dr.COUNTS, np.uint32)
            assert np.array_equal(cc[:dr.COUNTS], want[2]) and (cc[dr.COUNTS:] == CANARY32).all(), f"{where}: the counts of reset_done_device"
        sp = state(p, cfg)
        ps.assert_same(sp, state(u, cfg), f"{where}, behind reset_done_device")
        home = np.asarray(cfg.model.home_pose(), dtype=np.float32)
        assert (p.raw_state()[0][done] == home).all() and (sp["start"][done] == p.step_count).all() and not sp["start"][~done].any(), f"{where}: reset_done_device did not reset exactly the done robots"
        u.update(5), p.update(5)
        ps.assert_same(state(p, cfg), state(u, cfg), f"{where}, 5 steps behind reset_done_device")
    bp.free(), bu.free()
    u.close(), p.close()


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", ps.EDGE_BATCHES)
@pytest.mark.parametrize("kind", prk.LAYOUTS)
def test_batch_edges_with_and_without_a_pad(pkg, oracle, monkeypatch, kind, batch):
    cfg = ps.ops_config(pkg, kind, monkeypatch, batch)
    x, born, source = ps.chain_inputs(cfg.model, batch, 411)
    dest = cr.destinations_of(source)
    where = f"{kind}, B = {batch}"
    u, (p,) = ps.twins(pkg, cfg, monkeypatch, 64, x["pose"], where=where)
    ora = parity.oracle_at(oracle, cfg, born["pose"])
    ps.chain_history([u, p], x)
    ps.chain_history([ora], born)

    def both(label, rows):
        ps.assert_same(state(p, cfg), state(u, cfg), f"{where}, {label}")
        ps.against_the_oracle(p, ora, cfg, f"{where}, {label}", rows=rows)

    both("the history", ~dest)
    for key, steps in ps.CHAIN_STEPS:
        before, m = state(u, cfg), x[key].astype(bool)
        for e in (u, p):
            e.reset_robots(x[key], x["fresh"])
        ps.chain_reset_on_the_oracle(ora, born, key)
        after = state(p, cfg)
        ps.assert_same(after, state(u, cfg), f"{where}, right after the reset {key}")
        ps.assert_same(after, before, f"{where}, reset {key}: a robot outside the mask changed", rows=~m)
        assert np.array_equal(after["raw_pose"][m], x["fresh"].astype(after["raw_pose"].dtype)[m]), f"{where}, reset {key}: a reset robot is not at its fresh pose"
        for sim in (u, p, ora):
            sim.update(steps)
        both(f"{steps} steps after the reset {key}", ~dest)
    # the done rule and one full observation
    rule = ps.edge_rule(pkg, p.step_count)
    got = p.evaluate_done(rule)
    print(f"padded stride, done, {where}: counts {got[2][:10].tolist()}")
    gd.assert_verdict(got, gd.expect(p, cfg, rule), f"{where}, the reference on the padded handle's own getters")
    gd.assert_verdict(got, u.evaluate_done(rule), f"{where}, the unpadded twin's verdict")
    ps.assert_counts_are_live(got[2], rule, batch, where)
    bufs = ev.Buffers(p)
    every = ev.fields_of(cfg)
    want_obs = ev.observation_reference(every, **ev.check_observation(p, cfg, bufs, where, batch))
    assert np.array_equal(u.observe(every), want_obs), f"{where}: the unpadded twin's observation"
    # the copy: sources across waves, robot B - 1 onto robot 0; device form with its status words
    before = state(u, cfg)
    for e, b in ((u, ev.Buffers(u)), (p, bufs)):
        d_status = b.upload(np.array([7, 7], np.uint32))
        e.copy_robots_device(b.upload(source), d_status)
        assert np.array_equal(e.device_download(d_status, (2,), np.uint32), [int(dest.sum()), 0]), f"{where}: the status words of the copy"
        b.free()
    after = state(p, cfg)
    ps.assert_same(after, state(u, cfg), f"{where}, right after the copy")
    ps.assert_same(after, before, f"{where}, the copy: a robot that is no destination changed", rows=~dest)
    ps.assert_same(after, before, f"{where}, the copy: a destination is not its source", rows=dest, rows_want=source[dest])
    for sim in (u, p, ora):
        assert sim.set_velocity_command(born["v2"], mask=born["v2_mask"]) == 0
        sim.update(8)
    both("8 steps after the copy and a masked velocity Joy", EVERY)
    if kind not in lf.GENERAL:
        now = state(p, cfg)
        ps.assert_same(now, now, f"{where}, 8 steps on: destination and source have parted", rows=dest, rows_want=source[dest])
    for e in (u, p, ora):
        e.close()


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
def test_the_create_rule_pads_131072_robots(pkg, oracle, monkeypatch):
    """B = 131 072, n = 4, stages = 0, per-robot commands: the default handle (no variable set) has stride B + 128, its twin is created
    under CDPR_STRIDE_PAD=0.  Masked Joys as test_per_robot_handles_at_full_size (groups by (index // 7) mod 3), a reset spread over the
    batch, a copy from the other half, the done rule, one observation: equal to the bit; three 128-robot slices on the oracle, each
    the twin from birth of its robots."""
    N = ps.FULL_B
    rng = np.random.default_rng(1241)
    model = gd.limited(pkg.cube_model())
    kw = dict(model=model, stages=0, perRobotCommands=True)
    cfg = pkg.Config(batch=N, **kw)
    grp = (np.arange(N) // 7) % 3
    x = dict(pose=parity.perturbed_poses(model, N, rng, 0.03, 0.05).astype(np.float32), v1=rng.uniform(-0.03, 0.03, (N, 4)).astype(np.float32),
             p1=rng.uniform(-0.003, 0.003, (N, 4)).astype(np.float32), fresh=parity.perturbed_poses(model, N, rng, 0.03, 0.05).astype(np.float32),
             vel=(grp >= 1).astype(np.uint8), pos=(grp == 2).astype(np.uint8), reset=ps.spread_mask(N))
    source = ps.other_half_map(N)
    dest = cr.destinations_of(source)
    assert cr.validate_map(source) is None and x["reset"][[0, N // 2 - 1, N // 2, N - 1]].all() and (np.abs(source[dest] - np.flatnonzero(dest)) >= N // 2 - 1).all()
    born = cr.twin_rows(x, source)
    (p,) = ps.create(pkg, cfg, monkeypatch, None)  # the create rule's own pad
    (u,) = ps.create(pkg, cfg, monkeypatch, 0)
    ps.assert_pad_took(u, p, cfg, 128, "131 072 robots")
    assert ps.stride_of(p, cfg) == N + 128 and ps.stride_of(u, cfg) == N
    slices = (slice(0, 128), slice(N // 2 - 64, N // 2 + 64), slice(N - 128, N))
    oras = [parity.oracle_at(oracle, pkg.Config(batch=128, **kw), born["pose"][sl]) for sl in slices]
    for e in (u, p):
        e.set_platform_state(pose7=x["pose"])

    def everyone(fn):
        for e in (u, p):
            fn(e, x, EVERY)
        for o, sl in zip(oras, slices):
            fn(o, born, sl)

    def both(label, after_the_copy):
        ps.assert_same(state(p, cfg), state(u, cfg), f"131 072 robots, {label}")
        for o, sl in zip(oras, slices):
            rows = np.arange(sl.start, sl.stop)
            keep = np.ones(128, bool) if after_the_copy else ~dest[sl]
            ps.against_the_oracle(p, o, cfg, f"131 072 robots, {label}, robots {sl.start} .. {sl.stop - 1}", rows=rows[keep], ora_rows=keep)

    everyone(lambda e, i, sl: e.update(3))
    everyone(lambda e, i, sl: e.set_velocity_command(i["v1"][sl], mask=i["vel"][sl]))
    everyone(lambda e, i, sl: e.update(5))
    everyone(lambda e, i, sl: e.set_position_command(i["p1"][sl], mask=i["pos"][sl]))
    everyone(lambda e, i, sl: e.update(4))
    both("12 steps under masked Joys", False)
    before, m = state(u, cfg), x["reset"].astype(bool)
    for e in (u, p):
        e.reset_robots(x["reset"], x["fresh"])
    for o, sl in zip(oras, slices):
        ri.oracle_reset(o, born["reset"][sl], born["fresh"][sl])
    after = state(p, cfg)
    ps.assert_same(after, state(u, cfg), "131 072 robots, right after the reset")
    ps.assert_same(after, before, "131 072 robots, the reset: a robot outside the mask changed", rows=~m)
    assert np.array_equal(after["raw_pose"][m], x["fresh"][m])
    everyone(lambda e, i, sl: e.update(3))
    both("3 steps after the reset", False)
    # the done rule and one observation
    rule = ps.edge_rule(pkg, p.step_count)
    got = p.evaluate_done(rule)
    print(f"padded stride, done, 131 072 robots: counts {got[2][:10].tolist()}")
    gd.assert_verdict(got, gd.expect(p, cfg, rule), "131 072 robots, the reference on the padded handle's own getters")
    gd.assert_verdict(got, u.evaluate_done(rule), "131 072 robots, the unpadded twin's verdict")
    ps.assert_counts_are_live(got[2], rule, N, "131 072 robots")
    every = ev.fields_of(cfg)
    want_obs = ev.observation_reference(every, **ev.view_getters(p, cfg))
    assert np.array_equal(p.observe(every), want_obs) and np.array_equal(u.observe(every), want_obs), "131 072 robots: the observation"
    # the copy
    before = state(u, cfg)
    for e in (u, p):
        e.copy_robots(source)
    after = state(p, cfg)
    ps.assert_same(after, state(u, cfg), "131 072 robots, right after the copy")
    ps.assert_same(after, before, "131 072 robots, the copy: a robot that is no destination changed", rows=~dest)
    ps.assert_same(after, before, "131 072 robots, the copy: a destination is not its source", rows=dest, rows_want=source[dest])
    for e in (u, p):
        e.update(3)
    for o in oras:
        o.update(3)
    both("3 steps after the copy", True)
    for e in [u, p] + oras:
        e.close()


# ---- coverage ------------------------------------------------------------------------------------------------------------------
def test_zy_every_family_ran_on_a_padded_handle():
    """as test_zy_every_family_ran of tests/test_gpu_workspace.py, on what section 1 recorded of its PADDED handles"""
    missing = [fam for fam, (cell, pred) in wp.FAMILIES.items() if not any(pred(k) for k in RAN.get(cell, ()))]
    assert not missing, (f"families that did not run on a padded handle IN THIS PROCESS: {missing}.  This test reads what test_step_kernels_on_a_padded_stride "
                         f"recorded: run the whole module in one process.  Ran: { {c: sorted(v) for c, v in RAN.items()} }")
    print(f"padded stride: all {len(wp.FAMILIES)} families ran on a padded handle")


def test_zy_every_kind_and_form_ran_on_a_padded_handle():
    want = {(kind, form) for kind in lf.KINDS for form in lf.FORMS}
    assert FORMS_RAN == want and len(want) == 60, f"(kind, form) that did not run on a padded handle IN THIS PROCESS: {sorted(want - FORMS_RAN)}"
    print(f"padded stride: all {len(want)} (kind, form) pairs ran on a padded handle")
