"""The conditions tests/test_gpu_padded_stride.py relies on, established without a GPU on the fp64 oracle and on the inputs alone, with
the seeds, kinds and batches of tests/padded_stride.py that the GPU module uses.

  masks and maps   the reset masks and copy maps touch every wavefront of the batch and robot B - 1, at B = 130, at every B of the batch
                   edges and at 131 072; every map is one cdpr_copy_robots accepts.
  home margin      a pad column holds the home state (home pose, nothing published).  Under every history the GPU module plays, every
                   robot of the oracle is away from that state by more than the comparison tolerance (TOL of tests/parity.py, the wider
                   of the two tables) in pose or in effort: a kernel that read a pad column for some robot could not stay within
                   tolerance of the oracle.  Asserted per cell and per kind; the margin is printed (-s).
  live counts      the done rules of sections 3 and 4 keep each enabled bit's count strictly between 0 and B on the oracle (B = 1 has
                   no `between`: there the count is 0 or 1).
  stride_of        on a hand-made table of image sizes.
"""
import numpy as np
import pytest

import copy_robots as cr
import done_handles as gd
import done_rules as dr
import padded_stride as ps
import parity
import per_robot_kinds as prk
import readout_layout
import robot_histories as ri
import workspace_poses as wp
from parity import TOL

clean_env = prk.clean_env  # (autouse: config_of sets a kind's routing switches, which plan nothing here but must not leak)

MARGIN = 1.0  # units of TOL: "more than the comparison tolerances"


# ---- masks and maps ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", ps.EDGE_BATCHES)
def test_edge_masks_and_map_touch_every_wave_and_the_last_robot(pkg, batch):
    masks = ps.edge_masks(batch)
    assert masks[0][0] and masks[0].sum() == 1 and masks[1][batch - 1] and masks[1].sum() == 1
    assert np.array_equal(np.flatnonzero(masks[2]), np.arange(0, batch, 3))
    assert ps.waves_touched(np.maximum.reduce(masks), batch)[1] and np.maximum.reduce(masks)[batch - 1]  # (B = 65: the last wave is robot 64 alone)
    source = ps.edge_map(batch)
    assert cr.validate_map(source) is None and source.dtype == np.int32
    dest = cr.destinations_of(source)
    if batch == 1:
        assert not dest.any()
        return
    used = dest.copy()
    used[source[dest]] = True
    assert ps.waves_touched(used, batch)[1] and used[batch - 1] and source[0] == batch - 1
    if batch > 64:  # sources across wave boundaries: robot B - 1 sits in the last wave, robot 0 in the first
        assert source[0] // 64 == (batch - 1) // 64 > 0
    if batch >= 128:
        assert (source[dest] // 64 != np.flatnonzero(dest) // 64).mean() > 0.5
    # the twin from birth's inputs: a destination's rows, its reset flags included, are its source's
    x, born, again = ps.chain_inputs(gd.limited(pkg.cube_model()), batch, 411)
    assert np.array_equal(again, source)
    for k, v in x.items():
        assert np.array_equal(born[k][dest], v[source[dest]]) and np.array_equal(born[k][~dest], v[~dest]), k


def test_masks_and_maps_at_130_and_at_131072_robots(pkg):
    m = ri.reset_mask()
    assert ps.waves_touched(m, ps.B)[1] and m[ps.B - 1] and m[0] and not m.all()
    for source in (cr.copy_map(), ps.ops_inputs(pkg.cube_model(), "resample")[5]):
        dest = cr.destinations_of(source)
        used = dest.copy()
        used[source[dest]] = True  # (the resampler's dead robots take survivors of their own group of 65: the last wave holds sources only)
        assert cr.validate_map(source) is None and ps.waves_touched(used, ps.B)[1] and 20 < dest.sum() < ps.B
    assert cr.destinations_of(cr.copy_map())[ps.B - 1]
    N = ps.FULL_B
    m = ps.spread_mask(N)
    assert m[[0, N // 2 - 1, N // 2, N - 1]].all() and ps.waves_touched(m, N)[1] and 1000 < m.sum() < N // 50
    source = ps.other_half_map(N)
    dest = cr.destinations_of(source)
    assert cr.validate_map(source) is None and not (dest & m.astype(bool))[2:].any() and source[1] == N - 2 and 1000 < dest.sum()
    assert ((np.flatnonzero(dest) < N // 2) != (source[dest] < N // 2)).all(), "every source lies in the other half"
    for sl in (slice(0, 128), slice(N // 2 - 64, N // 2 + 64), slice(N - 128, N)):  # every oracle slice sees a reset robot and a destination
        assert m[sl].any() and dest[sl].any(), sl


# ---- home margin ---------------------------------------------------------------------------------------------------------------
def margin_of(sim, cfg, where):
    d = ps.home_margin(parity.observed(sim), cfg.model.home_pose(), TOL)
    print(f"padded stride, home margin, {where}: {d:.1f} x TOL")
    return d


@pytest.mark.parametrize("cell", list(wp.CELLS))
def test_cells_leave_the_home_state(pkg, oracle, cell):
    cfg, states = ps.cell_states_on_the_oracle(pkg, oracle, cell)
    worst = min(ps.home_margin(s, cfg.model.home_pose(), TOL) for s in states)
    print(f"padded stride, home margin, cell {cell}: {worst:.1f} x TOL over the {len(states)} segments")
    assert worst > MARGIN, cell


@pytest.mark.parametrize("kind", ps.OPS_KINDS)
def test_op_histories_leave_the_home_state(pkg, oracle, monkeypatch, kind):
    """sections 2 and 3a: the 37-step history, then the reset of the mask and ri.play_after"""
    cfg = ps.ops_config(pkg, kind, monkeypatch)
    h, a, _, _, mask, _, _ = ps.ops_inputs(cfg.model, "reset")
    ora = parity.oracle_at(oracle, cfg, h["pose"])
    ri.play_history([ora], h)
    lim = ora.limit_state() != 0
    assert 0 < lim.sum() < ps.B, f"{kind}: the travel bits do not tell the robots apart ({int(lim.sum())})"
    worst = [margin_of(ora, cfg, f"{kind}, the end of the history")]
    ri.oracle_reset(ora, mask, a["pose"])
    ri.play_after([ora], a, lambda label: worst.append(margin_of(ora, cfg, f"{kind}, {label}")))
    assert min(worst) > MARGIN, (kind, worst)
    ora.close()


@pytest.mark.parametrize("kind", ps.VIEW_KINDS)
def test_view_histories_leave_the_home_state_and_the_rule_is_live(pkg, oracle, monkeypatch, kind):
    """section 3b: test_after_real_steps' history on the oracle; every enabled bit of the rule fires for some robots and not for all"""
    cfg = ps.view_config(pkg, kind, monkeypatch)
    h = ri.history_inputs(cfg.model, ps.VIEW_SEED)
    ora = parity.oracle_at(oracle, cfg, h["pose"])
    gd.drive([ora], cfg, h, ps.VIEW_STEPS)
    assert margin_of(ora, cfg, kind) > MARGIN, kind
    g = ps.oracle_getters(ora, cfg)
    rule, k = ps.view_rule(pkg, cfg, g["fk_residual"])
    mask, reason, counts = dr.done_reference(rule, **g)
    print(f"padded stride, done on the oracle, {kind}: counts {counts[:10].tolist()}")
    ps.assert_counts_are_live(counts, rule, ps.B, kind)
    assert rule.enable & dr.TRAVEL and bool(rule.enable & dr.FK_RESIDUAL) == bool(cfg.stages & 1) and bool(rule.enable & dr.INFEASIBLE) == bool(cfg.stages & 2)
    ora.close()


@pytest.mark.parametrize("batch", ps.EDGE_BATCHES)
@pytest.mark.parametrize("kind", prk.LAYOUTS)
def test_edge_chains_leave_the_home_state_and_the_rule_is_live(pkg, oracle, monkeypatch, kind, batch):
    """section 4 on the oracle, with the engines' own inputs (before the copy every robot has its own history)"""
    cfg = ps.ops_config(pkg, kind, monkeypatch, batch)
    x, _, _ = ps.chain_inputs(cfg.model, batch, 411)
    ora = parity.oracle_at(oracle, cfg, x["pose"])
    ps.chain_history([ora], x)
    where = f"{kind}, B = {batch}"
    worst = [margin_of(ora, cfg, f"{where}, the history")]
    start = np.zeros(batch, np.uint32)
    for key, steps in ps.CHAIN_STEPS:
        ps.chain_reset_on_the_oracle(ora, x, key)
        start[x[key].astype(bool)] = ora.step_count
        ora.update(steps)
        worst.append(margin_of(ora, cfg, f"{where}, {steps} steps after the reset {key}"))
    assert min(worst) > MARGIN, (where, worst)
    rule = ps.edge_rule(pkg, ora.step_count)
    counts = dr.done_reference(rule, **ps.oracle_getters(ora, cfg, start))[2]
    print(f"padded stride, done on the oracle, {where}: counts {counts[:10].tolist()}")
    ps.assert_counts_are_live(counts, rule, batch, where)
    ora.close()


def test_the_full_size_inputs_leave_the_home_state(pkg):
    """section 5: start and fresh poses of every robot, before any step (15 steps move a robot by less than its distance from home)"""
    N = ps.FULL_B
    rng = np.random.default_rng(1241)
    model = gd.limited(pkg.cube_model())
    for name in ("start", "fresh"):
        pose = parity.perturbed_poses(model, N, rng, 0.03, 0.05).astype(np.float32)
        if name == "start":
            rng.uniform(-0.03, 0.03, (N, 4)), rng.uniform(-0.003, 0.003, (N, 4))  # (the draws the GPU test makes in between)
        d = np.abs(pose.astype(np.float64) - np.asarray(model.home_pose())).max(axis=1)
        print(f"padded stride, home margin, 131 072 robots, {name} poses: {d.min() / TOL['pose']:.1f} x TOL")
        assert d.min() > 10 * TOL["pose"], name  # 15 steps at <= 0.03 m/s move a cable by <= 0.45 mm; the margin is on the pose the robot starts from


# ---- stride_of -----------------------------------------------------------------------------------------------------------------
class Image:
    def __init__(self, nbytes):
        self.nbytes = nbytes

    def observable_image_bytes(self):
        return self.nbytes


def test_stride_of_on_a_hand_made_table():
    from types import SimpleNamespace as Cfg

    # fp32: n_obs float4 slots of 16 B per column; n = 4: 4 + 3 = 7 slots, n = 8: 4 + 6 = 10, n = 7: 10, n = 12: 13, n = 9: 13
    table = [(4, 130, 7 * 16 * 192, 192), (4, 130, 7 * 16 * 256, 256), (8, 130, 10 * 16 * 320, 320), (7, 130, 10 * 16 * 192, 192), (12, 130, 13 * 16 * 256, 256),
             (9, 1, 13 * 16 * 128, 128), (4, 131072, 7 * 16 * 131200, 131200), (4, 131072, 7 * 16 * 131072, 131072), (8, 257, 10 * 16 * 384, 384)]
    for n, batch, image, stride in table:
        assert ps.row_bytes(n) == 16 * readout_layout.image_rows(n, False)
        assert ps.stride_of(Image(image), Cfg(n_cables=n, batch=batch, precision=32)) == stride, (n, batch, image)
    # precision = 64: rows of doubles, 16 + 3 n of them; the row size comes from the unpadded twin's image
    for n, batch, pad in ((8, 130, 0), (8, 130, 64), (8, 130, 128), (12, 63, 64), (8, 1, 64), (8, 257, 64)):
        rows, su = readout_layout.image_rows(n, True), ps.round_up(batch)
        twin, eng = Image(rows * 8 * su), Image(rows * 8 * (su + pad))
        cfg = Cfg(n_cables=n, batch=batch, precision=64)
        assert ps.row_bytes(n, True, twin.nbytes, batch) == rows * 8
        assert ps.stride_of(eng, cfg, twin) == su + pad and ps.stride_of(twin, cfg, twin) == su, (n, batch, pad)
    assert ps.round_up(1) == 64 and ps.round_up(64) == 64 and ps.round_up(65) == 128 and ps.round_up(130) == 192 and ps.round_up(257) == 320
    with pytest.raises(AssertionError):
        ps.stride_of(Image(7 * 16 * 192 + 8), Cfg(n_cables=4, batch=130, precision=32))
    with pytest.raises(AssertionError):
        ps.stride_of(Image(1000), Cfg(n_cables=8, batch=130, precision=64))  # (no twin)


def test_assert_same_and_the_pad_check_can_fail():
    a = dict(x=np.arange(6.0).reshape(3, 2), n=np.asarray(5))
    ps.assert_same(a, dict(x=a["x"].copy(), n=np.asarray(5)), "equal")
    b = dict(x=a["x"].copy(), n=np.asarray(5))
    b["x"][2, 1] = np.nextafter(b["x"][2, 1], 9.0)
    with pytest.raises(AssertionError, match=r"x differs to the bit.*\[2\]"):
        ps.assert_same(a, b, "one bit")
    ps.assert_same(a, b, "the other rows", rows=np.array([True, True, False]))
    ps.assert_same(a, b, "row 0 against row 0", rows=np.array([0]), rows_want=np.array([0]))
    with pytest.raises(AssertionError):
        ps.assert_same(a, dict(x=a["x"].astype(np.float32), n=np.asarray(5)), "dtype")
    with pytest.raises(AssertionError):
        ps.assert_same(a, dict(x=a["x"], n=np.asarray(6)), "scalar")
    from types import SimpleNamespace as Cfg

    cfg = Cfg(n_cables=8, batch=130, precision=32)
    ps.assert_pad_took(Image(10 * 16 * 192), Image(10 * 16 * 256), cfg, 64)
    with pytest.raises(AssertionError, match="did not take"):
        ps.assert_pad_took(Image(10 * 16 * 192), Image(10 * 16 * 192), cfg, 64)
    with pytest.raises(AssertionError, match="did not take"):
        ps.assert_pad_took(Image(10 * 16 * 192), Image(10 * 16 * 320), cfg, 64)
    with pytest.raises(AssertionError, match="strictly|do not tell|does not tell"):
        ps.assert_counts_are_live(np.array([130, 0, 0, 0, 0, 0, 0, 0, 130] + [0] * 7), Cfg(enable=dr.TRAVEL), 130, "all done")
