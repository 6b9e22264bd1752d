"""The host forms that stage their arguments - cdpr_reset_robots, cdpr_copy_robots, cdpr_set_velocity_command - called back to back:
each call's arrays go through a pair of pinned blocks that take turns (StagePair, csrc/cdpr_engine_internal.hpp), the caller's arrays
are the caller's again the moment the call returns, and nothing waits for the stream.  Five calls in a row pass every block at least
twice, so a block is refilled while the copy of two calls back may still be queued.

After a 12-step history: five reset_robots with different masks and poses, five copy_robots with different valid maps, five velocity
batches each followed by update(1) - the arrays overwritten the moment each call returns (NaN; the masks inverted, the maps -1), no
synchronize in between.  Every getter must equal, to the bit, a second engine that gets the same calls from untouched arrays with a
synchronize() after each.  B = 130 on one handle per record layout.
"""
import numpy as np
import pytest

import copy_robots as cr
import robot_histories as ri
from parity import perturbed_poses
from per_robot_kinds import LAYOUTS, clean_env, config_of, state_of  # noqa: F401  (clean_env: autouse here too)

pytestmark = pytest.mark.gpu

B = ri.B
CALLS = 5


def script(model):
    """the arguments of the fifteen calls"""
    rng = np.random.default_rng(1401)
    resets = []
    for j in range(CALLS):
        mask = (np.arange(B) % CALLS == j).astype(np.uint8)
        mask[[0, 63, 64, B - 1][j % 4]] = 1
        resets.append((mask, perturbed_poses(model, B, rng, 0.02, 0.05).astype(np.float32), rng.uniform(-0.01, 0.01, (B, 6)).astype(np.float32)))
    maps = []
    for j in range(CALLS):  # destinations: r = j mod 5; sources: 66 + j further on, never = j mod 5 (66 + j = 1 + 2 j mod 5 is never 0)
        source = np.full(B, -1, dtype=np.int32)
        for d in range(j, B, CALLS):
            s = (d + 66 + j) % B
            while s % CALLS == j:
                s = (s + 1) % B
            source[d] = s
        assert cr.validate_map(source) is None and cr.destinations_of(source).sum() == B // CALLS
        maps.append(source)
    joys = [rng.uniform(-0.03, 0.03, (B, model.n_cables)).astype(np.float32) for _ in range(CALLS)]
    return resets, maps, joys


def play(eng, model, careful):
    """careful: untouched arrays and a synchronize() after each call; else the arrays are ruined as each call returns and nothing waits"""
    resets, maps, joys = script(model)

    def after(*arrays):
        if careful:
            eng.synchronize()
            return
        for a in arrays:
            if a.dtype == np.uint8:
                a[:] = 1 - a
            else:
                a[:] = -1 if a.dtype == np.int32 else np.nan

    for mask, pose, twist in resets:
        eng.reset_robots(mask, pose, twist)
        after(mask, pose, twist)
    for source in maps:
        eng.copy_robots(source)
        after(source)
    for joy in joys:
        assert eng.set_velocity_command(joy) == 0
        after(joy)
        eng.update(1)
        after()


@pytest.mark.parametrize("kind", LAYOUTS)
def test_staged_calls_back_to_back(pkg, monkeypatch, kind):
    cfg = config_of(pkg, kind, monkeypatch)
    h = ri.history_inputs(cfg.model, 1400)
    engs = [pkg.Engine(cfg, 0) for _ in range(2)]
    for e in engs:
        e.set_platform_state_f64(pose7=h["pose"].astype(np.float64)) if cfg.precision == 64 else e.set_platform_state(pose7=h["pose"])
    ri.play_history(engs, h, 12)
    fast, careful = engs
    play(fast, cfg.model, careful=False)
    play(careful, cfg.model, careful=True)
    assert fast.step_count == careful.step_count == 12 + CALLS
    for i, (x, y) in enumerate(zip(state_of(fast, cfg) + (fast.episode_start(),), state_of(careful, cfg) + (careful.episode_start(),))):
        assert np.isfinite(y).all(), (kind, i)
        assert np.array_equal(x, y), f"{kind}, getter {i}: back-to-back staged calls differ from the same calls with a synchronize() after each"
    assert (careful.episode_start() == 12).all()  # (the five masks reach every robot once, at world step 12; a copy moves a 12 onto a 12)
    for e in engs:
        e.close()
