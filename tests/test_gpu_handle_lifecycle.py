"""What a handle holds and how it lets go of it: the grow-only scratch of the MPC rollout and of the getters, and handles that are
created, stepped and destroyed next to each other.  Every assertion is bit equality between two runs of the same library on the
same seeded inputs, so there is no tolerance.

Shapes: 70 robots (the second wavefront is partly filled), 8 cables, FK + TD, 30 world steps; four kinds of handle: plain fp32,
the general controller path (velocityEpsilon 0.004: the hold branch is live), plain fp64, fp64 with per-robot command arrival.
"""
import os
import sys

import numpy as np
import pytest

from parity import perturbed_poses

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
from variant_digest import Collector  # noqa: E402  (what the bit-level digests snapshot of a handle)

pytestmark = pytest.mark.gpu

B, N, H = 70, 8, 4
KINDS = {
    "fp32": dict(),
    "general": dict(velocityEpsilon=0.004),
    "fp64": dict(precision=64),
    "fp64_per_robot": dict(precision=64, perRobotCommands=True),
}


def make(pkg, kind):
    return pkg.Engine(pkg.Config(model=pkg.eight_cable_model(), batch=B, stages=3, **KINDS[kind]), 0)


def joy(rng, eps=0.004):
    """A Joy batch whose axes lie on both sides of velocityEpsilon (general path: cables in the hold branch and out of it)."""
    cmd = rng.uniform(-0.03, 0.03, (B, N)).astype(np.float32)
    low = rng.random((B, N)) < 0.3
    cmd[low] = (rng.uniform(-1.0, 1.0, int(low.sum())) * eps).astype(np.float32)
    return cmd


def thirty_steps(eng, seed, between=None):
    """Spawn poses, then three rounds of ten world steps: Position mode at target 0, then two Joy batches.  `between(round)` runs
    after every half round (the other handles' turns)."""
    rng = np.random.default_rng(seed)
    eng.set_platform_state(pose7=perturbed_poses(eng.config.model, B, rng, 0.03, 0.05).astype(np.float32))
    for r in range(3):
        if r:
            eng.set_velocity_command(joy(rng))
        for _ in range(2):
            eng.update(5)
            if between:
                between(r)


def snapshot(eng):
    c = Collector()
    c.snap(eng, f64=eng.config.precision == 64)
    c.add(*eng.observables())
    return [(a.dtype, a.shape, a.tobytes()) for a in c.arrays]


@pytest.mark.parametrize("kind", list(KINDS))
def test_rollout_scratch_grows_and_is_reused(pkg, kind):
    """Rollouts of 2, then 6, then 2 samples on one handle (the scratch is allocated, replaced by a longer one, then reused with room
    to spare) cost, bit for bit, what each costs on a fresh handle in the same state; the handle's own state is not touched."""
    rng = np.random.default_rng(2024)
    rollouts = [(rng.uniform(-0.03, 0.03, (B, H, 1, N)) + rng.normal(0.0, 0.01, (B, H, s, N))).astype(np.float32) for s in (2, 6, 2)]
    eng = make(pkg, kind)
    thirty_steps(eng, 7)
    ref = eng.raw_state()[0][:, :3] + np.float32([0.0, 0.0, 0.005])
    before = snapshot(eng)
    costs = [eng.rollout_velocity(cmds, ref) for cmds in rollouts]
    assert snapshot(eng) == before, "a rollout changed the handle's state or observables"
    eng.close()
    for j, cmds in enumerate(rollouts):
        fresh = make(pkg, kind)
        thirty_steps(fresh, 7)
        assert snapshot(fresh) == before
        want = fresh.rollout_velocity(cmds, ref)
        fresh.close()
        assert costs[j].shape == (B, cmds.shape[2]) and np.isfinite(want).all()
        assert costs[j].tobytes() == want.tobytes(), f"rollout {j} ({cmds.shape[2]} samples) differs from the same rollout on a fresh handle"


def test_handles_come_and_go_independently(pkg):
    """A stepped alone, then next to a general-path handle (destroyed after 10 steps) and an fp64 handle (destroyed after 20), then
    again after cdpr_reset: the same bits at 30 steps every time."""
    a = make(pkg, "fp32")
    thirty_steps(a, 11)
    alone = snapshot(a)
    a.close()

    a, others = make(pkg, "fp32"), {"general": make(pkg, "general"), "fp64": make(pkg, "fp64")}
    leaves_after = {"general": 0, "fp64": 1}  # the round after which the handle is destroyed
    rngs = {k: np.random.default_rng(100 + i) for i, k in enumerate(others)}
    for k, e in others.items():
        e.set_platform_state(pose7=perturbed_poses(e.config.model, B, rngs[k], 0.03, 0.05).astype(np.float32))
    half = [0]

    def turn(r):
        half[0] += 1
        for k in list(others):
            if half[0] % 2 == 1:
                others[k].set_velocity_command(joy(rngs[k]))
            others[k].update(5)
            if half[0] % 2 == 0 and leaves_after[k] == r:
                assert np.isfinite(others[k].joint_states()[2]).all()
                others.pop(k).close()

    thirty_steps(a, 11, between=turn)
    assert not others and a.step_count == 30
    assert snapshot(a) == alone, "stepping next to handles that were destroyed on the way changed the results"
    a.reset()
    thirty_steps(a, 11)
    assert snapshot(a) == alone, "cdpr_reset + the same 30 steps gives other bits"
    a.close()
