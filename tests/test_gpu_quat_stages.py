"""The pair-packed quaternion stages of the role-split kernels (quat_to_rot_pk, quat_apply_rotvec_pk, ik_rows_pk: csrc/cdpr_step_kernel.hpp)
and the rotation matrix the steady kernel's estimator wave hands to its controller wave (CDPR_STEADY_SHARED_ROT, csrc/cdpr_onestep_kernel.hpp).

The pair forms are meant to be the scalar stages' IEEE operations on the same operands, so every comparison between kernels here is BIT
EQUALITY.  The one-wave cdpr_step_kernel keeps the scalar stages: it is the reference the packed lanes, swizzles and signs are held against.

Per cell (n = 8, 7, 6; Velocity and Position mode; 65 robots = two workgroups with a ragged tail of one, and 64), 25 world steps with a new
command every 10, so that the launches cross from the generic role-split kernel to the steady one where the derivative window fills:
  (a) the default handle and a handle kept on the generic role-split kernel (CDPR_SPLIT_STEADY=0) agree on all five read-outs after every step;
  (b) the default handle and the one-wave cdpr_step_kernel mapping (CDPR_ONESTEP=1) do;
  (c) the default handle stays within tests/parity.py's TOL of the fp64 oracle after every step, every robot.
Start poses (R = I would hide a swapped or mis-signed matrix entry: every entry off the diagonal is then zero):
  row 0        the spawn pose at rest.  cdpr_set_platform_state seeds the FK estimate with the pose, so on world step 0 EVERY robot's first
               Newton update has |theta|^2 < 1e-8 (the series branch of quat_apply_rotvec); this one stays there longest;
  row 1        the spawn pose turning at 200 rad/s about (1, 1, 1): world step 0 turns it by 0.2 rad while its estimate stays, so the first
               Newton update of step 1 has |theta| ~ 0.2 (the API has no setter for the estimate alone).  Its rate is set to zero after step 0
               on every simulator;
  rows 2 ..    poses from box W of tests/workspace_poses.py, ill-conditioned draws rejected (below);
  last 8 rows  the spawn position turned by +-0.3 rad about x, y, z and (1, 1, 1) (the ragged tail of 65 is the last of them).

The box poses and the conditioning of the reduced models.  The n = 7 and n = 6 models are the first cables of twelve_cable_model, and across
box W (yaw up to pi) some of their poses are close to singular: the normal matrix J^T J of the tension distribution has a condition number
(fp64, from the oracle's structure matrix) of up to 6e6 at n = 7 and 1.6e8 at n = 6 among 55 draws, against at most 1.3e4 for the eight-cable
model.  A float32 solve loses kappa * 2^-24 of its solution there whatever kernel runs it: with such a draw in the batch (kappa = 6e6, n = 7)
the efforts were 5.1e-2 N from the oracle at step 1, with bits EQUAL to the scalar one-wave kernel's.  TOL was stated for the four- and
eight-cable models (tests/parity.py; the suite's other n = 6, 7 comparisons start within 0.05 rad of the spawn pose), so start_state
(tests/quat_stage_poses.py, shared with tests/test_gpu_model_constants.py) draws from
the box until it has enough poses with kappa <= KAPPA_MAX = 1.5e4, just above the eight-cable model's largest; the bound is a property of the
models, not of the engine.  No draw of the n = 8 cells is rejected; the named poses are fixed and are not filtered (kappa <= 1e4).

Build switches: libraries built with -DCDPR_QUAT_PK=0 and with -DCDPR_STEADY_SHARED_ROT=0 (scripts/build_variants.sh quat_pk0 shared_rot0; loaded
through CDPR_LIB in a child process each), and one without the estimator wave's pin of the tension distribution's factor
(-DCDPR_EST_PIN_FACTOR=0, pin0), leave the same bits in the final state of the 65-robot cells as the shipped build.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import workspace_poses as wp
from parity import NAMES, ROUTING_OVERRIDES, TOL, assert_within, observed, worst_errors
from quat_stage_poses import KAPPA_MAX, TURNING, start_state

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cdpr-simulation_amd")
STEPS, REFRESH = 25, 10
SPLIT, ONE_WAVE = "cdpr_split_kernel<%d, false>", "cdpr_step_kernel<"
OVERRIDES = ROUTING_OVERRIDES + ("CDPR_SPLIT_STEADY", "CDPR_NO_GRAPH", "CDPR_LIB")
CELLS = [(n, mode, batch) for n in (8, 7, 6) for mode in ("velocity", "position") for batch in (65, 64)]
SWITCH_LIBS = {"CDPR_QUAT_PK=0": "quat_pk0", "CDPR_STEADY_SHARED_ROT=0": "shared_rot0", "CDPR_EST_PIN_FACTOR=0": "pin0"}


def commands(batch, n, seed):
    """(velocity commands j -> float32[B, n] in +-0.03 m/s, position offsets j -> float32[B, n] in +-0.004 m): workspace_poses' script ranges."""
    rng = np.random.default_rng(seed)
    v, off = rng.uniform(-0.03, 0.03, (3, batch, n)).astype(np.float32), rng.uniform(-0.004, 0.004, (3, batch, n)).astype(np.float32)
    return (lambda j: v[j]), (lambda j: off[j])


def run_cell(pkg, n, mode, batch, sims, after_step):
    """The cell's 25 steps on `sims` (the first is the one whose joint positions the position targets are taken from); after_step(k) sees
    every simulator after world step k."""
    vel, off = commands(batch, n, 77 * n + batch)
    for k in range(STEPS):
        if k % REFRESH == 0:
            target = vel(k // REFRESH) if mode == "velocity" else (sims[0].joint_states()[0] + off(k // REFRESH)).astype(np.float32)
            for s in sims:
                (s.set_velocity_command if mode == "velocity" else s.set_position_command)(target)
        for s in sims:
            s.update(1)
        if k == 0:  # the turning robot has made its 0.2 rad: every simulator goes on from the default handle's rates with that one at zero
            twist = sims[0].raw_state()[1].copy()
            twist[TURNING] = 0.0
            for s in sims:
                s.set_platform_state(twist6=twist)
        after_step(k)


def make_engine(pkg, monkeypatch, cfg, pose, twist, **env):
    for k in OVERRIDES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = pkg.Engine(cfg, 0)  # (the overrides are read when the handle is created)
    for k in env:
        monkeypatch.delenv(k, raising=False)
    eng.set_platform_state(pose7=pose, twist6=twist)
    return eng


@pytest.mark.parametrize("n,mode,batch", CELLS, ids=[f"n{n} {mode} b{b}" for n, mode, b in CELLS])
def test_pair_forms_against_generic_one_wave_and_oracle(pkg, oracle, monkeypatch, n, mode, batch):
    model = wp.cell_model(pkg, n)
    cfg = pkg.Config(model=model, batch=batch, stages=3)
    pose, twist, kappa = start_state(pkg, n, batch)
    assert kappa <= KAPPA_MAX, kappa
    default = make_engine(pkg, monkeypatch, cfg, pose, twist)
    generic = make_engine(pkg, monkeypatch, cfg, pose, twist, CDPR_SPLIT_STEADY="0")
    one_wave = make_engine(pkg, monkeypatch, cfg, pose, twist, CDPR_ONESTEP="1")
    ora = oracle.OracleSim(cfg.to_struct(), oracle.DERIV_EXACT)
    ora.set_platform_state(pose7=pose.astype(np.float64), twist6=twist.astype(np.float64))
    variants, worst_all, first_theta = [], dict.fromkeys(NAMES, 0.0), []
    def after_step(k):
        got = default.observables()
        for other, what in ((generic, "(a) the generic role-split kernel"), (one_wave, "(b) the one-wave kernel")):
            diff = [name for name, x, y in zip(("q", "qd", "eff", "pose", "twist"), got, other.observables()) if not np.array_equal(x, y)]
            assert not diff, f"step {k}: {diff} differ between the default handle and {what}"
        assert default.kernel_name == generic.kernel_name == SPLIT % n and one_wave.kernel_name.startswith(ONE_WAVE), (default.kernel_name, one_wave.kernel_name)
        assert generic.last_variant == 0
        variants.append(default.last_variant)
        if k == 0:  # how far the turning robot's pose is from its estimate before step 1
            rel = Rotation.from_quat(default.raw_state()[0][TURNING, 3:].astype(np.float64)) * Rotation.from_quat(default.fk_state()[0][TURNING, 3:].astype(np.float64)).inv()
            first_theta.append(float(np.linalg.norm(rel.as_rotvec())))
        worst = worst_errors(observed(default), observed(ora), f"step {k}")
        for name in NAMES:
            worst_all[name] = max(worst_all[name], worst[name][0])
        if any(worst[name][0] > TOL[name] for name in NAMES):
            print(f"step {k}: " + "  ".join(f"{name} {v[0]:.2e} (robot {v[1]})" for name, v in worst.items()))
        assert_within(worst, TOL, f"(c) step {k}")

    run_cell(pkg, n, mode, batch, [default, generic, one_wave, ora], after_step)
    print(f"n{n} {mode} b{batch}: worst error against the oracle over {STEPS} steps: " + "  ".join(f"{k} {v:.2e}" for k, v in worst_all.items())
          + f"; largest kappa {kappa:.2e}; turning robot before step 1: |theta| = {first_theta[0]:.3f} rad")
    assert 0.15 < first_theta[0] < 0.25, first_theta
    nbuf = getattr(pkg.Config(), mode + "Controller").dBufferLength
    assert variants == [0] * (nbuf + 1) + [1] * (STEPS - nbuf - 1), variants  # the launches crossed into the steady kernel where the window filled
    # the rows no read-out of the published step shows: true state, estimate, residual and iteration count, tensions and flag
    for other in (generic, one_wave):
        for x, y in zip(list(default.raw_state()) + list(default.fk_state()) + list(default.td_state()), list(other.raw_state()) + list(other.fk_state()) + list(other.td_state())):
            assert np.array_equal(x, y)
    assert set(default.fk_state()[2].tolist()) == {4}
    for s in (default, generic, one_wave):
        s.close()


# ---- the build switches, each alone: a child process per library ----------------------------------------------------------------------
def final_digests():
    """(child process) {cell: sha256 of the final state} of the 65-robot cells on the library CDPR_LIB selects."""
    import cdpr_simulation_amd as pkg

    out = {}
    for n, mode, batch in CELLS:
        if batch != 65:
            continue
        model = wp.cell_model(pkg, n)
        eng = pkg.Engine(pkg.Config(model=model, batch=batch, stages=3), 0)
        pose, twist, _ = start_state(pkg, n, batch)
        eng.set_platform_state(pose7=pose, twist6=twist)
        variants = []
        run_cell(pkg, n, mode, batch, [eng], lambda k: variants.append(eng.last_variant))
        final = list(eng.raw_state()) + list(eng.fk_state()) + list(eng.td_state()) + list(eng.observables())
        out[f"n{n} {mode}"] = {"digest": hashlib.sha256(b"".join(np.ascontiguousarray(x).tobytes() for x in final)).hexdigest(), "steady": int(sum(variants))}
        eng.close()
    print(json.dumps(out))


_digests = {}


def digests_of(lib):
    if lib not in _digests:
        env = dict(os.environ, CDPR_LIB=lib)
        for k in OVERRIDES[:-1]:
            env.pop(k, None)
        env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, f"{lib}: the run failed\n{r.stdout[-1000:]}\n{r.stderr[-3000:]}"
        _digests[lib] = json.loads(r.stdout.strip().splitlines()[-1])
    return _digests[lib]


@pytest.mark.parametrize("switch", list(SWITCH_LIBS), ids=list(SWITCH_LIBS))
def test_a_build_with_one_switch_off_leaves_the_same_bits(switch):
    name = SWITCH_LIBS[switch]
    lib = f"libcdpr_hip_var_{name}.so"
    if not os.path.exists(os.path.join(PKG, lib)):  # shipped with the snapshot where it was built beforehand; else build it here
        r = subprocess.run(["bash", os.path.join(ROOT, "scripts", "build_variants.sh"), name], capture_output=True, text=True, timeout=3000)
        assert r.returncode == 0, f"building variant {name} failed:\n{r.stderr[-3000:]}"
    ref, var = digests_of("libcdpr_hip.so"), digests_of(lib)
    assert len(ref) == 6 and all(v["steady"] > 0 for v in ref.values()), ref
    moved = sorted(k for k in ref if var.get(k) != ref[k])
    assert not moved, f"{switch} changes the final state of: {moved}"


if __name__ == "__main__":
    final_digests()
