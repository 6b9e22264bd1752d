"""What deciding on the device who is done costs next to the step it sits behind (cdpr_evaluate_done_device, cdpr_reset_done_device)
and next to the host loop it replaces: per_robot_commands handles at 65 536 x 8 (FK + TD, register-resident) and 4 096 x 4.

The rule: a workspace box of +-48 mm around the home position that leaves some robots outside (how many is printed; the respawn poses
are the start poses), tilt, speed and rate thresholds nobody reaches, the FK residual and the infeasible flag where the handle has the
stages, a timeout nobody reaches.  By HIP events on the engine's stream, LOOP calls per sample, ALTERNATIONS samples of each after a
warm-up, medians:
  A  evaluate_done_device(mask, reason, counts)     A'  evaluate_done_device(mask): no counts, so no zeroing in front of the kernel
  B  reset_done_device(poses, counts)     B'  reset_done_device(poses)     C  update(1)
  D  LOOP x { evaluate_done_device; update(1) } - C: the verdict behind a step, as a loop would queue it
Beside them, by the wall clock, the host loop there was before: raw_state, fk_state, td_state, limit_state (each waits for the
stream), the predicate in numpy, reset_robots with the mask.  Usage: done_cost.py [out.txt]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bench  # noqa: E402
import cdpr_simulation_amd as pkg  # noqa: E402
from cdpr_simulation_amd import _abi  # noqa: E402

LOOP, ALTERNATIONS = 10, 300
SHAPES = ((65536, 8, 3), (4096, 4, 0))  # batch, cables, stages


def timed(eng, body):
    eng.profile_begin()
    for _ in range(LOOP):
        body()
    return eng.profile_end()[0] * 1e3 / LOOP  # us per iteration


def host_predicate(rule, pose, twist, residual, infeasible, limits):
    lo, hi = np.asarray(rule.pos_lo, np.float32), np.asarray(rule.pos_hi, np.float32)
    q = pose[:, 3:]
    done = ~np.isfinite(pose).all(axis=1) | ~np.isfinite(twist).all(axis=1) | ((pose[:, :3] < lo) | (pose[:, :3] > hi)).any(axis=1)
    done |= 1.0 - 2.0 * (q[:, 0] ** 2 + q[:, 1] ** 2) / (q * q).sum(axis=1) < rule.min_up
    done |= ((twist[:, :3] ** 2).sum(axis=1) > rule.max_speed ** 2) | ((twist[:, 3:] ** 2).sum(axis=1) > rule.max_rate ** 2)
    if residual is not None:
        done |= (residual > rule.max_fk_residual) | (infeasible != 0)
    return (done | (limits != 0)).astype(np.uint8)


def main():
    lines = []
    for B, N, stages in SHAPES:
        model, pose, command, _ = bench.make_workload(pkg, B, N, 1235, 10)
        eng = pkg.Engine(pkg.Config(model=model, batch=B, stages=stages, perRobotCommands=True), 0)
        eng.set_platform_state(pose7=pose)
        eng.set_velocity_command(command(0))
        eng.update(200)
        eng.synchronize()
        home = np.asarray(model.home_pose())[:3]
        enable = _abi.DONE_NONFINITE | _abi.DONE_WORKSPACE | _abi.DONE_TILT | _abi.DONE_SPEED | _abi.DONE_RATE | _abi.DONE_TRAVEL | _abi.DONE_TIMEOUT
        if stages:
            enable |= _abi.DONE_FK_RESIDUAL | _abi.DONE_INFEASIBLE
        rule = pkg.DoneRule(enable=enable, pos_lo=tuple(home - 0.048), pos_hi=tuple(home + 0.048), min_up=0.5, max_speed=10.0, max_rate=50.0, max_fk_residual=1.0, max_steps=1 << 30)
        rule_s = rule.to_struct()  # built once, as a loop that calls every step would
        d_pose = eng.device_upload(np.ascontiguousarray(pose, dtype=np.float32))
        d_mask, d_reason, d_counts = eng.device_alloc(B), eng.device_alloc(4 * B), eng.device_alloc(4 * _abi.DONE_COUNTS)
        bodies = {
            "evaluate": lambda: eng.evaluate_done_device(rule_s, d_mask, d_reason, d_counts),
            "evaluate, mask only": lambda: eng.evaluate_done_device(rule_s, d_mask),
            "reset_done, no counts": lambda: eng.reset_done_device(rule_s, d_pose),
            "reset_done": lambda: eng.reset_done_device(rule_s, d_pose, 0, d_counts),
            "step": lambda: eng.update(1),
            "evaluate + step": lambda: (eng.evaluate_done_device(rule_s, d_mask, d_reason, d_counts), eng.update(1)),
        }
        for _ in range(20):  # warm-up
            for body in bodies.values():
                timed(eng, body)
        samples = {k: [] for k in bodies}
        for _ in range(ALTERNATIONS):
            for k, body in bodies.items():
                samples[k].append(timed(eng, body))
        med = {k: float(np.median(v)) for k, v in samples.items()}
        counts = eng.evaluate_done(rule)[2]
        lines.append(f"{B} x {N}, stages {stages}: {eng.kernel_name}; {int(counts[0])} robots done per call ({counts[0] / B:.1%})")
        lines.append(f"  evaluate_done_device           {med['evaluate']:8.2f} us per call")
        lines.append(f"  evaluate_done_device, mask only{med['evaluate, mask only']:8.2f} us per call (no counts: nothing is zeroed in front of the kernel)")
        lines.append(f"  reset_done_device              {med['reset_done']:8.2f} us per call (verdict + reset, two launches)")
        lines.append(f"  reset_done_device, no counts   {med['reset_done, no counts']:8.2f} us per call")
        lines.append(f"  update(1)                      {med['step']:8.2f} us per step")
        lines.append(f"  evaluate_done_device + step    {med['evaluate + step']:8.2f} us: the verdict adds {med['evaluate + step'] - med['step']:6.2f} us ({(med['evaluate + step'] - med['step']) / med['step']:5.1%} of a step)")
        old = []
        for _ in range(20):
            eng.synchronize()
            t0 = time.perf_counter()
            p, t = eng.raw_state()
            residual = eng.fk_state()[1] if stages else None
            infeasible = eng.td_state()[1] if stages else None
            mask = host_predicate(rule, p, t, residual, infeasible, eng.limit_state())
            eng.reset_robots(mask, pose)
            eng.synchronize()
            old.append((time.perf_counter() - t0) * 1e6)
        lines.append(f"  host loop ({'four' if stages else 'two'} getters, numpy, reset_robots, synchronize): {float(np.median(old)):10.1f} us by the wall clock")
        eng.synchronize()
        for x in (d_pose, d_mask, d_reason, d_counts):
            eng.device_free(x)
        eng.close()
    text = "\n".join(lines)
    print(text, flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
