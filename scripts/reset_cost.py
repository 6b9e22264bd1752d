"""What a model reset of some robots costs next to the step it sits in front of (cdpr_reset_robots_device): 65 536 x 8, FK + TD,
per_robot_commands, on the register-resident handle and on the general path's lean role-split handle (velocityEpsilon 0.002, hot rows).

Two loops by HIP events on the engine's stream, in one process, alternating 500 times after a warm-up:
  A  LOOP x { reset_robots_device(mask, poses); update(1) }        B  LOOP x { update(1) }
for three masks (1 robot in 64, every other robot, every robot); A - B is the reset.  Beside it the only route there was before
- raw_state + set_platform_state, which waits for the stream twice and resets no controller, so it is a lower bound on the old cost -
by the wall clock.  Usage: reset_cost.py [out.txt]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bench  # noqa: E402
import cdpr_simulation_amd as pkg  # noqa: E402

B, N, LOOP, ALTERNATIONS = 65536, 8, 10, 500
HANDLES = {"register-resident": dict(stages=3), "general lean (hot rows)": dict(stages=3, velocityEpsilon=0.002)}
MASKS = {"1/64": lambda r: r % 64 == 0, "1/2": lambda r: r % 2 == 0, "all": lambda r: r >= 0}


def timed(eng, body):
    eng.profile_begin()
    for _ in range(LOOP):
        body()
    return eng.profile_end()[0] * 1e3 / LOOP  # us per iteration


def main():
    lines = []
    model, pose, command, _ = bench.make_workload(pkg, B, N, 1235, 10)
    for name, kw in HANDLES.items():
        eng = pkg.Engine(pkg.Config(model=model, batch=B, perRobotCommands=True, **kw), 0)
        eng.set_platform_state(pose7=pose)
        eng.set_velocity_command(command(0))
        eng.update(200)
        eng.synchronize()
        d_pose = eng.device_upload(np.ascontiguousarray(pose, dtype=np.float32))
        lines.append(f"{name}: {eng.kernel_name}")
        for label, pick in MASKS.items():
            d_mask = eng.device_upload(pick(np.arange(B)).astype(np.uint8))

            def with_reset():
                eng.reset_robots_device(d_mask, d_pose)
                eng.update(1)

            for _ in range(20):  # warm-up
                timed(eng, with_reset), timed(eng, lambda: eng.update(1))
            a, b = [], []
            for _ in range(ALTERNATIONS):
                a.append(timed(eng, with_reset))
                b.append(timed(eng, lambda: eng.update(1)))
            a, b = float(np.median(a)), float(np.median(b))
            lines.append(f"  mask {label:5s} reset + step {a:7.2f} us   step alone {b:7.2f} us   reset {a - b:6.2f} us ({(a - b) / b:5.1%} of a step)")
            eng.synchronize()
            eng.device_free(d_mask)
        old = []
        for _ in range(20):
            eng.synchronize()
            t0 = time.perf_counter()
            p, t = eng.raw_state()
            eng.set_platform_state(p, t)
            old.append((time.perf_counter() - t0) * 1e6)
        lines.append(f"  raw_state + set_platform_state (platform only, host in the loop): {float(np.median(old)):9.1f} us by the wall clock")
        eng.device_free(d_pose)
        eng.close()
    text = "\n".join(lines)
    print(text, flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
