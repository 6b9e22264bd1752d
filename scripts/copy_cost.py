"""What forking robots onto others costs (cdpr_copy_robots_device) next to a model reset of the same robots
(cdpr_reset_robots_device) and next to the step it sits in front of: 65 536 x 8 and 4 096 x 4, per_robot_commands, one handle per
record layout - register-resident, general path (velocityEpsilon 0.002; hot rows at 65 536 x 8), precision = 64.

Four loops by HIP events on the engine's stream, in one process, interleaved ALTERNATIONS times after a warm-up:
  C  LOOP x { copy_robots_device(map); update(1) }      R  LOOP x { reset_robots_device(the map's destinations); update(1) }
  S  LOOP x { update(1) }                               A  LOOP x { copy_robots_device(map) }  (the copy alone, back to back)
for two maps: "quarter" (every fourth robot takes its right neighbour: one destination in four lanes of every wavefront) and "waves"
(the robots of every fourth wavefront take the wavefront behind them, lane for lane: full-wave copies, the same number of robots).
C - S is the copy in a loop, R - S the reset.  Usage: copy_cost.py [out.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bench  # noqa: E402
import cdpr_simulation_amd as pkg  # noqa: E402

SIZES = [(65536, 8), (4096, 4)]
LOOP, ALTERNATIONS, WARM = 10, 200, 10
HANDLES = {"register-resident": dict(), "general path": dict(velocityEpsilon=0.002), "precision = 64": dict(precision=64)}


def maps(batch):
    r = np.arange(batch)
    quarter = np.where(r % 4 == 0, r + 1, -1).astype(np.int32)
    waves = np.where((r // 64) % 4 == 0, r + 64, -1).astype(np.int32)
    return {"quarter": quarter, "waves": waves}


def timed(eng, body):
    eng.profile_begin()
    for _ in range(LOOP):
        body()
    return eng.profile_end()[0] * 1e3 / LOOP  # us per iteration


def main():
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    for batch, n in SIZES:
        model, pose, command, _ = bench.make_workload(pkg, batch, n, 1235, 10)
        for name, kw in HANDLES.items():
            eng = pkg.Engine(pkg.Config(model=model, batch=batch, stages=3 if n == 8 else 0, perRobotCommands=True, **kw), 0)
            eng.set_platform_state_f64(pose7=pose.astype(np.float64)) if kw.get("precision") == 64 else eng.set_platform_state(pose7=pose)
            eng.set_velocity_command(command(0))
            eng.update(200)
            eng.synchronize()
            d_pose = eng.device_upload(pose)
            say(f"{batch} x {n}, {name}: {eng.kernel_name}")
            for label, source in maps(batch).items():
                assert source.max() < batch
                dest = source >= 0
                d_source, d_mask = eng.device_upload(source), eng.device_upload(dest.astype(np.uint8))

                def copy_step():
                    eng.copy_robots_device(d_source)
                    eng.update(1)

                def reset_step():
                    eng.reset_robots_device(d_mask, d_pose)
                    eng.update(1)

                bodies = [copy_step, reset_step, lambda: eng.update(1), lambda: eng.copy_robots_device(d_source)]
                for _ in range(WARM):
                    for body in bodies:
                        timed(eng, body)
                samples = [[] for _ in bodies]
                for _ in range(ALTERNATIONS):
                    for k, body in enumerate(bodies):
                        samples[k].append(timed(eng, body))
                c, r, s, a = (float(np.median(x)) for x in samples)
                say(f"  map {label:8s} ({int(dest.sum()):6d} robots)  step alone {s:8.2f} us   copy + step {c:8.2f}   reset + step {r:8.2f}   "
                             f"copy {c - s:7.2f} us ({(c - s) / s:6.1%} of a step)   reset {r - s:7.2f} us   copy alone, back to back {a:7.2f} us")
                eng.synchronize()
                eng.device_free(d_source), eng.device_free(d_mask)
            eng.device_free(d_pose)
            eng.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
