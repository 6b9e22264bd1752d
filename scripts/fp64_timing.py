"""precision = 64 beside fp32: us per world step (HIP events, one launch per step and ten steps per launch) for config 1
(one 4-cable robot), 4 096 x 4 and 4 096 x 8 with FK + TD."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
os.environ["CDPR_NO_GRAPH"] = "1"
import cdpr_simulation_amd as pkg, bench
for B, n, stages in ((1, 4, 0), (4096, 4, 0), (1, 8, 3), (4096, 8, 3), (65536, 8, 3)):
    model, pose, command, _ = bench.make_workload(pkg, B, n, 1235, 10)
    for prec in (32, 64):
        eng = pkg.Engine(pkg.Config(model=model, batch=B, stages=stages, precision=prec), 0)
        eng.set_platform_state(pose7=pose); eng.set_velocity_command(command(0)); eng.update(50); eng.synchronize()
        out = []
        for spl in (1, 10):
            ts = []
            for rnd in range(5):
                eng.profile_begin(); eng.update(200, spl); ms, nl = eng.profile_end(); ts.append(ms / 200 * 1e3)
            out.append(f"spl={spl}: {np.median(ts):.2f} us/step")
        print(f"B={B} n={n} stages={stages} fp{prec} ({eng.mapping}): " + ", ".join(out), flush=True)
        eng.close()

# The hold branch (velocityEpsilon >= 0) in double beside the fp32 general path: steady commands above epsilon, then a third of
# the cables at or below it (their windows non-uniform: fits).
for B, n, stages in ((1, 8, 3), (4096, 8, 3), (65536, 8, 3)):
    model, pose, command, _ = bench.make_workload(pkg, B, n, 1235, 10)
    rng = np.random.default_rng(5)
    for prec in (32, 64):
        eng = pkg.Engine(pkg.Config(model=model, batch=B, stages=stages, precision=prec, velocityEpsilon=0.001), 0)
        eng.set_platform_state(pose7=pose); eng.set_velocity_command(command(0)); eng.update(120); eng.synchronize()
        out = []
        for label in ("steady", "holding"):
            if label == "holding":
                cmd = command(0).copy(); low = rng.random(cmd.shape) < 0.33; cmd[low] = (0.0005 * rng.uniform(-1, 1, int(low.sum()))).astype(np.float32)
                eng.set_velocity_command(cmd); eng.update(120)
            ts = []
            for rnd in range(5):
                eng.profile_begin(); eng.update(200, 1); ms, nl = eng.profile_end(); ts.append(ms / 200 * 1e3)
            out.append(f"{label}: {np.median(ts):.2f} us/step")
        print(f"hold branch B={B} n={n} stages={stages} fp{prec} ({eng.mapping}): " + ", ".join(out), flush=True)
        eng.close()

# The other families of the one-wave fp64 kernel, by the kernel the handle ran: per-robot modes, derivative windows of 12 .. 32 samples
# (W = 31), the joint stop with lumped legs (TSTOP), and the long HOLD records (HW = 32).
from dataclasses import replace
for B in (1, 65536):
    model, pose, command, _ = bench.make_workload(pkg, B, 8, 1235, 10)
    stop = replace(model, passive_damping=0.01, leg_inertia=0.004, travel_lower=-0.004, travel_upper=0.004, travel_stop=2)
    for label, kw, window in (("per-robot", dict(perRobotCommands=True), None), ("long window", dict(), 16), ("per-robot, long window", dict(perRobotCommands=True), 16),
                              ("joint stop", dict(model=stop), None), ("hold, long window", dict(velocityEpsilon=0.001), 16)):
        cfg = pkg.Config(**dict(dict(model=model, batch=B, stages=3, precision=64), **kw))
        if window:
            cfg.velocityController.dBufferLength = window
        eng = pkg.Engine(cfg, 0)
        eng.set_platform_state(pose7=pose); eng.set_velocity_command(command(0)); eng.update(120); eng.synchronize()
        ts = []
        for rnd in range(5):
            eng.profile_begin(); eng.update(200, 1); ms, nl = eng.profile_end(); ts.append(ms / 200 * 1e3)
        print(f"{label} B={B} n=8 stages=3 fp64 {eng.kernel_name}: {np.median(ts):.2f} us/step", flush=True)
        eng.close()
