"""Host in the loop, one world step at a time — what a Gazebo-style caller pays per step (the reference's own use:
ConnectWorldUpdateBegin -> update() every 1 ms step, messages published every step).  Two levels:
  C-ABI   cdpr_update(1) + cdpr_get_observables (one gather launch into a pinned host image, host spins on its completion
          word), against the two separate getters (five gather / copy / wait rounds) and against no read-out at all
  facade  CdprGazeboPlugin.update() with a subscriber on jointStates / platformPose and a 100 Hz sine publisher
for the reference's robot (1 x 4 cables) and for batches.

  python scripts/host_loop_latency.py getters          the per-getter table: update(1) + one getter, us per step, for every getter of a
                                                       published step or of the state, every shape, both precisions where they apply
  python scripts/host_loop_latency.py ab LIB_A LIB_B   that table for two builds of the library (CDPR_LIB), three runs each in alternating
                                                       child processes (A B, B A, A B): a getter's figures are its three medians per build
  python scripts/host_loop_latency.py one              update(1) + the five-array getter at ONE robot (observables at 1 x 4 and 1 x 8, observables_f64
                                                       on precision = 64): median, minimum and maximum of nine blocks of 2 000 steps, then 2 000
                                                       calls of the getter alone
  python scripts/host_loop_latency.py one-ab LIB_A LIB_B   that for two builds, four runs each in the order A B B A A B B A: at one robot a build's own
                                                       medians spread further than three runs show"""
import os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import cdpr_simulation_amd as pkg

def c_abi(batch, n, steps=3000):
    model = pkg.cube_model() if n == 4 else pkg.eight_cable_model()
    eng = pkg.Engine(pkg.Config(model=model, batch=batch, stages=0 if n == 4 else 3), 0)
    eng.set_velocity_command(np.full(n, 0.01, dtype=np.float32))
    for _ in range(200):
        eng.update(1); eng.joint_states(); eng.platform_state()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(steps):
            eng.update(1); eng.joint_states(); eng.platform_state()
        ts.append((time.perf_counter() - t0) / steps * 1e6)
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.update(1); eng.synchronize()
    only = (time.perf_counter() - t0) / steps * 1e6
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.update(1); eng.observables()
    one = (time.perf_counter() - t0) / steps * 1e6
    eng.close()
    return float(np.median(ts)), only, one

def facade(steps=3000):
    from cdpr_simulation_amd.messages import Joy
    bus = pkg.TopicBus(); got = [0]
    plug = pkg.CdprGazeboPlugin(bus); plug.Load(pkg.Config())
    bus.subscribe("jointStates", lambda m: got.__setitem__(0, got[0] + 1)); bus.subscribe("platformPose", lambda m: None)
    pub = bus.advertise("jointVelocities")
    for k in range(200): plug.update()
    t0 = time.perf_counter()
    for k in range(steps):
        if k % 10 == 0: pub(Joy(axes=[np.float32(0.05 * np.sin(2 * np.pi * 0.1 * k * 1e-3))] * 4))
        plug.update()
    return (time.perf_counter() - t0) / steps * 1e6, got[0]

SHAPES = ((1, 4), (1, 8), (4096, 4), (65536, 8))
GETTERS = ("observables", "joint_states", "platform_state", "raw_state", "fk_state", "observables_f64")

def getter_table():
    """{(precision, batch, n, getter): us per step of update(1) + getter, the median of five blocks}"""
    out = {}
    for precision in (32, 64):
        for batch, n in SHAPES:
            model = pkg.cube_model() if n == 4 else pkg.eight_cable_model()
            eng = pkg.Engine(pkg.Config(model=model, batch=batch, stages=0 if n == 4 else 3, precision=precision), 0)
            eng.set_velocity_command(np.full(n, 0.01, dtype=np.float32))
            steps = 1000 if batch <= 4096 else 100
            for name in GETTERS:
                if (name == "fk_state" and n == 4) or (name == "observables_f64" and precision != 64):
                    continue
                get = getattr(eng, name)
                for _ in range(50):
                    eng.update(1); get()
                ts = []
                for _ in range(5):
                    t0 = time.perf_counter()
                    for _ in range(steps):
                        eng.update(1); get()
                    ts.append((time.perf_counter() - t0) / steps * 1e6)
                out[(precision, batch, n, name)] = float(np.median(ts))
            eng.close()
    return out

def print_table(table):
    for (precision, batch, n, name), us in table.items():
        print(f"getter fp{precision} {batch:6d} x {n} update(1) + {name:16s} {us:9.1f} us/step", flush=True)

def one_robot():
    for precision, name in ((32, "observables"), (64, "observables_f64")):
        for batch, n in SHAPES[:2]:
            model = pkg.cube_model() if n == 4 else pkg.eight_cable_model()
            eng = pkg.Engine(pkg.Config(model=model, batch=batch, stages=0 if n == 4 else 3, precision=precision), 0)
            eng.set_velocity_command(np.full(n, 0.01, dtype=np.float32))
            get = getattr(eng, name)
            for _ in range(500):
                eng.update(1); get()
            ts = []
            for _ in range(9):
                t0 = time.perf_counter()
                for _ in range(2000):
                    eng.update(1); get()
                ts.append((time.perf_counter() - t0) / 2000 * 1e6)
            t0 = time.perf_counter()
            for _ in range(2000):
                get()
            alone = (time.perf_counter() - t0) / 2000 * 1e6
            print(f"row fp{precision} {batch} x {n} {name}: median {np.median(ts):.2f} min {min(ts):.2f} max {max(ts):.2f} getter alone {alone:.2f}", flush=True)
            eng.close()

def one_robot_ab(lib_a, lib_b):
    for lib in (lib_a, lib_b, lib_b, lib_a, lib_a, lib_b, lib_b, lib_a):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "one"], env=dict(os.environ, CDPR_LIB=lib), capture_output=True, text=True, check=True)
        for line in r.stdout.splitlines():
            if line.startswith("row "):
                print(f"{lib:24s} {line[4:]}", flush=True)

def ab(lib_a, lib_b, runs=3):
    rows = {}
    for run in range(runs):
        for lib in ((lib_a, lib_b) if run % 2 == 0 else (lib_b, lib_a)):  # (both orders: a build's figures also move with its place in the pair)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "getters"], env=dict(os.environ, CDPR_LIB=lib), capture_output=True, text=True, check=True)
            for line in r.stdout.splitlines():
                if line.startswith("getter "):
                    rows.setdefault(line[7:line.index("+") + 18], {}).setdefault(lib, []).append(float(line.split()[-2]))
    print(f"update(1) + getter, us per step, {runs} runs per build in alternating child processes: A = {lib_a}, B = {lib_b}")
    for key, by_lib in rows.items():
        a, b = by_lib[lib_a], by_lib[lib_b]
        verdict = "within A's runs" if min(a) <= np.median(b) <= max(a) else ("faster than A's fastest" if np.median(b) < min(a) else "SLOWER than A's slowest")
        print(f"{key}  A {' '.join(f'{x:8.1f}' for x in a)}   B {' '.join(f'{x:8.1f}' for x in b)}   B's median {verdict}")

if __name__ == "__main__":
    if sys.argv[1:2] == ["getters"]:
        print_table(getter_table())
        sys.exit(0)
    if sys.argv[1:2] == ["one"]:
        one_robot()
        sys.exit(0)
    if sys.argv[1:2] == ["one-ab"]:
        one_robot_ab(sys.argv[2], sys.argv[3])
        sys.exit(0)
    if sys.argv[1:2] == ["ab"]:
        ab(sys.argv[2], sys.argv[3])
        sys.exit(0)
    for batch, n in ((1, 4), (1, 8), (4096, 4), (65536, 8)):
        full, only, one = c_abi(batch, n, 3000 if batch <= 4096 else 600)
        print(f"C-ABI  {batch:6d} x {n}: update(1) + cdpr_get_observables {one:7.1f} us/step (real-time factor of a 1 ms step {1000.0 / one:6.1f})   "
              f"update(1) + get_joint_states + get_platform_state {full:7.1f}   update(1) + synchronize only {only:6.1f}")
    us, n_msgs = facade()
    print(f"facade      1 x 4: CdprGazeboPlugin.update() with subscribers and a 100 Hz sine publisher {us:8.1f} us/step ({n_msgs} JointState messages)   real-time factor {1000.0 / us:7.1f}")
