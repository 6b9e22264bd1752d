"""Host overhead per call, parent library against this one: median of update(1) + synchronize() over 2 000 calls at B = 64 (a toy size on
purpose: a measurement of host overhead) on a register-resident, a general-path and a precision = 64 HOLD handle.  Child processes,
alternating A B B A A B, three runs per build.
  python scripts/host_args_latency.py LIB_A LIB_B        |        python scripts/host_args_latency.py one"""
import os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

HANDLES = (("register-resident", dict()), ("general path", dict(velocityEpsilon=0.001)), ("fp64 HOLD", dict(velocityEpsilon=0.001, precision=64)))


def one():
    import cdpr_simulation_amd as pkg
    for name, kw in HANDLES:
        eng = pkg.Engine(pkg.Config(model=pkg.eight_cable_model(), batch=64, stages=3, **kw), 0)
        eng.set_velocity_command(np.full(8, 0.01, dtype=np.float32))
        for _ in range(300):
            eng.update(1); eng.synchronize()
        ts = np.empty(2000)
        for i in range(2000):
            t0 = time.perf_counter()
            eng.update(1); eng.synchronize()
            ts[i] = time.perf_counter() - t0
        # ... and the enqueue alone (no wait in the timed part): what the host pays before the launch is on the stream
        qs = np.empty(2000)
        for i in range(2000):
            t0 = time.perf_counter()
            eng.update(1)
            qs[i] = time.perf_counter() - t0
            eng.synchronize()
        print(f"row {name}: median {np.median(ts) * 1e6:.2f} us  p10 {np.percentile(ts, 10) * 1e6:.2f}  p90 {np.percentile(ts, 90) * 1e6:.2f}  enqueue-only median {np.median(qs) * 1e6:.2f}", flush=True)
        eng.close()


if __name__ == "__main__":
    if sys.argv[1:2] == ["one"]:
        one()
        sys.exit(0)
    a, b = sys.argv[1], sys.argv[2]
    rows = {}
    for lib in (a, b, b, a, a, b):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "one"], env=dict(os.environ, CDPR_LIB=lib), capture_output=True, text=True, timeout=240)
        if r.returncode != 0:
            print(r.stdout, r.stderr)
            sys.exit(r.returncode or 1)
        for line in r.stdout.splitlines():
            if line.startswith("row "):
                print(f"{lib:26s} {line[4:]}", flush=True)
                name = line[4:line.index(":")]
                f = line.split()
                rows.setdefault(name, {}).setdefault(lib, []).append((float(f[f.index("median") + 1]), float(f[-1])))
    print(f"update(1) + synchronize(), B = 64, n = 8, FK + TD: medians of 2 000 calls, three runs per build; A (parent) = {a}, B (this tree) = {b}")
    for name, by in rows.items():
        for col, what in ((0, "update+sync"), (1, "enqueue only")):
            xa, xb = [x[col] for x in by[a]], [x[col] for x in by[b]]
            mb = float(np.median(xb))
            verdict = "within A's runs" if min(xa) <= mb <= max(xa) else ("below A's lowest" if mb < min(xa) else "ABOVE A's highest")
            print(f"{name:18s} {what:13s} A {' '.join(f'{x:7.2f}' for x in xa)}  (spread {max(xa) - min(xa):.2f})   B {' '.join(f'{x:7.2f}' for x in xb)}   B's median {verdict}")
