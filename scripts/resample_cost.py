"""What resampling on the device costs (cdpr_resample_map_device, cdpr_resample_device) next to the fork it feeds, to a launch floor
and to the host round trip it replaces: per_robot_commands handles on the register-resident path, heavy-tailed weights
(rand ** 8), one random word per group, ess_gate 2 (every group is resampled).

  512 groups x 128 robots (65 536 x 8)      1 group x 65 536 robots (65 536 x 8)      1 group x 4 096 robots (4 096 x 4)

Six bodies, all but `host` by HIP events on the engine's stream, LOOP calls back to back per sample, interleaved ALTERNATIONS times
after a warm-up, medians:
  map     resample_map_device(weights, words -> map, ess, status)
  fused   resample_device(the same): the map, then the copy kernel on it
  copy    copy_robots_device(the map the first body made)
  floor   evaluate_done_device(mask only): one small launch over the batch, the launch floor
  bare    resample_map_device(weights, words -> map): no ess, no status - one launch, no memset of the status words in front
  host    by the wall clock, HOST_SAMPLES times: device_download(weights), systematic resampling in numpy (cumulative sum, search,
          survivors keep their index), copy_robots(map), synchronize - the path a loop took before these calls existed

The expectations were written down before the first measurement; the script says which of them the figures bear out.
Usage: resample_cost.py [out.txt]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bench  # noqa: E402
import cdpr_simulation_amd as pkg  # noqa: E402

CASES = [(65536, 8, 128), (65536, 8, 65536), (4096, 4, 4096)]  # batch, cables, group size
LOOP, ALTERNATIONS, WARM, HOST_SAMPLES = 10, 100, 5, 15
EXPECTATIONS = """Expectations (stated before any figure existed):
  1. the map call at many small groups (512 x 128) is within a few launch floors (taken as: at most 4 floors);
  2. the fused call costs about the map plus the copy (taken as: within 25 % of their sum);
  3. the single group of 65 536, one workgroup on one CU, is the slow case (the slowest map call of the three)."""


def host_map(w, P, words):
    """systematic resampling as a host loop writes it: float cumulative sums, one search per group, survivors keep their index"""
    w = w.reshape(-1, P).astype(np.float64)
    G = len(w)
    w = np.where(np.isfinite(w) & (w > 0), w, 0.0)
    c = np.cumsum(w, axis=1)
    pos = (np.arange(P)[None, :] + (words.astype(np.float64) / 2.0**32)[:, None]) / P * c[:, -1:]
    src = np.full((G, P), -1, np.int32)
    for g in range(G):
        counts = np.bincount(np.minimum(np.searchsorted(c[g], pos[g], side="right"), P - 1), minlength=P)
        dead = np.flatnonzero(counts == 0)
        src[g, dead] = g * P + np.repeat(np.arange(P), np.maximum(counts - 1, 0))[:len(dead)]
    return src.reshape(-1)


def timed(eng, body):
    eng.profile_begin()
    for _ in range(LOOP):
        body()
    return eng.profile_end()[0] * 1e3 / LOOP  # us per call


def main():
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    say(EXPECTATIONS)
    say("")
    rule = pkg.DoneRule(enable=pkg._abi.DONE_NONFINITE)
    result = {}
    for batch, n, P in CASES:
        G = batch // P
        model, pose, command, _ = bench.make_workload(pkg, batch, n, 1235, 10)
        eng = pkg.Engine(pkg.Config(model=model, batch=batch, stages=3 if n == 8 else 0, perRobotCommands=True), 0)
        eng.set_platform_state(pose7=pose)
        eng.set_velocity_command(command(0))
        eng.update(200)
        eng.synchronize()
        rng = np.random.default_rng(P)
        w = rng.random(batch, np.float32) ** np.float32(8)
        words = rng.integers(0, 1 << 32, G, dtype=np.uint64).astype(np.uint32)
        spec = pkg.ResampleSpec(P)
        d_w, d_u = eng.device_upload(w), eng.device_upload(words)
        d_map, d_fused_map, d_bare_map, d_mask = eng.device_alloc(4 * batch), eng.device_alloc(4 * batch), eng.device_alloc(4 * batch), eng.device_alloc(batch)
        d_ess, d_status = eng.device_alloc(4 * G), eng.device_alloc(4 * pkg._abi.RESAMPLE_STATUS)
        eng.resample_map_device(spec, d_w, d_map, d_u, d_ess, d_status)
        status = eng.device_download(d_status, pkg._abi.RESAMPLE_STATUS, np.uint32)
        bodies = [lambda: eng.resample_map_device(spec, d_w, d_map, d_u, d_ess, d_status),
                  lambda: eng.resample_device(spec, d_w, d_fused_map, d_u, d_ess, d_status),
                  lambda: eng.copy_robots_device(d_map),
                  lambda: eng.evaluate_done_device(rule, d_mask),
                  lambda: eng.resample_map_device(spec, d_w, d_bare_map, d_u)]
        for _ in range(WARM):
            for body in bodies:
                timed(eng, body)
        samples = [[] for _ in bodies]
        for _ in range(ALTERNATIONS):
            for k, body in enumerate(bodies):
                samples[k].append(timed(eng, body))
        m, f, c, floor, bare = (float(np.median(x)) for x in samples)
        host = []
        for _ in range(HOST_SAMPLES):
            eng.synchronize()
            t0 = time.perf_counter()
            eng.copy_robots(host_map(eng.device_download(d_w, batch, np.float32), P, words))
            eng.synchronize()
            host.append((time.perf_counter() - t0) * 1e6)
        h = float(np.median(host))
        result[(batch, P)] = (m, f, c, floor)
        say(f"{G} group(s) x {P} robots ({batch} x {n}, {eng.kernel_name}): {int(status[0])} robots copied, {int(status[2])} group(s) resampled")
        say(f"  map {m:9.2f} us   fused {f:9.2f} us   copy on the same map {c:8.2f} us   launch floor {floor:7.2f} us   host path {h:10.1f} us (wall clock)")
        say(f"  map = {m / floor:6.1f} floors   fused / (map + copy) = {f / (m + c):5.2f}   host path / fused = {h / f:7.1f}   "
            f"map without ess and status (no memset in front, one launch) {bare:8.2f} us")
        eng.synchronize()
        for d in (d_w, d_u, d_map, d_fused_map, d_bare_map, d_mask, d_ess, d_status):
            eng.device_free(d)
        eng.close()
    say("")
    m, f, c, floor = result[(65536, 128)]
    say(f"1. {'holds' if m <= 4 * floor else 'FAILS'}: the map call at 512 x 128 is {m / floor:.1f} launch floors")
    worst = max(abs(f / (m + c) - 1.0) for m, f, c, _ in result.values())
    say(f"2. {'holds' if worst <= 0.25 else 'FAILS'}: the fused call is within {worst:.0%} of map + copy at every size")
    slow = result[(65536, 65536)][0]
    say(f"3. {'holds' if slow >= max(v[0] for v in result.values()) else 'FAILS'}: the single group of 65 536 takes {slow:.1f} us, "
        f"{slow / m:.1f} x the 512 x 128 call on the same batch")
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
