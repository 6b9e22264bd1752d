"""What MPPI on the device costs (cdpr_mppi_sample_device, cdpr_mppi_update_device) next to the rollout between them and to the host
path they replace, at BASELINE config 5's rollout (512 robots x 128 samples x 64 steps, 8 cables, FK + TD: a command batch of 134 MB)
and at one small shape (64 x 32 x 16, 4 cables).

Five bodies, all but `host` by HIP events on the engine's stream, LOOP calls back to back per sample, interleaved ALTERNATIONS times
after a warm-up, medians:
  sample   mppi_sample_device(plan -> command batch), NOMINAL_FIRST | CLAMP
  rollout  rollout_velocity_device(command batch -> costs)
  update   mppi_update_device(costs, command batch -> plan, action, weights, ess, status), SHIFT
  loop     the three back to back, then set_velocity_command_device(action)
  host     by the wall clock, HOST_SAMPLES times: numpy normals around the plan, clip, device_upload_into(commands); after the rollout
           device_download(costs), softmin weights and the weighted mean in numpy (the rollout itself is not in this figure)

Bytes: the sampler writes 4 B E bytes and the update reads them once (plus B S costs); both are set against HBM's bandwidth.
The expectations were written down before the first measurement; the script says which of them the figures bear out.
Usage: mppi_cost.py [out.txt]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bench  # noqa: E402
import cdpr_simulation_amd as pkg  # noqa: E402

CASES = [(512, 128, 64, 8), (64, 32, 16, 4)]  # robots, samples, horizon, cables
LOOP, ALTERNATIONS, WARM, HOST_SAMPLES = 10, 40, 3, 5
HBM_PEAK = 8.0e12  # B/s, the figure BASELINE.md takes shares of
EXPECTATIONS = """Expectations (stated before any figure existed):
  1. the sampler runs near the time of a 134 MB write (taken as: at least half of HBM's peak write rate);
  2. the update runs near the time of a 134 MB read (taken as: at least half of HBM's peak read rate);
  3. both are well under the rollout (taken as: each at most a quarter of it)."""


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
    result = {}
    for B, S, H, n in CASES:
        model, pose, _, _ = bench.make_workload(pkg, B, n, 1235, 10)
        eng = pkg.Engine(pkg.Config(model=model, batch=B, stages=3 if n == 8 else 0), 0)
        eng.set_platform_state(pose7=pose)
        eng.update(20)
        eng.synchronize()
        rng = np.random.default_rng(S)
        U = rng.uniform(-0.02, 0.02, (B, H, n)).astype(np.float32)
        spec = pkg.MppiSpec(samples=S, horizon=H, flags=pkg._abi.MPPI_NOMINAL_FIRST | pkg._abi.MPPI_CLAMP | pkg._abi.MPPI_SHIFT, sigma=0.02, cmd_min=-0.1,
                            cmd_max=0.1, temperature=1e-6, seed=2024)
        nbytes = 4 * B * H * S * n
        d_u, d_ref = eng.device_upload(U), eng.device_upload(pose[:, :3].astype(np.float32))
        d_v, d_c, d_action = eng.device_alloc(nbytes), eng.device_alloc(4 * B * S), eng.device_alloc(4 * B * n)
        d_w, d_ess, d_status = eng.device_alloc(4 * B * S), eng.device_alloc(4 * B), eng.device_alloc(4 * pkg._abi.MPPI_STATUS)
        it = [0]

        def sample():
            it[0] += 1
            eng.mppi_sample_device(spec, it[0], d_u, d_v)

        def rollout():
            eng.rollout_velocity_device(d_v, S, H, d_ref, d_c)

        def update():
            eng.mppi_update_device(spec, d_c, d_v, d_u, d_action, d_w, d_ess, d_status)

        def loop():
            sample(), rollout(), update()
            eng.set_velocity_command_device(d_action, B * n)

        sample(), rollout(), update()
        status = eng.device_download(d_status, pkg._abi.MPPI_STATUS, np.uint32)
        ess = eng.device_download(d_ess, B, np.float32)
        bodies = [sample, rollout, update, loop]
        for _ in range(WARM):
            for body in bodies:
                timed(eng, body)
        samples = [[] for _ in bodies]
        for _ in range(ALTERNATIONS):
            for k, body in enumerate(bodies):
                samples[k].append(timed(eng, body))
        med = [float(np.median(x)) for x in samples]
        spread = [float(np.percentile(x, 90) - np.percentile(x, 10)) for x in samples]
        # the host path: what a caller of the library did before these calls existed
        host_up, host_down = [], []
        gen = np.random.default_rng(7)
        for _ in range(HOST_SAMPLES):
            eng.synchronize()
            t0 = time.perf_counter()
            V = np.clip(U[:, :, None, :] + np.float32(0.02) * gen.standard_normal((B, H, S, n), dtype=np.float32), np.float32(-0.1), np.float32(0.1))
            V[:, :, 0, :] = U
            eng.device_upload_into(d_v, V)
            eng.synchronize()
            host_up.append((time.perf_counter() - t0) * 1e6)
            rollout()
            eng.synchronize()
            t0 = time.perf_counter()
            c = eng.device_download(d_c, (B, S), np.float32).astype(np.float64)
            w = np.exp((c.min(axis=1, keepdims=True) - c) / 1e-6)
            plan = np.einsum("bs,bhsn->bhn", w, V) / w.sum(axis=1)[:, None, None]
            eng.device_upload_into(d_u, np.concatenate([plan[:, 1:], plan[:, -1:]], axis=1).astype(np.float32))
            eng.set_velocity_command(plan[:, 0].astype(np.float32))
            eng.synchronize()
            host_down.append((time.perf_counter() - t0) * 1e6)
        hu, hd = float(np.median(host_up)), float(np.median(host_down))
        s_us, r_us, u_us, l_us = med
        result[(B, S, H)] = med
        say(f"{B} robots x {S} samples x {H} steps, {n} cables ({eng.kernel_name}): command batch {nbytes / 1e6:.1f} MB, "
            f"{int(status[0])} robots updated, {int(status[1])} degenerate, {int(status[2])} bad costs, median ess {float(np.median(ess)):.1f} of {S}")
        say(f"  sample {s_us:9.2f} us   rollout {r_us:9.2f} us   update {u_us:9.2f} us   the three and the command, back to back {l_us:9.2f} us "
            f"(sum of the parts {s_us + r_us + u_us:9.2f} us)")
        say(f"  spread (p90 - p10) {spread[0]:7.2f} / {spread[1]:7.2f} / {spread[2]:7.2f} / {spread[3]:7.2f} us over {ALTERNATIONS} samples of {LOOP} calls")
        say(f"  sample writes {nbytes / s_us / 1e6:7.3f} TB/s ({nbytes / s_us / 1e6 / (HBM_PEAK / 1e12):5.1%} of 8 TB/s)   "
            f"update reads {(nbytes + 4 * B * S) / u_us / 1e6:7.3f} TB/s ({(nbytes + 4 * B * S) / u_us / 1e6 / (HBM_PEAK / 1e12):5.1%})   "
            f"sample / rollout {s_us / r_us:5.2f}   update / rollout {u_us / r_us:5.2f}")
        say(f"  host path: normals + clip + upload {hu:11.1f} us   download + weights + mean + uploads {hd:11.1f} us (wall clock)   "
            f"host / device: {hu / s_us:8.1f} x and {hd / u_us:8.1f} x")
        eng.synchronize()
        for d in (d_u, d_ref, d_v, d_c, d_action, d_w, d_ess, d_status):
            eng.device_free(d)
        eng.close()
    say("")
    B, S, H, n = CASES[0]
    s_us, r_us, u_us, _ = result[(B, S, H)]
    nbytes = 4 * B * H * S * n
    say(f"1. {'holds' if nbytes / s_us / 1e6 >= 0.5 * HBM_PEAK / 1e12 else 'FAILS'}: the sampler writes {nbytes / s_us / 1e6:.2f} TB/s at {B} x {S} x {H}")
    say(f"2. {'holds' if nbytes / u_us / 1e6 >= 0.5 * HBM_PEAK / 1e12 else 'FAILS'}: the update reads {nbytes / u_us / 1e6:.2f} TB/s")
    say(f"3. {'holds' if max(s_us, u_us) <= 0.25 * r_us else 'FAILS'}: sample {s_us / r_us:.2f} and update {u_us / r_us:.2f} of the rollout's {r_us:.1f} us")
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
