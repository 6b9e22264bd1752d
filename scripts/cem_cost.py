"""What CEM on the device costs (cdpr_cem_sample_device, cdpr_cem_update_device) next to (a) the host path it replaces and (b) the MPPI
sample and update of the same build, at BASELINE config 5's rollout (512 robots x 128 samples x 64 steps, 8 cables, FK + TD: a command
batch of 134 MB) with K = 13 elites, and at one small shape (64 x 32 x 16, 4 cables, K = 4).

All bodies but `host` by HIP events on the engine's stream, LOOP calls back to back per sample, interleaved ALTERNATIONS times after a
warm-up, medians:
  sample        cem_sample_device(mean, sigma -> command batch), NOMINAL_FIRST | CLAMP
  rollout       rollout_velocity_device(command batch -> costs)
  update        cem_update_device(costs, command batch -> mean, sigma, action, elite, best, status), SHIFT, alpha 0.7
  loop          the three back to back, then set_velocity_command_device(action)
  mppi sample / mppi update   the MPPI calls on the same buffers
  update K = 1, update K = S  the same update with one elite (the selection and next to no rows) and with every sample an elite (the
                whole batch read twice from the cache hierarchy): where the update's time goes, and the rate at which the rows of
                4 n bytes of K = 13 scattered elites come in - (K - 1) H n 4 B bytes over the time K = 13 takes longer than K = 1
  update H = 1  the same update (K = 13) told that the horizon is one step: the status words' memset, the launch, the whole selection
                and ONE round of the fit; what the full horizon takes longer is the other H / 4 - 1 rounds of the fit, a wave per step
  host          by the wall clock, HOST_SAMPLES times: numpy normals times sigma around the mean, clip, device_upload_into(commands);
                after the rollout device_download(costs), numpy.argpartition, mean and std of the elites, blend, the uploads (the
                rollout itself is not in this figure)

The update reads K / S of what the MPPI update reads; the script says whether it is faster and, if it is not, which part takes the time.
Usage: cem_cost.py [out.txt]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bench  # noqa: E402
import cdpr_simulation_amd as pkg  # noqa: E402

CASES = [(512, 128, 64, 8, 13), (64, 32, 16, 4, 4)]  # robots, samples, horizon, cables, elites
LOOP, ALTERNATIONS, WARM, HOST_SAMPLES = 10, 40, 3, 5
ALPHA, SIGMA_MIN, SIGMA_MAX = 0.7, 1e-3, 0.05


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

    A = pkg._abi
    for B, S, H, n, K in CASES:
        model, pose, _, _ = bench.make_workload(pkg, B, n, 1235, 10)
        eng = pkg.Engine(pkg.Config(model=model, batch=B, stages=3 if n == 8 else 0), 0)
        eng.set_platform_state(pose7=pose)
        eng.update(20)
        eng.synchronize()
        rng = np.random.default_rng(S)
        U = rng.uniform(-0.02, 0.02, (B, H, n)).astype(np.float32)
        G = np.full((B, H, n), 0.02, np.float32)
        kw = dict(samples=S, horizon=H, flags=A.CEM_NOMINAL_FIRST | A.CEM_CLAMP | A.CEM_SHIFT, alpha=ALPHA, sigma_min=SIGMA_MIN, sigma_max=SIGMA_MAX,
                  cmd_min=-0.1, cmd_max=0.1, seed=2024)
        spec, spec_1, spec_all = pkg.CemSpec(elites=K, **kw), pkg.CemSpec(elites=1, **kw), pkg.CemSpec(elites=S, **kw)
        spec_h1 = pkg.CemSpec(elites=K, **dict(kw, horizon=1))
        mspec = pkg.MppiSpec(samples=S, horizon=H, flags=A.MPPI_NOMINAL_FIRST | A.MPPI_CLAMP | A.MPPI_SHIFT, sigma=0.02, cmd_min=-0.1, cmd_max=0.1,
                             temperature=1e-6, seed=2024)
        nbytes = 4 * B * H * S * n
        d_u, d_g, d_ref = eng.device_upload(U), eng.device_upload(G), eng.device_upload(pose[:, :3].astype(np.float32))
        d_v, d_c, d_action = eng.device_alloc(nbytes), eng.device_alloc(4 * B * S), eng.device_alloc(4 * B * n)
        d_e, d_best, d_status = eng.device_alloc(4 * B * S), eng.device_alloc(4 * B), eng.device_alloc(4 * A.CEM_STATUS)
        d_mu, d_w, d_ess, d_mstatus = eng.device_upload(U), eng.device_alloc(4 * B * S), eng.device_alloc(4 * B), eng.device_alloc(4 * A.MPPI_STATUS)
        it = [0]

        def sample():
            it[0] += 1
            eng.cem_sample_device(spec, it[0], d_u, d_g, d_v)

        def rollout():
            eng.rollout_velocity_device(d_v, S, H, d_ref, d_c)

        def update(s=spec):
            eng.cem_update_device(s, d_c, d_v, d_u, d_g, d_action, d_e, d_best, d_status)

        def loop():
            sample(), rollout(), update()
            eng.set_velocity_command_device(d_action, B * n)

        def mppi_sample():
            it[0] += 1
            eng.mppi_sample_device(mspec, it[0], d_mu, d_v)

        def mppi_update():
            eng.mppi_update_device(mspec, d_c, d_v, d_mu, d_action, d_w, d_ess, d_mstatus)

        sample(), rollout(), update()
        status = eng.device_download(d_status, A.CEM_STATUS, np.uint32)
        sigma_now = eng.device_download(d_g, (B, H, n), np.float32)
        names = ["sample", "rollout", "update", "loop", "mppi sample", "mppi update", "update K = 1", f"update K = {S}", "update H = 1"]
        bodies = [sample, rollout, update, loop, mppi_sample, mppi_update, lambda: update(spec_1), lambda: update(spec_all), lambda: update(spec_h1)]
        for _ in range(WARM):
            for body in bodies:
                timed(eng, body)
        samples = [[] for _ in bodies]
        for _ in range(ALTERNATIONS):
            for k, body in enumerate(bodies):
                samples[k].append(timed(eng, body))
        med = [float(np.median(x)) for x in samples]
        spread = [float(np.percentile(x, 90) - np.percentile(x, 10)) for x in samples]
        # the host path: what a caller of the library does without these calls
        host_up, host_down = [], []
        gen = np.random.default_rng(7)
        for _ in range(HOST_SAMPLES):
            eng.synchronize()
            t0 = time.perf_counter()
            V = np.clip(U[:, :, None, :] + G[:, :, None, :] * gen.standard_normal((B, H, S, n), dtype=np.float32), np.float32(-0.1), np.float32(0.1))
            V[:, :, 0, :] = U
            eng.device_upload_into(d_v, V)
            eng.synchronize()
            host_up.append((time.perf_counter() - t0) * 1e6)
            rollout()
            eng.synchronize()
            t0 = time.perf_counter()
            c = eng.device_download(d_c, (B, S), np.float32)
            el = np.argpartition(c, K - 1, axis=1)[:, :K]
            picked = np.take_along_axis(V, el[:, None, :, None], axis=2)
            mean = U + np.float32(ALPHA) * (picked.mean(axis=2) - U)
            sig = np.clip(G + np.float32(ALPHA) * (picked.std(axis=2) - G), np.float32(SIGMA_MIN), np.float32(SIGMA_MAX))
            eng.device_upload_into(d_u, np.concatenate([mean[:, 1:], mean[:, -1:]], axis=1).astype(np.float32))
            eng.device_upload_into(d_g, np.concatenate([sig[:, 1:], sig[:, -1:]], axis=1).astype(np.float32))
            eng.set_velocity_command(mean[:, 0].astype(np.float32))
            eng.synchronize()
            host_down.append((time.perf_counter() - t0) * 1e6)
        hu, hd = float(np.median(host_up)), float(np.median(host_down))
        s_us, r_us, u_us, l_us, ms_us, mu_us, u1_us, ua_us, uh_us = med
        elite_bytes = 4 * B * H * K * n
        say(f"{B} robots x {S} samples x {H} steps, {n} cables, K = {K} ({eng.kernel_name}): command batch {nbytes / 1e6:.1f} MB, the elites' rows "
            f"{elite_bytes / 1e6:.1f} MB, {int(status[0])} robots updated, {int(status[1])} degenerate, {int(status[2])} bad costs, {int(status[3])} short, "
            f"sigma after one update {float(sigma_now.min()):.4f} .. {float(sigma_now.max()):.4f}")
        say(f"  sample {s_us:9.2f} us   rollout {r_us:9.2f} us   update {u_us:9.2f} us   the three and the command, back to back {l_us:9.2f} us "
            f"(sum of the parts {s_us + r_us + u_us:9.2f} us)")
        say("  spread (p90 - p10) " + " / ".join(f"{x:6.2f}" for x in spread) + f" us over {ALTERNATIONS} samples of {LOOP} calls ({', '.join(names)})")
        say(f"  (a) host path: normals + clip + upload {hu:11.1f} us   download + argpartition + mean/std + uploads {hd:11.1f} us (wall clock)   "
            f"host / device: {hu / s_us:8.1f} x and {hd / u_us:8.1f} x")
        say(f"  (b) MPPI of the same build: sample {ms_us:9.2f} us (CEM / MPPI {s_us / ms_us:5.2f})   update {mu_us:9.2f} us (CEM / MPPI {u_us / mu_us:5.2f})")
        say(f"  sample writes {nbytes / s_us / 1e6:7.3f} TB/s   update K = 1 {u1_us:9.2f} us   update K = {S} {ua_us:9.2f} us "
            f"({2 * nbytes / ua_us / 1e6:7.3f} TB/s over two passes)")
        if u_us > u1_us:
            say(f"  rows of {4 * n} bytes gathered for K = {K}: {4 * B * H * (K - 1) * n / 1e6:.1f} MB in the {u_us - u1_us:.2f} us past K = 1: "
                f"{4 * B * H * (K - 1) * n / (u_us - u1_us) / 1e6:7.3f} TB/s")
        if u_us < mu_us:
            say(f"  the update beats the MPPI update it reads {K / S:.2f} as much as: {u_us:.2f} us against {mu_us:.2f} us")
        else:
            rounds = -(-H // 4)
            say(f"  the update does NOT beat the MPPI update ({u_us:.2f} us against {mu_us:.2f} us).  Not the bytes: K = 1 takes {u1_us:.2f} us.  With H = 1 "
                f"(memset, launch, the selection's 33 counting passes with a barrier each, the placement pass, one round of the fit) it takes {uh_us:.2f} us; "
                f"the other {rounds - 1} rounds of the fit take {u_us - uh_us:.2f} us, {(u_us - uh_us) / max(rounds - 1, 1):.2f} us a round: a wave goes through "
                f"its steps one after the other - list, one row load in flight, two butterflies of {n} sums, under SHIFT a barrier - with {min(K, 64)} of 64 lanes at work")
        eng.synchronize()
        for d in (d_u, d_g, d_ref, d_v, d_c, d_action, d_e, d_best, d_status, d_mu, d_w, d_ess, d_mstatus):
            eng.device_free(d)
        eng.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
