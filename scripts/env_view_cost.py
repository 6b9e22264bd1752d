"""What the environment view costs (cdpr_observe_device, cdpr_env_evaluate_device) next to the done verdict it contains, to the three
launches it stands for and to the host path it replaces: per_robot_commands handles at 65 536 x 8 (FK + TD) and 4 096 x 4.

The spec: every field the handle serves, all six weights (five without FK), the rule of scripts/done_cost.py.  By HIP events on the
engine's stream, LOOP calls per sample, ALTERNATIONS samples of each form taken in turn after a warm-up, medians:
  observe          observe_device, all fields
  full             env_evaluate_device: observation, reward, mask, reason, counts
  no counts        the same without d_counts: nothing is zeroed in front of the kernel, no atomics
  verdict          env_evaluate_device(d_mask, d_reason, d_counts)
  mask only        env_evaluate_device(d_mask): the work of evaluate_done_device(d_mask)
  reward only      env_evaluate_device(d_reward)          three launches = verdict + observe + reward only, what `full` stands for
  done             evaluate_done_device(d_mask) of this library
  step             update(1)
`done` is also taken from the parent commit's library (cdpr-simulation_amd/libcdpr_hip_parent.so, which __graft_entry__.build() makes) in
the same session: child processes of this script, parent and own library in turn, twice each - their run-to-run spread is what "mask
only" is compared with.  Beside them, by the wall clock, the host path: observables() + raw_state() + the reward in numpy.  Bytes: what
each form has to move per robot (rows read once, outputs written once) and the rate that makes, beside the 6.29 TB/s a float4 copy
reaches on this part.  Usage: env_view_cost.py [out.txt]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

LOOP, ALTERNATIONS = 10, 300
SHAPES = ((65536, 8, 3), (4096, 4, 0))  # batch, cables, stages
PARENT = "libcdpr_hip_parent.so"
COPY_CEILING = 6.29e12  # B/s, float4 copy


def timed(eng, body):
    eng.profile_begin()
    for _ in range(LOOP):
        body()
    return eng.profile_end()[0] * 1e3 / LOOP  # us per iteration


def measure(eng, bodies):
    for _ in range(20):  # warm-up
        for body in bodies.values():
            timed(eng, body)
    samples = {k: [] for k in bodies}
    for _ in range(ALTERNATIONS):
        for k, body in bodies.items():
            samples[k].append(timed(eng, body))
    return {k: float(np.median(v)) for k, v in samples.items()}


def start(pkg, B, N, stages):
    import bench
    from cdpr_simulation_amd import _abi

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
    return eng, model, pose, rule


def done_only():
    """child mode: evaluate_done_device(d_mask) of the library CDPR_LIB names, one JSON line"""
    import cdpr_simulation_amd as pkg

    out = {}
    for B, N, stages in SHAPES:
        eng, _, _, rule = start(pkg, B, N, stages)
        rule_s, d_mask = rule.to_struct(), eng.device_alloc(B)
        out[f"{B}x{N}"] = measure(eng, {"done": lambda: eng.evaluate_done_device(rule_s, d_mask)})["done"]
        eng.synchronize()
        eng.device_free(d_mask)
        eng.close()
    print(json.dumps(out), flush=True)


def child(lib):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--done-only"], env=dict(os.environ, CDPR_LIB=lib), capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"{lib}: {r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def bytes_per_robot(n, fk, width, obs, reward, verdict):
    groups = (n + 3) // 4
    read = 4 * 16 + 16 + 4  # state slots 0-3, observable slot 3, the episode clock
    if obs:
        read += 3 * groups * 16 + (16 if fk else 0)
    elif reward:
        read += groups * 16  # the effort slots
    if reward:
        read += 28  # the target row
    return read + (4 * width if obs else 0) + (4 if reward else 0) + (1 + 4 if verdict else 0)


def numpy_reward(spec, pose, twist, effort, target):
    e = pose[:, :3] - target[:, :3]
    c = (pose[:, 3:] * target[:, 3:]).sum(axis=1)
    ori = 1.0 - c * c / ((pose[:, 3:] ** 2).sum(axis=1) * (target[:, 3:] ** 2).sum(axis=1))
    return (spec.alive - spec.w_position * (e * e).sum(axis=1) - spec.w_orientation * ori - spec.w_speed * (twist[:, :3] ** 2).sum(axis=1)
            - spec.w_rate * (twist[:, 3:] ** 2).sum(axis=1) - spec.w_effort * (effort ** 2).sum(axis=1))


def main():
    import cdpr_simulation_amd as pkg
    from cdpr_simulation_amd import _abi

    lines = []
    have_parent = os.path.exists(os.path.join(ROOT, "cdpr-simulation_amd", PARENT))
    runs = [(lib, child(lib)) for lib in (PARENT, "libcdpr_hip.so") * 2] if have_parent else []
    for B, N, stages in SHAPES:
        eng, model, pose, rule = start(pkg, B, N, stages)
        fields = _abi.OBS_ALL if stages & 1 else _abi.OBS_ALL & ~_abi.OBS_NEED_FK
        width = eng.observation_width(fields)
        spec = pkg.EnvSpec(done=rule, fields=fields, w_position=40.0, w_orientation=3.0, w_speed=0.5, w_rate=0.25, w_effort=0.002, w_fk_residual=7.0 if stages & 1 else 0.0,
                           alive=1.0, done_penalty=5.0)
        rule_s = rule.to_struct()
        target = np.ascontiguousarray(pose, dtype=np.float32)
        d_target, d_obs, d_reward = eng.device_upload(target), eng.device_alloc(4 * B * width), eng.device_alloc(4 * B)
        d_mask, d_reason, d_counts = eng.device_alloc(B), eng.device_alloc(4 * B), eng.device_alloc(4 * _abi.DONE_COUNTS)
        med = measure(eng, {
            "observe": lambda: eng.observe_device(fields, d_obs),
            "full": lambda: eng.env_evaluate_device(spec, d_target, d_obs, d_reward, d_mask, d_reason, d_counts),
            "no counts": lambda: eng.env_evaluate_device(spec, d_target, d_obs, d_reward, d_mask, d_reason),
            "verdict": lambda: eng.env_evaluate_device(spec, 0, 0, 0, d_mask, d_reason, d_counts),
            "mask only": lambda: eng.env_evaluate_device(spec, 0, 0, 0, d_mask),
            "reward only": lambda: eng.env_evaluate_device(spec, d_target, 0, d_reward),
            "done": lambda: eng.evaluate_done_device(rule_s, d_mask),
            "step": lambda: eng.update(1),
        })
        three = med["verdict"] + med["observe"] + med["reward only"]
        counts = eng.evaluate_done(rule)[2]
        moved = {"observe": bytes_per_robot(N, stages & 1, width, True, False, False), "full": bytes_per_robot(N, stages & 1, width, True, True, True),
                 "no counts": bytes_per_robot(N, stages & 1, width, True, True, True), "verdict": bytes_per_robot(N, stages & 1, width, False, False, True),
                 "mask only": bytes_per_robot(N, stages & 1, width, False, False, True) - 4, "reward only": bytes_per_robot(N, stages & 1, width, False, True, False)}
        lines.append(f"{B} x {N}, stages {stages}: {eng.kernel_name}; observation width {width}; {int(counts[0])} robots done per call")
        for k, label in (("observe", "observe_device, all fields"), ("full", "env_evaluate_device, everything"), ("no counts", "env_evaluate_device, no counts"),
                         ("verdict", "env_evaluate_device, verdict"), ("mask only", "env_evaluate_device, mask only"),
                         ("reward only", "env_evaluate_device, reward only")):
            rate = moved[k] * B / (med[k] * 1e-6)
            lines.append(f"  {label:34s}{med[k]:8.2f} us per call; {moved[k]:4d} B per robot, {rate / 1e9:8.1f} GB/s ({rate / COPY_CEILING:5.1%} of the 6.29 TB/s copy ceiling)")
        lines.append(f"  evaluate_done_device(mask), this library  {med['done']:8.2f} us per call")
        lines.append(f"  update(1)                                 {med['step']:8.2f} us per step")
        lines.append(f"  three launches (verdict + observe + reward only) {three:8.2f} us against {med['full']:.2f} us for the one launch ({med['full'] / three:5.1%})")
        if runs:
            key = f"{B}x{N}"
            lines.append("  evaluate_done_device(mask) in child processes, in turn: " + ", ".join(f"{'parent' if lib == PARENT else 'own'} {r[key]:.2f}" for lib, r in runs) + " us")
            parents = [r[key] for lib, r in runs if lib == PARENT]
            lines.append(f"  the parent's run-to-run spread {min(parents):.2f} .. {max(parents):.2f} us; mask only {med['mask only']:.2f} us")
        else:
            lines.append(f"  ({PARENT} not built: no comparison with the parent commit's evaluate_done_device)")
        old = []
        for _ in range(20):
            eng.synchronize()
            t0 = time.perf_counter()
            _, _, effort, _, _ = eng.observables()
            p, t = eng.raw_state()
            numpy_reward(spec, p, t, effort, target)
            old.append((time.perf_counter() - t0) * 1e6)
        lines.append(f"  host path (observables, raw_state, the reward in numpy): {float(np.median(old)):10.1f} us by the wall clock")
        eng.synchronize()
        for x in (d_target, d_obs, d_reward, d_mask, d_reason, d_counts):
            eng.device_free(x)
        eng.close()
    text = "\n".join(lines)
    print(text, flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    done_only() if "--done-only" in sys.argv else main()
