"""The nine kinds of per-robot handle the tests of the calls over chosen robots run on (reset_robots, copy_robots, the done rules, the
environment view): three per record layout - register-resident per-robot records, the general path's record buffer, the
precision = 64 rows - with the Config that makes each, the environment switches it needs and what kernel_name must then hold.
ALL names those nine; HANDLES holds one more, general_one_wave, for the launch-form tests (tests/launch_forms.py).

B = 130: two full wavefronts and a ragged one, stride 192.
"""
import parity
import robot_histories as ri

B = ri.B
EPS = ri.EPS

# handle kind: (cables, Config arguments, environment switches, what kernel_name must hold)
HANDLES = {
    "fast_n8": (8, dict(stages=3), {}, ("cdpr_split_kernel<8, true>",)),  # the role-split per-robot kernel
    "fast_n4": (4, dict(stages=0), {}, ("cdpr_step_kernel<4,", "PR")),
    "fast_n7": (7, dict(stages=3), {}, ("cdpr_split_kernel<7, true>",)),  # the padding cable and the odd integral row
    "general_n8": (8, dict(stages=3, velocityEpsilon=EPS), {}, ("cdpr_gen_split_kernel<8>",)),
    "general_lean_hot": (8, dict(stages=3, velocityEpsilon=EPS), {"CDPR_GEN_SPLIT": "0", "CDPR_GEN_LEAN": "1"}, ("cdpr_gen_lean_kernel<8>", "hot rows")),
    "general_long": (8, dict(stages=3), {}, ("cdpr_gen_step_kernel<8,", ", 32")),
    "fp64_n8": (8, dict(stages=3, precision=64), {}, ("cdpr_step_kernel_f64<8, PR",)),
    "fp64_hold_n8": (8, dict(stages=3, precision=64, velocityEpsilon=EPS), {}, ("cdpr_step_kernel_f64<8, PR, HOLD = 1",)),
    "fp64_hold_long": (8, dict(stages=3, precision=64, velocityEpsilon=EPS), {}, ("cdpr_step_kernel_f64<8, PR, HOLD = 2, HW = 32",)),
    # the one-wave general kernel on 11-sample windows: the only such handle whose fused launches are several steps per launch
    # (tests/launch_forms.py; not one of ALL)
    "general_one_wave": (8, dict(stages=3, velocityEpsilon=EPS), {"CDPR_GEN_SPLIT": "0", "CDPR_GEN_LEAN": "0"}, ("cdpr_gen_step_kernel<8,",)),
}
ALL = ["fast_n8", "fast_n4", "fast_n7", "general_n8", "general_lean_hot", "general_long", "fp64_n8", "fp64_hold_n8", "fp64_hold_long"]
LAYOUTS = ["fast_n8", "general_lean_hot", "fp64_hold_n8"]  # one handle per record layout


clean_env = parity.clean_env_fixture("CDPR_NO_GRAPH")  # (autouse in every module that imports it)


def config_of(pkg, kind, monkeypatch, per_robot=True, more_stages=0):
    n, kw, env, _ = HANDLES[kind]
    parity.clear_overrides(monkeypatch, ("CDPR_NO_GRAPH",))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kw = dict(kw, stages=kw["stages"] | more_stages)
    cfg = pkg.Config(model=ri.model_of(pkg, n), batch=B, perRobotCommands=per_robot, **kw)
    if kind.endswith("_long"):  # 32-sample derivative windows ...
        for p in (cfg.velocityController, cfg.positionController):
            p.dBufferLength, p.dDegree = 32, 2
    if kind == "general_long":  # ... and a gentle loop through a biquad on the P and the D input of the velocity Pid (cascade_config of tests/test_gpu_general_matrix.py)
        for f in (cfg.velocityController.pFilter, cfg.velocityController.dFilter):
            f.cascade, f.relCutoff, f.quality = 1, 0.05, 0.5
        cfg.velocityController.pGain, cfg.velocityController.iGain, cfg.velocityController.dGain = 4.0, 40.0, 0.01
    return cfg


def named(eng, kind):
    name = eng.kernel_name
    assert all(part in name for part in HANDLES[kind][3]), (kind, name)


def state_of(eng, cfg):
    """raw_state, joint_states and observables (the doubles of a precision = 64 handle)"""
    return parity.state_of(eng, cfg.precision == 64, joint_states=True)
