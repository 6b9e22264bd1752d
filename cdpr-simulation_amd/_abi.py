"""ctypes mirror of include/cdpr.h (the C-ABI of libcdpr_hip.so).

Only data definitions live here: the structs and constants of the boundary.  The
loader and the function prototypes are in `_native.py`.
"""
import ctypes as C

ABI_VERSION = 8
MAX_CABLES = 12
MAX_D_BUFFER = 32
MAX_D_DEGREE = 4
COMMAND_VELOCITY, COMMAND_POSITION, COMMAND_FORCE = 0, 1, 2  # cdpr_update_scheduled_kind
MAX_CASCADE = 4
PID_DEBUG_AXES = 9

OK = 0
IGNORED = 1
ERR_INVALID = -1
ERR_DEVICE = -2
ERR_UNSUPPORTED = -3
ERR_NOMEM = -4

STAGE_FK = 0x1
STAGE_TD = 0x2
STAGE_PID_DEBUG = 0x4

# cdpr_done_rule_t.enable / the reason word of cdpr_evaluate_done
DONE_NONFINITE, DONE_WORKSPACE, DONE_TILT, DONE_SPEED, DONE_RATE, DONE_FK_RESIDUAL, DONE_INFEASIBLE, DONE_TRAVEL, DONE_TIMEOUT = (1 << k for k in range(9))
DONE_COUNTS = 16  # counts[0] = robots done, counts[1 + k] = robots with reason bit k

# cdpr_env_spec_t.fields / cdpr_observe_device: the columns of the observation tensor, in bit order (n = cables)
OBS_POSE, OBS_TWIST, OBS_JOINT_POSITION, OBS_JOINT_VELOCITY, OBS_EFFORT, OBS_FK_POSE, OBS_FK_RESIDUAL, OBS_AGE = (1 << k for k in range(8))
OBS_ALL = 0xFF
OBS_NEED_FK = OBS_FK_POSE | OBS_FK_RESIDUAL  # fields only a STAGE_FK handle serves

PLAN_FIRST_WORLD_STEP, PLAN_SCHEDULED, PLAN_ROLLOUT, PLAN_NOT_STEADY = 1, 2, 4, 8  # cdpr_plan_kernel flags
MAP_AUTO = 0
MAP_LANE_PER_ROBOT = 1
MAP_LANE_PAIR = 2
MAP_LANE_PER_CABLE = 3


class FilterParams(C.Structure):
    _fields_ = [("rel_cutoff", C.c_double), ("quality", C.c_double), ("cascade", C.c_uint32), ("reserved_", C.c_uint32)]


class PidParams(C.Structure):
    _fields_ = [
        ("forward_gain", C.c_double),
        ("p_gain", C.c_double),
        ("i_gain", C.c_double),
        ("d_gain", C.c_double),
        ("d_degree", C.c_uint32),
        ("d_buffer_length", C.c_uint32),
        ("i_limit", C.c_double),
        ("cmd_limit", C.c_double),
        ("p_filter", FilterParams),
        ("d_filter", FilterParams),
    ]


class ConfigStruct(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("n_cables", C.c_uint32),
        ("batch", C.c_uint64),
        ("dt", C.c_double),
        ("frame_anchor", (C.c_double * 3) * MAX_CABLES),
        ("platform_anchor", (C.c_double * 3) * MAX_CABLES),
        ("cable_ref_length", C.c_double * MAX_CABLES),
        ("home_pose", C.c_double * 7),
        ("mass", C.c_double),
        ("inertia", C.c_double * 6),
        ("gravity", C.c_double * 3),
        ("joint_damping", C.c_double),
        ("effort_limit", C.c_double),
        ("velocity_limit", C.c_double),
        ("unilateral_cables", C.c_uint32),
        ("precision", C.c_uint32),
        ("velocity_pid", PidParams),
        ("position_pid", PidParams),
        ("velocity_epsilon", C.c_double),
        ("publish_period", C.c_double),
        ("stages", C.c_uint32),
        ("mapping", C.c_uint32),
        ("fk_max_iterations", C.c_uint32),
        ("per_robot_commands", C.c_uint32),
        ("fk_lambda", C.c_double),
        ("fk_tolerance", C.c_double),
        ("td_f_min", C.c_double),
        ("td_f_max", C.c_double),
        ("passive_damping", C.c_double),
        ("leg_inertia", C.c_double),
        ("cable_axial_mass", C.c_double),
        ("anchor_point_mass", C.c_double),
        ("anchor_inertia", C.c_double),
        ("travel_lower", C.c_double),
        ("travel_upper", C.c_double),
        ("travel_stop", C.c_uint32),
        ("reserved3_", C.c_uint32),
    ]


class DoneRuleStruct(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("enable", C.c_uint32),
        ("pos_lo", C.c_float * 3),
        ("pos_hi", C.c_float * 3),
        ("min_up", C.c_float),
        ("max_speed", C.c_float),
        ("max_rate", C.c_float),
        ("max_fk_residual", C.c_float),
        ("max_steps", C.c_uint32),
        ("reserved_", C.c_uint32),
    ]


class EnvSpec(C.Structure):
    """cdpr_env_spec_t: what Engine.env_evaluate[_device] computes.  fields: OBS_* bits of the observation tensor, ld: floats per row of
    it (0 = packed); the reward's weights, `alive` and `done_penalty` (float32); `done`: the rule of the verdict (a DoneRuleStruct, or
    anything with to_struct() such as config.DoneRule).  struct_size is filled in."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("fields", C.c_uint32),
        ("ld", C.c_uint32),
        ("reserved_", C.c_uint32),
        ("w_position", C.c_float),
        ("w_orientation", C.c_float),
        ("w_speed", C.c_float),
        ("w_rate", C.c_float),
        ("w_effort", C.c_float),
        ("w_fk_residual", C.c_float),
        ("alive", C.c_float),
        ("done_penalty", C.c_float),
        ("done", DoneRuleStruct),
    ]
    WEIGHTS = ("w_position", "w_orientation", "w_speed", "w_rate", "w_effort", "w_fk_residual")  # the order the reward applies them in

    def __init__(self, done=None, **kw):
        super().__init__(**kw)
        self.struct_size = C.sizeof(EnvSpec)
        rule = done.to_struct() if hasattr(done, "to_struct") else done
        if rule is None:
            rule = DoneRuleStruct()
            rule.struct_size = C.sizeof(DoneRuleStruct)
        self.done = rule


RESAMPLE_STATUS = 5  # cdpr_resample_*_device's d_status: [robots copied, destinations skipped, groups resampled, groups degenerate, bad weights]


class ResampleSpec(C.Structure):
    """cdpr_resample_spec_t: what Engine.resample[_map]_device computes.  group_size: robots per group, consecutive (0 = the whole batch);
    ess_gate: a group is resampled iff its effective sample size is below ess_gate * group_size (2 = always, 0 = never).  struct_size
    is filled in."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("group_size", C.c_uint32),
        ("ess_gate", C.c_float),
        ("flags", C.c_uint32),
    ]

    def __init__(self, group_size=0, ess_gate=2.0, flags=0):
        super().__init__(C.sizeof(ResampleSpec), int(group_size), float(ess_gate), int(flags))


MPPI_NOMINAL_FIRST, MPPI_CLAMP, MPPI_SHIFT = 1, 2, 4  # cdpr_mppi_spec_t.flags
MPPI_STATUS = 3  # cdpr_mppi_update_device's d_status: [robots updated, robots degenerate, bad costs]


class MppiSpec(C.Structure):
    """cdpr_mppi_spec_t: what Engine.mppi_sample[_device] and Engine.mppi_update[_device] compute.  samples S and horizon H shape the
    command batch float[B][H][S][n]; sigma scales the noise, cmd_min / cmd_max bound the commands under MPPI_CLAMP, temperature divides
    the cost differences of the update; (seed_lo, seed_hi) is the Philox key and robot_offset the global index of the handle's robot 0
    (a shard of a larger batch).  struct_size is filled in."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("samples", C.c_uint32),
        ("horizon", C.c_uint32),
        ("flags", C.c_uint32),
        ("sigma", C.c_float),
        ("cmd_min", C.c_float),
        ("cmd_max", C.c_float),
        ("temperature", C.c_float),
        ("seed_lo", C.c_uint32),
        ("seed_hi", C.c_uint32),
        ("robot_offset", C.c_uint32),
        ("reserved", C.c_uint32),
    ]

    def __init__(self, samples=1, horizon=1, flags=0, sigma=0.0, cmd_min=0.0, cmd_max=0.0, temperature=1.0, seed=0, robot_offset=0):
        super().__init__(C.sizeof(MppiSpec), int(samples), int(horizon), int(flags), float(sigma), float(cmd_min), float(cmd_max), float(temperature),
                         int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF, int(robot_offset) & 0xFFFFFFFF, 0)

    def with_offset(self, robot_offset):
        """a copy whose robot 0 has the global index robot_offset more (modulo 2^32): the spec of a shard"""
        s = MppiSpec.from_buffer_copy(self)
        s.robot_offset = (self.robot_offset + int(robot_offset)) & 0xFFFFFFFF
        return s


CEM_NOMINAL_FIRST, CEM_CLAMP, CEM_SHIFT = 1, 2, 4  # cdpr_cem_spec_t.flags: the bits of their MPPI namesakes
CEM_STATUS = 4  # cdpr_cem_update_device's d_status: [robots updated, robots degenerate, bad costs, robots short of K usable costs]


class CemSpec(C.Structure):
    """cdpr_cem_spec_t: what Engine.cem_sample[_device] and Engine.cem_update[_device] compute.  samples S and horizon H shape the command
    batch float[B][H][S][n]; the elites are the K best samples of a robot; alpha in (0, 1] blends the fit into the old plans (1: the fit
    itself), sigma' is clamped to [sigma_min, sigma_max] (inf: no upper clamp); cmd_min / cmd_max bound the commands under CEM_CLAMP;
    (seed_lo, seed_hi) is the Philox key and robot_offset the global index of the handle's robot 0 (a shard of a larger batch).
    struct_size is filled in."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("samples", C.c_uint32),
        ("horizon", C.c_uint32),
        ("flags", C.c_uint32),
        ("elites", C.c_uint32),
        ("alpha", C.c_float),
        ("sigma_min", C.c_float),
        ("sigma_max", C.c_float),
        ("cmd_min", C.c_float),
        ("cmd_max", C.c_float),
        ("seed_lo", C.c_uint32),
        ("seed_hi", C.c_uint32),
        ("robot_offset", C.c_uint32),
        ("reserved", C.c_uint32 * 3),
    ]

    def __init__(self, samples=1, horizon=1, flags=0, elites=1, alpha=1.0, sigma_min=0.0, sigma_max=float("inf"), cmd_min=0.0, cmd_max=0.0,
                 seed=0, robot_offset=0):
        super().__init__(C.sizeof(CemSpec), int(samples), int(horizon), int(flags), int(elites), float(alpha), float(sigma_min), float(sigma_max),
                         float(cmd_min), float(cmd_max), int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF, int(robot_offset) & 0xFFFFFFFF)

    def with_offset(self, robot_offset):
        """a copy whose robot 0 has the global index robot_offset more (modulo 2^32): the spec of a shard"""
        s = CemSpec.from_buffer_copy(self)
        s.robot_offset = (self.robot_offset + int(robot_offset)) & 0xFFFFFFFF
        return s
