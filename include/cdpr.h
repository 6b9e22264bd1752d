/*
 * cdpr.h — C-ABI of the MI355X-native batched CDPR step engine (libcdpr_hip.so).
 *
 * This is the drop-in boundary for the per-step hot path of the reference Gazebo
 * plugin `cdpr_gazebo` (balazs-bamer/cdpr-simulation).  The reference has no C ABI
 * of its own (it is a Gazebo ModelPlugin registered by GZ_REGISTER_MODEL_PLUGIN,
 * CdprGazeboPlugin.h:105); every entry point below names the reference interface
 * it replaces so a maintainer can bind it from the plugin shell (see
 * INTEGRATION.md for the C++ stub).  Paths are relative to
 * src/cdpr_gazebo/ in the reference tree:
 *   PLG.h/.cpp = include/cdpr_gazebo/CdprGazeboPlugin.h, src/CdprGazeboPlugin.cpp
 *   JFC.h/.cpp = .../JointForceCalculator.h/.cpp      Pid.h/.cpp, Filter.h likewise
 *
 * Conventions
 *   - plain C, no C++ exceptions cross the boundary; every call returns an int:
 *       0  = CDPR_OK, >0 = accepted-but-ignored (mirrors the reference's silent
 *       drops), <0 = error (text via cdpr_last_error()).
 *   - the caller owns every host buffer passed in or out; the library owns all
 *     device state behind the opaque handle and never retains a caller pointer
 *     after the call returns (PLG.cpp:69,78: messages are copied on receipt).
 *   - batched payloads are robot-major ("leading B dimension"): a Joy.axes of
 *     one robot is float[n]; the batch is float[B][n].
 *   - a handle is bound to one GPU and is not thread-safe (the reference runs
 *     update() and both callbacks on the one physics thread, PLG.cpp:203-204).
 *   - quaternions are x,y,z,w on the wire (PLG.cpp:266-269).
 *   - sign: positive joint position / velocity / force = cable shortening /
 *     tension (prismatic axis = -u, gen_cdpr.py:181, cube.sdf:434).
 */
#ifndef CDPR_H_
#define CDPR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The environment view (cdpr_env_spec_t, cdpr_env_spec_size, cdpr_observation_width, cdpr_observe_device, cdpr_env_evaluate_device) came
 * after 8 as new exports only: no struct or call that existed changed, so the number stays 8.  A caller discovers the feature by those
 * symbols and checks its cdpr_env_spec_t against cdpr_env_spec_size().  So did the fork (cdpr_copy_robots*) and the resampler
 * (cdpr_resample_spec_t, cdpr_resample_spec_size, cdpr_resample_map_device, cdpr_resample_device) and MPPI (cdpr_mppi_spec_t, cdpr_mppi_spec_size, cdpr_mppi_sample_device,
 * cdpr_mppi_update_device) and CEM (cdpr_cem_spec_t, cdpr_cem_spec_size, cdpr_cem_sample_device, cdpr_cem_update_device). */
#define CDPR_ABI_VERSION 8u   /* 8 = 7 + cdpr_done_rule_t, cdpr_evaluate_done, cdpr_evaluate_done_device, cdpr_reset_done_device, cdpr_get_episode_start, cdpr_done_rule_size; 7 = 6 + cdpr_reset_robots, cdpr_reset_robots_device; 6 = 5 + cdpr_plan_kernel, cdpr_kernel_name, CDPR_MAX_CABLES 8 -> 12 (cdpr_config_t's anchor arrays grow); 5 = 4 + cdpr_update_scheduled_kind, cdpr_device_pci_bus_id, cdpr_decode_observables_f64 */
#define CDPR_MAX_CABLES 12u         /* PLG.h:20 fixes 4 (kCableCount); cube.yaml:21-29 is a free-length `points` list: the engine takes 1..12
                                      (9..12: uniform-mode fp32 handles on the lane-per-robot kernels, FK and TD included; see cdpr_create) */
#define CDPR_MAX_D_BUFFER 32u       /* Pid: mDbufferLength                      */
#define CDPR_MAX_D_DEGREE 4u        /* Pid: mDpolynomialDegree                  */
#define CDPR_MAX_CASCADE 4u         /* Pid::CascadeFilter: mCascade             */
#define CDPR_PID_DEBUG_AXES 9u      /* PLG.cpp:194  pidMsg.axes.resize(9)       */

/* return codes */
#define CDPR_OK 0
#define CDPR_IGNORED 1              /* wrong-length command, dropped (PLG.cpp:68-73,77-82) */
#define CDPR_ERR_INVALID (-1)       /* bad argument / bad configuration         */
#define CDPR_ERR_DEVICE (-2)        /* HIP runtime failure                      */
#define CDPR_ERR_UNSUPPORTED (-3)   /* valid request the engine cannot serve    */
#define CDPR_ERR_NOMEM (-4)

/* cdpr_config_t.stages: optional stages added to the always-on IK -> PID -> dynamics loop */
#define CDPR_STAGE_FK 0x1u          /* Newton-Raphson forward kinematics (n >= 6) */
#define CDPR_STAGE_TD 0x2u          /* closed-form tension distribution  (n >= 6) */
#define CDPR_STAGE_PID_DEBUG 0x4u   /* record the `pid` debug topic for cable 0 (PLG.cpp:223-227,233-235) */

/* cdpr_config_t.mapping: how robots are laid onto wavefronts */
#define CDPR_MAP_AUTO 0u
#define CDPR_MAP_LANE_PER_ROBOT 1u  /* one lane owns one robot                                               */
#define CDPR_MAP_LANE_PAIR 2u       /* two adjacent lanes share a robot, half the cables each (n = 4 or 8):   */
                                    /* twice the wavefronts, partial sums meet through a DPP add             */
#define CDPR_MAP_LANE_PER_CABLE 3u  /* one lane owns one cable, 8 (n <= 4: 4) adjacent lanes a robot: the structure matrix */
                                    /* row by row in registers, J^T J / J^T r by DPP reductions inside the group, the 6x6  */
                                    /* solve redundantly in every lane (BASELINE.json's north-star mapping; wins only     */
                                    /* while the batch leaves most SIMDs empty: DESIGN.md section 4)                     */

/* Pid::FilterParameters (Pid.h:64-68) */
typedef struct cdpr_filter_params {
  double rel_cutoff;                /* relCutoff: fc relative to fs = 1 (Pid.cpp:34) */
  double quality;                   /* Q                                               */
  uint32_t cascade;                 /* number of identical biquads in series; 0 = bypass */
  uint32_t reserved_;
} cdpr_filter_params_t;

/* Pid::PidParameters (Pid.h:70-81) */
typedef struct cdpr_pid_params {
  double forward_gain;
  double p_gain;
  double i_gain;
  double d_gain;
  uint32_t d_degree;                /* polynomial degree of the derivative fit */
  uint32_t d_buffer_length;         /* samples in the derivative window        */
  double i_limit;
  double cmd_limit;
  cdpr_filter_params_t p_filter;
  cdpr_filter_params_t d_filter;
} cdpr_pid_params_t;

/*
 * Everything CdprGazeboPlugin::Load reads from the ROS parameter server
 * (PLG.h:32-54, PLG.cpp:57,102-138) plus the model constants Gazebo takes from
 * cube.sdf / cube.yaml (anchors, mass, inertia, damping, effort limit) and the
 * world constants that are Gazebo defaults (dt, gravity).
 */
typedef struct cdpr_config {
  uint32_t abi_version;             /* CDPR_ABI_VERSION */
  uint32_t n_cables;                /* PLG.h:20 cWireCount */
  uint64_t batch;                   /* B independent robots on this handle */
  double dt;                        /* world step, Gazebo default 1e-3 s */

  double frame_anchor[CDPR_MAX_CABLES][3];     /* a_i, frame coords    (cube.yaml:21-29 `frame`)    */
  double platform_anchor[CDPR_MAX_CABLES][3];  /* b_i, platform coords (cube.yaml:21-29 `platform`) */
  double cable_ref_length[CDPR_MAX_CABLES];    /* L0_i = cable length at joint position 0           */
  double home_pose[7];              /* x y z qx qy qz qw (cube.sdf:310); state after create/reset   */

  double mass;                      /* cube.sdf:340 */
  double inertia[6];                /* ixx iyy izz ixy ixz iyz, body frame (cube.sdf:332-339) */
  double gravity[3];                /* frame coords; Gazebo default (0,0,-9.8) */
  double joint_damping;             /* cube.sdf:442 actuated-joint damping */
  double effort_limit;              /* cube.sdf:438; Joint::SetForce clamp; < 0 disables */
  double velocity_limit;            /* cube.sdf:439 (10); Joint::SetForce drops a force that pushes a joint already past
                                       +-limit further out [EXT Gazebo]; <= 0 disables (the contract's reduced model,
                                       and what a zero-initialised struct gets) */
  uint32_t unilateral_cables;       /* 1: a cable cannot push, axial force max(T, 0) ([NEW]; the reference has no slack model) */
  uint32_t precision;               /* 0 or 32: fp32 kernels (what every throughput figure is quoted on).  64: the step in the
                                       reference's own precision (Pid.h, Gazebo/ODE compute in double): one plain fp64 kernel for
                                       handles on the register-resident path (IK, Pid, FK, TD, limits, observables, world step; any steps
                                       per launch; trajectory records, command schedules and per_robot_commands since ABI 5), meant for
                                       one robot / small batches; read it out with the *_f64 getters.  velocity_epsilon >= 0 (the position-hold
                                       branch, JFC.cpp:72-82: both Pids of every cable alive, derivative windows on real stamps) is served in
                                       double too (round 5), with the rest of Pid::update - biquad cascades, cmd_limit = 0 - and with
                                       per_robot_commands (two different derivative windows included).  Round 6: the joint stop
                                       (travel_stop > 0), the lumped legs, derivative windows to 32 samples and cdpr_rollout_velocity* in
                                       double as well; every combination of the controller's and the physics' options is served, nine to
                                       twelve cables where the fp32 kernels serve them */

  cdpr_pid_params_t velocity_pid;   /* PLG.cpp:102-120 */
  cdpr_pid_params_t position_pid;   /* PLG.cpp:123-134 (forward gain and filters are forced to 0 by the facade) */
  double velocity_epsilon;          /* PLG.cpp:137-138, JFC.cpp:72 */
  double publish_period;            /* PLG.cpp:57,237; observables are refreshed when now - prev > period */

  uint32_t stages;                  /* CDPR_STAGE_* */
  uint32_t mapping;                 /* CDPR_MAP_*   */
  uint32_t fk_max_iterations;       /* Newton-Raphson iteration cap */
  uint32_t per_robot_commands;      /* 1: every robot has its own JointForceCalculator mode and Pid call history, as B
                                       independent plugin instances have (PLG.cpp:206-219 runs per model): a Joy may reach
                                       some robots only (cdpr_set_*_command_masked).  Runs on the same register-resident kernels as a uniform handle
                                       (mode and Pid call count per lane), unless the configuration needs the general controller path.
                                       0: a Joy batch always addresses every robot (mode uniform over the batch) */
  double fk_lambda;                 /* Levenberg damping added to the diagonal of J^T J */
  double fk_tolerance;              /* stop when max_i |L*_i - L_i| < tol; 0 = always run the cap */
  double td_f_min;                  /* cube.yaml:9 `min: 5`   */
  double td_f_max;                  /* cube.yaml:9 `effort`   */

  /* What the massless-cable reduction drops of the 22-link SDF model, as lumped first-order terms ([EXT] Gazebo/ODE
   * integrates these bodies and joints; closed forms: DESIGN.md section 1).  All 0 = the contract's reduced model. */
  double passive_damping;           /* damping of EVERY passive revolute joint of a leg: the frame-side universal pair
                                       rev_X / rev_Y and the platform-side spherical triple rev_Xpf / rev_Ypf / rev_Zpf
                                       (cube.sdf:396,425,471,500,515: 0.01) */
  double leg_inertia;               /* inertia of the links that turn with a cable about its frame anchor: virt_X, virt_Y,
                                       the cable link, virt_Ypf (cube.sdf:359-366,...: 4 x 0.001 kg m^2) */
  double cable_axial_mass;          /* mass that slides along the cable axis with the prismatic joint: the cable link
                                       (cube.sdf:368: 0.001 kg) */
  double anchor_point_mass;         /* mass carried at each platform anchor: virt_Xpf, virt_Ypf (cube.sdf:456,485: 2 x 0.001 kg) */
  double anchor_inertia;            /* inertia each leg adds to the platform: virt_Xpf (cube.sdf:448-455: 0.001 kg m^2) */

  /* Travel limits of the prismatic joints (cube.sdf:436-437: <lower>-0.5196</lower> <upper>0.5196</upper>; [EXT]
   * Gazebo/ODE enforces them as joint stops).  lower == upper == 0 (a zero-initialised struct): no limits.  With limits
   * set, every step raises a per-cable flag where the joint position q_i = L0_i - L_i lies outside [lower, upper]
   * (cdpr_get_limit_state).  travel_stop > 0 additionally models the stop itself, inelastically: after the velocity
   * update of the world step, a joint at or beyond a limit that is still moving outward (q_i >= upper and qdot_i > 0, or
   * q_i <= lower and qdot_i < 0) takes the impulse that brings its rate to zero, lambda = qdot_i / (J_i M^-1 J_i^T),
   * twist += M^-1 J_i^T lambda, with M the platform's own mass and inertia; cables in index order, travel_stop sweeps
   * over the cables (projected Gauss-Seidel on the velocity constraints: what ODE's quickstep iterates 50 times [EXT];
   * with several joints on their stops one sweep lets them creep, 4 sweeps hold them to within one step's travel;
   * DESIGN.md section 1). */
  double travel_lower;
  double travel_upper;
  uint32_t travel_stop;             /* 0: flag only; k > 0: k sweeps of the stop (<= 64) */
  uint32_t reserved3_;
} cdpr_config_t;

typedef struct cdpr_engine *cdpr_handle_t;

/* Library-level queries (no GPU needed). */
uint32_t cdpr_abi_version(void);
size_t cdpr_config_size(void);                       /* sizeof(cdpr_config_t) as compiled */
int cdpr_device_count(void);                         /* visible GPUs, 0 if none */
/* PCI address "dddd:bb:dd.f" of HIP ordinal `device` (len >= 13): a multi-process host that also runs another GPU runtime
 * (bench.py: torch.distributed over RCCL) checks with it that both runtimes mean the same GPU by ordinal r. */
int cdpr_device_pci_bus_id(int device, char *out, size_t len);
/* Algorithmic HBM bytes one robot moves per state-step for this configuration
 * (state round trip + command read + observables written); see DESIGN.md. */
size_t cdpr_bytes_per_state_step(const cdpr_config_t *cfg);
/* Least-squares end-point derivative weights for an N-sample, degree-d window
 * on a uniform grid (the closed form of Pid::derive + fitPolynomial,
 * Pid.cpp:193-247): derivative = (1/dt) * sum_j w[j] * e[j], oldest first. */
int cdpr_derivative_weights(uint32_t n, uint32_t degree, double *w);

/* Replaces CdprGazeboPlugin::Load (PLG.cpp:49-65): validates the configuration
 * (invalid cable count -> error, PLG.cpp:167-168), allocates device state for
 * `batch` robots on GPU `device`, puts every robot at home_pose with zero twist
 * and every JointForceCalculator in Position mode with target 0
 * (PLG.cpp:153-157, JFC.cpp:38-51). */
int cdpr_create(const cdpr_config_t *cfg, int device, cdpr_handle_t *out);
void cdpr_destroy(cdpr_handle_t h);
/* World reset: back to the state cdpr_create leaves (JFC.h:69-73 reset()). */
int cdpr_reset(cdpr_handle_t h);
const char *cdpr_last_error(cdpr_handle_t h);       /* h may be NULL: last create error */

/* Overwrite the platform state of every robot: pose7[B][7] (x y z qx qy qz qw),
 * twist6[B][6] (world-frame linear, angular).  Either may be NULL (unchanged).
 * Stands in for spawning the model at a pose (launch file `-x -y -z -R -P -Y`). */
int cdpr_set_platform_state(cdpr_handle_t h, const float *pose7, const float *twist6);

/* Model reset of chosen robots while the batch keeps running (a Monte-Carlo sweep, an RL-style environment batch or an MPC loop
 * re-seeding the instances that diverged): the robots with robot_mask[b] != 0 (uint8[B]) are left exactly as cdpr_create /
 * cdpr_reset leave every robot, at pose7[b] / twist6[b] (float[B][7] / float[B][6]; NULL = home_pose / zero; rows of the other
 * robots are never read) in place of home_pose and zero:
 *   platform   the pose as given (no normalisation, as cdpr_set_platform_state), the twist, the FK seed at the pose;
 *   controller JointForceCalculator::reset() (JFC.h:69-73) plus the state Load leaves (PLG.cpp:153-157): Position mode, position
 *              and velocity target 0, force 0, both Pids reset - integral 0, the next Pid::update is the "first" and returns 0
 *              (Pid.cpp:123-126), derivative windows empty, stamps gone, biquad states 0, mCmd 0 - and mLastPosition 0;
 *   read-outs  the robot's observables show the new pose and zeros elsewhere, as before the first publish; its `pid` debug row,
 *              limit flags, FK residual and iterations and infeasible flag are cleared (precision = 64: in double).
 * Untouched: the world-step counter and the publish clock (time goes on: a model reset, not a world reset), every bit of every
 * other robot, the status word, the caller's bound or scheduled command buffers, and every pending command - one addressed to
 * a reset robot stays pending and is latched at the next cdpr_update onto the reset robot, as a Joy sent right after Load.
 * Stream-ordered: after every update queued so far, before every later one.  Needs cdpr_config_t.per_robot_commands = 1 (any
 * such handle, precision = 64 included: a float pose becomes a double exactly), else CDPR_ERR_UNSUPPORTED - a uniform handle
 * keeps one mode and one Pid call count for the whole batch.  NULL handle or mask: CDPR_ERR_INVALID.
 * cdpr_reset_robots: host arrays, copied before the call returns; the work is queued, the stream is not waited for.
 * cdpr_reset_robots_device: device buffers (a loop that computes its "done" mask on the GPU), nothing copied or synchronised;
 * they must stay valid until the stream has passed the reset.
 * Either form stamps the reset robots' episode clock with the world step of the call (cdpr_get_episode_start, below). */
int cdpr_reset_robots(cdpr_handle_t h, const uint8_t *robot_mask, const float *pose7, const float *twist6);
int cdpr_reset_robots_device(cdpr_handle_t h, const uint8_t *d_robot_mask, const float *d_pose7, const float *d_twist6);

/* Fork robots: robot r continues from where robot s = source[r] is NOW (particle-filter resampling, MPPI / CEM with a stateful plant,
 * population search, restart-from-the-best).  New exports after ABI 8, no struct changes.
 *   the map    int32[B].  Robot r with 0 <= source[r] < B and source[r] != r is a DESTINATION; every other robot - a negative entry or
 *              r itself means "leave me" - is untouched: to the bit, never written, read only as somebody's source.  A source must
 *              itself be untouched (source[s] < 0 or source[s] == s): sources are only read, destinations only written, so one launch
 *              needs no scratch copy.  In-place resampling has this shape (survivors keep their index); one source may feed many.
 *   a copy     after the call every getter returns for r, to the bit, what it returns for s - cdpr_get_raw_state[_f64], the joint-state,
 *              observable, FK, TD, limit and `pid` debug getters, cdpr_get_episode_start, the environment view - and from then on r and
 *              s advance identically for as long as they receive the same commands, through every launch form.  Everything
 *              robot-indexed the handle owns moves: platform, FK estimate, observable image, `pid` row, both Pids' records with
 *              their rings, integrals, stamps and hot rows, mode and call count, the active target / latched command rows, the
 *              episode clock.
 *   untouched  the world-step counter and the publish clock, the status word, caller-bound buffers, and every PENDING command: it is
 *              addressed to an index and is latched onto whoever sits there at the next cdpr_update, exactly as after a reset.
 * Source and destination share the world step, so nothing is rebased: a fork at one instant, not a checkpoint across time.
 * Stream-ordered after every update queued so far, before every later one; no host wait, no step launch: cdpr_kernel_name and
 * cdpr_plan_kernel do not see it.  Needs per_robot_commands = 1 (the handles cdpr_reset_robots_device serves, every record layout,
 * precision = 64 included), else CDPR_ERR_UNSUPPORTED with nothing changed.  NULL handle or map: CDPR_ERR_INVALID.
 * cdpr_copy_robots_device: d_source on the device, nothing copied or synchronised; it must stay valid until the stream has passed
 *   the copy.  A destination whose source is out of range (>= B) or is itself a destination is SKIPPED - left as it was - and counted:
 *   d_status is uint32[2] = [robots copied, destinations skipped], zeroed on the stream in front of the kernel, or NULL (no counting).
 * cdpr_copy_robots: a host map, validated first - any entry the device form would skip returns CDPR_ERR_INVALID with nothing changed -
 *   then copied before the call returns and queued; the stream is not waited for. */
int cdpr_copy_robots_device(cdpr_handle_t h, const int32_t *d_source, uint32_t *d_status);
int cdpr_copy_robots(cdpr_handle_t h, const int32_t *source);

/* Resampling on the device: weights to the map of the fork, no host wait.  Systematic (low-variance) resampling per group of P
 * consecutive robots (G = B / P groups; a particle filter per robot team, MPPI / CEM populations, restart-from-the-best): float
 * weights that live on the GPU - a reward buffer, a policy's output - become the int32 source map cdpr_copy_robots_device takes, and
 * the fused form queues the copy right behind.  New exports after ABI 8, no struct changes.
 *
 * The definition is in integers, so that the result does not depend on the order a parallel scan adds in and a sequential restatement
 * (tests/resample_oracle.py) reproduces map, ess and counts to the bit.  Group g has the weights w[gP .. gP + P) and one random word
 * u_g (uint32):
 *   usable   a weight that is finite and > 0; every other weight counts as 0, and NaN, +-inf and negative ones are counted as BAD.
 *            m = the largest usable weight.  None: the group is DEGENERATE - map entries -1, ess 0, counted.
 *   q_i      (uint64) floor((double)w_i / (double)m * 2^30) for a usable weight, else 0: one IEEE double division, then the power of
 *            two.  The maximum becomes exactly 2^30.  Q = sum q_i, C_i its inclusive prefix sum, C_{-1} = 0 (P <= 65 536: Q <= 2^46,
 *            P * C_i <= 2^62).
 *   ess      q_i^2 = hi_i * 2^30 + lo_i, Shi = sum hi_i, Slo = sum lo_i (exact in uint64 and as doubles);
 *            ess = ((double)Q * (double)Q) / ((double)Shi * 2^30 + (double)Slo), exactly those four double operations, never
 *            contracted.  d_ess[g] = (float)ess.  The group is RESAMPLED iff ess < (double)ess_gate * (double)P; ess <= P, so a gate
 *            of 2 means "always" and 0 "never".  A group that is not resampled has map entries -1.
 *   counts   o = (Q * u_g) >> 32 (the full 96-bit product), positions j * Q + o for j = 0 .. P - 1 against the bounds P * C_i:
 *            c_i = #{ j : P * C_{i-1} <= j * Q + o < P * C_i } = N(P * C_i) - N(P * C_{i-1}), N(x) = 0 for x <= o, else
 *            min(P, (x - o + Q - 1) / Q).  sum c_i = P and |c_i - P * q_i / Q| < 1.
 *   the map  survivors (c_i > 0) keep their index, as the copy's rule demands.  extras_i = max(c_i - 1, 0), dead_i = (c_i == 0),
 *            sum extras = sum dead.  The k-th dead robot in index order takes the k-th extra slot in index order: its source is the
 *            smallest i whose inclusive scan of extras exceeds k, its entry gP + i.  Every other entry is -1: all of d_source[0, B) is
 *            written, the buffer needs no clearing.  Every source is a survivor, so the copy skips nothing.
 * spec: struct_size = sizeof(cdpr_resample_spec_t) (cdpr_resample_spec_size()), group_size P (0: the whole batch), ess_gate, flags 0.
 * d_weights float[B]; d_words uint32[G] or NULL (u_g = 2^31 for every group); d_source int32[B]; d_ess float[G] or NULL; d_status
 * uint32[5] or NULL, zeroed on the stream in front of the kernels: [0] robots copied (the map call: its own count of destinations, the
 * same number), [1] destinations the copy skipped (the map call: 0; the fused call: 0 by construction), [2] groups resampled, [3] groups
 * degenerate, [4] bad weights.  All device buffers; they must stay valid until the stream has passed the call.
 * cdpr_resample_map_device: the map alone.  Any handle - uniform or per-robot, every kernel family, both precisions: it reads no robot
 *   state, the handle supplies B and the stream.  Stream-ordered behind everything queued; copies nothing, waits for nothing.
 * cdpr_resample_device: the map, then cdpr_copy_robots_device on it, back to back.  d_source NULL: a buffer of the handle's own.
 *   Per-robot handles only (per_robot_commands = 1), else CDPR_ERR_UNSUPPORTED.
 * Refusals (a refused call queues nothing): CDPR_ERR_INVALID for a NULL handle, spec or weights, a NULL map (the map call),
 * struct_size != sizeof(cdpr_resample_spec_t), flags != 0, B not a multiple of P, an ess_gate that is NaN or negative;
 * CDPR_ERR_UNSUPPORTED for P > 65 536.  No step launch: cdpr_kernel_name and cdpr_plan_kernel do not see it. */
typedef struct cdpr_resample_spec {
  uint32_t struct_size;  /* sizeof(cdpr_resample_spec_t)                                  */
  uint32_t group_size;   /* P: robots per group, consecutive; 0 = the whole batch         */
  float ess_gate;        /* resample a group iff ess < ess_gate * P                       */
  uint32_t flags;        /* 0                                                             */
} cdpr_resample_spec_t;

size_t cdpr_resample_spec_size(void);                /* sizeof(cdpr_resample_spec_t) as compiled */
int cdpr_resample_map_device(cdpr_handle_t h, const cdpr_resample_spec_t *spec, const float *d_weights, const uint32_t *d_words,
                             int32_t *d_source, float *d_ess, uint32_t *d_status);
int cdpr_resample_device(cdpr_handle_t h, const cdpr_resample_spec_t *spec, const float *d_weights, const uint32_t *d_words,
                         int32_t *d_source, float *d_ess, uint32_t *d_status);

/* MPPI on the device: the two calls around cdpr_rollout_velocity_device that keep a sampling MPC loop on the GPU.  cdpr_mppi_sample_device
 * writes the perturbed command batch float[B][H][S][n] the rollout reads from a nominal plan float[B][H][n]; cdpr_mppi_update_device
 * folds the rollout's costs float[B][S] into the next plan and the action to apply (what cdpr_set_velocity_command_device takes).
 * Neither reads robot state or touches a step kernel; the handle supplies B, n (its cable count) and the stream.  New exports after ABI 8,
 * no struct changes.  tests/mppi_oracle.py restates the definition in numpy.
 *
 * Sample.  Robot b has the global index g = robot_offset + b (modulo 2^32).  Element e = (t * S + s) * n + i of its block of
 * E = H * S * n floats belongs to group j = e >> 2, lane k = e & 3.  The random words are
 *   (x0 .. x3) = Philox4x32-10(counter = (j, g, iteration, 0), key = (seed_lo, seed_hi))
 * with the published constants (multipliers D2511F53, CD9E8D57; key increments 9E3779B9, BB67AE85; one round is
 * c' = (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), then the key moves on).  The normals are Box-Muller in float:
 *   u1 = (float)((x >> 9) + 1) * 2^-23 in (0, 1],  a = (float)(y >> 8) * 2^-23 in [0, 2)  (both exact),  r = sqrtf(-2 * logf(u1)),
 *   (z0, z1) = r * (cos pi a, sin pi a) from (x0, x1) with one sincospif, (z2, z3) likewise from (x2, x3);  |z| <= 5.65.
 * The command is v = fmaf(sigma, z_k, U[b][t][i]); with CDPR_MPPI_CLAMP then v = fminf(fmaxf(v, cmd_min), cmd_max) (a NaN becomes
 * cmd_min); with CDPR_MPPI_NOMINAL_FIRST sample s = 0 is the (clamped) nominal without noise.  Only d_commands[0, B * E) is written.  A
 * robot's stream depends on (g, iteration, key) and on nothing else: a shard with robot_offset reproduces its rows of the unsharded batch.
 *
 * Update, per robot.  A cost is usable iff it is finite; any other has weight 0 and is counted BAD.  No usable cost: the robot is
 * DEGENERATE and counted - U' is the old nominal, the weights are 0, ess is 0.  Otherwise c_min is the least usable cost and
 *   w_s = expf((c_min - c_s) / temperature)   (one float subtraction, one float division),   eta = sum w_s,   ess = eta^2 / sum w_s^2,
 *   U'[t][i] = (sum_s w_s * V[t][s][i]) / eta.
 * A sample whose weight is exactly 0 is selected out, not multiplied: a NaN command behind it does not reach the plan (the rule of the
 * environment view's zero reward weights).  Sums are float, in a fixed order: the same inputs give the same bits on every run; against
 * the definition evaluated in double the results agree within the rounding bounds tests/mppi_oracle.py derives.
 * d_action[b][i] = U'[0][i].  The plan written to d_nominal is U'; with CDPR_MPPI_SHIFT it is out[t] = U'[t + 1], the last row repeated
 * (receding horizon).  In place: a robot's rows are all read before any of them is written.
 * d_weights float[B][S], d_ess float[B], d_action float[B][n], d_status uint32[3] = [robots updated, robots degenerate, bad costs] (zeroed on
 * the stream in front of the kernel): each may be NULL.  All device buffers; they must stay valid until the stream has passed the call.
 *
 * Both calls: any handle - uniform or per-robot, every kernel family, both precisions.  Stream-ordered behind everything queued; they
 * copy nothing and wait for nothing.  Not step launches: cdpr_kernel_name, cdpr_plan_kernel and the launch counter do not see them.
 * Refusals (a refused call queues nothing): CDPR_ERR_INVALID for a NULL handle, a NULL spec, a NULL required buffer (sample: d_nominal,
 * d_commands; update: d_cost, d_commands, d_nominal), struct_size != sizeof(cdpr_mppi_spec_t), an unknown flag bit, reserved != 0,
 * samples == 0, horizon == 0, a sigma that is negative or not finite, a temperature that is not finite or not > 0 (the update),
 * CDPR_MPPI_CLAMP with bounds that are not finite or with cmd_min > cmd_max;
 * CDPR_ERR_UNSUPPORTED for E > 2^34, B * S > 2^30 (the rollout's own limit). */
#define CDPR_MPPI_NOMINAL_FIRST 1u   /* sample 0 of every robot is the (clamped) nominal itself          */
#define CDPR_MPPI_CLAMP         2u   /* commands clamped to [cmd_min, cmd_max] (finite, cmd_min <= cmd_max) */
#define CDPR_MPPI_SHIFT         4u   /* update: the plan moves one step towards now (receding horizon)    */

typedef struct cdpr_mppi_spec {
  uint32_t struct_size, samples /*S*/, horizon /*H*/, flags;
  float sigma, cmd_min, cmd_max, temperature;
  uint32_t seed_lo, seed_hi;       /* Philox key                                      */
  uint32_t robot_offset;           /* global index of the handle's robot 0 (shards)   */
  uint32_t reserved;               /* 0                                               */
} cdpr_mppi_spec_t;

size_t cdpr_mppi_spec_size(void);                    /* sizeof(cdpr_mppi_spec_t) as compiled */
int cdpr_mppi_sample_device(cdpr_handle_t h, const cdpr_mppi_spec_t *spec, uint32_t iteration,
                            const float *d_nominal /*[B][H][n]*/, float *d_commands /*[B][H][S][n]*/);
int cdpr_mppi_update_device(cdpr_handle_t h, const cdpr_mppi_spec_t *spec, const float *d_cost /*[B][S]*/,
                            const float *d_commands, float *d_nominal /*in/out*/, float *d_action /*[B][n] or NULL*/,
                            float *d_weights /*[B][S] or NULL*/, float *d_ess /*[B] or NULL*/, uint32_t *d_status /*[3] or NULL*/);

/* CEM on the device: the cross-entropy method in MPPI's place around cdpr_rollout_velocity_device.  cdpr_cem_sample_device writes the
 * command batch float[B][H][S][n] from a mean plan and a sigma plan, float[B][H][n] each (a standard deviation per horizon step and
 * cable); cdpr_cem_update_device picks every robot's K best samples by the rollout's costs float[B][S] and refits both plans to them.
 * No temperature: only the order of the costs counts.  Neither reads robot state or touches a step kernel; the handle supplies B, n and
 * the stream.  New exports after ABI 8, no struct changes.  tests/cem_oracle.py restates the definition in numpy.
 *
 * Sample.  cdpr_mppi_sample_device's definition word for word - the same Philox4x32-10 counter (e >> 2, robot_offset + b, iteration, 0)
 * under the key (seed_lo, seed_hi), the same Box-Muller, the same element order e = (t * S + s) * n + i, the same clamp, the same
 * CDPR_CEM_NOMINAL_FIRST (sample 0 is the clamped mean), only d_commands[0, B * E) written - with one change: the command is
 *   v = fmaf(sigma[b][t][i], z, mean[b][t][i]).
 * A sigma entry is used as it is: 0 gives the mean to the bit, a NaN a NaN in front of the clamp.  The streams being the same, a sigma
 * plan filled with one value gives bit for bit the batch cdpr_mppi_sample_device writes for that spec.sigma under the same key,
 * iteration and offset.
 *
 * Update, per robot.  A cost is usable iff it is finite; the others are counted BAD.  The usable costs are ordered by value, -0 equal
 * to +0, equal values by sample index, lower first.  With M usable costs the elites are the first K' = min(K, M) of that order
 * (K = spec.elites).  M = 0: the robot is DEGENERATE and counted - both plans stay (moved one row on under CDPR_CEM_SHIFT), d_elite is 0,
 * d_best is -1, d_action the old mean's first row.  0 < M < K: the robot is counted SHORT (and updated).  The fit, for every (t, i) over
 * the elites' commands V[t][s][i]:
 *   m = (sum v) / K',   d = v - m (one float subtraction against the float m as computed),   var = (sum d * d) / K',   f = sqrtf(var)
 * (the population variance in two passes; K' as a float).  Sums are float in a fixed order: S <= 4096: lane l of 64 adds the elites
 * of rank l, l + 64, .. (ranks by ascending sample index) in that order, d * d by fmaf; S > 4096: lane l adds the elites among the
 * samples l, l + 64, .. in that order; then a xor butterfly over the 64 lanes (distances 32, 16, .. 1) either way.  The same inputs
 * give the same bits on every run; against the definition in double the results agree within the bounds tests/cem_oracle.py derives.
 * The commands of a sample that is no elite are not read: a NaN behind one does not reach a plan.  An elite's NaN does.
 * Smoothing against the old plans:
 *   mean' = fmaf(alpha, m - mean, mean),   sigma' = fminf(fmaxf(fmaf(alpha, f - sigma, sigma), sigma_min), sigma_max);
 * alpha == 1 selects m and f themselves (selected, not multiplied: a NaN in the old plan is then harmless; sigma' is still clamped).
 * d_action[b][i] = mean'[0][i].  d_elite[b][s] = 1.0f for an elite, else 0.0f.  d_best[b] = the first sample of the order.  The plans
 * written are mean' and sigma'; with CDPR_CEM_SHIFT out[t] = plan'[t + 1], the last row repeated.  In place: every row of a robot's
 * d_mean and d_sigma is read before it is written, also where under CDPR_CEM_SHIFT another row's blend is stored over it.
 * d_action float[B][n], d_elite float[B][S], d_best int32[B], d_status uint32[4] = [robots updated, robots degenerate, bad costs, robots
 * short] (zeroed on the stream in front of the kernel): each may be NULL.  All device buffers; they must stay valid until the stream
 * has passed the call.
 *
 * Both calls: any handle - uniform or per-robot, every kernel family, both precisions, 1 .. 12 cables.  Stream-ordered behind
 * everything queued; they copy nothing and wait for nothing.  Not step launches: cdpr_kernel_name, cdpr_plan_kernel and the launch
 * counter do not see them.  Both calls check the whole spec.
 * CEM refusals (a refused call queues nothing): CDPR_ERR_INVALID for a NULL handle, a NULL spec, a NULL required buffer (sample: d_mean,
 * d_sigma, d_commands; update: d_cost, d_commands, d_mean, d_sigma), struct_size != sizeof(cdpr_cem_spec_t), an unknown flag bit,
 * a reserved word != 0, samples == 0, horizon == 0, elites == 0, elites > samples, an alpha that is not in (0, 1] or not finite,
 * a sigma_min that is negative or not finite or greater than sigma_max, a sigma_max that is NaN (+inf is allowed: no upper clamp),
 * CDPR_CEM_CLAMP with bounds that are not finite or with cmd_min > cmd_max;
 * CDPR_ERR_UNSUPPORTED for E > 2^34, B * S > 2^30 (the rollout's own limit). */
#define CDPR_CEM_NOMINAL_FIRST 1u    /* sample 0 of every robot is the (clamped) mean itself              */
#define CDPR_CEM_CLAMP         2u    /* commands clamped to [cmd_min, cmd_max] (finite, cmd_min <= cmd_max) */
#define CDPR_CEM_SHIFT         4u    /* update: both plans move one step towards now (receding horizon)   */

typedef struct cdpr_cem_spec {
  uint32_t struct_size, samples /*S*/, horizon /*H*/, flags;
  uint32_t elites;                 /* K: 1 .. S                                       */
  float alpha;                     /* smoothing, (0, 1]; 1 = the fit itself           */
  float sigma_min, sigma_max;      /* sigma' clamped to [sigma_min, sigma_max]        */
  float cmd_min, cmd_max;
  uint32_t seed_lo, seed_hi;       /* Philox key                                      */
  uint32_t robot_offset;           /* global index of the handle's robot 0 (shards)   */
  uint32_t reserved[3];            /* 0                                               */
} cdpr_cem_spec_t;

size_t cdpr_cem_spec_size(void);                     /* sizeof(cdpr_cem_spec_t) as compiled */
int cdpr_cem_sample_device(cdpr_handle_t h, const cdpr_cem_spec_t *spec, uint32_t iteration, const float *d_mean /*[B][H][n]*/,
                           const float *d_sigma /*[B][H][n]*/, float *d_commands /*[B][H][S][n]*/);
int cdpr_cem_update_device(cdpr_handle_t h, const cdpr_cem_spec_t *spec, const float *d_cost /*[B][S]*/, const float *d_commands,
                           float *d_mean /*in/out*/, float *d_sigma /*in/out*/, float *d_action /*[B][n] or NULL*/,
                           float *d_elite /*[B][S] or NULL*/, int32_t *d_best /*[B] or NULL*/, uint32_t *d_status /*[4] or NULL*/);

/* Done rules: which robots a loop should put back, decided on the device.  cdpr_reset_robots_device takes a "done" mask that lives
 * on the GPU; these calls compute it there, from the state the handle already holds, so that a Monte-Carlo sweep, an RL-style
 * environment batch or an MPC loop never brings the state to the host to find out who has diverged.
 *
 * The verdict is a pure function of what the getters return at that point of the stream: cdpr_get_raw_state[_f64] (pose and twist:
 * the CURRENT state, not decimated by publish_period), cdpr_get_fk_state (residual), cdpr_get_td_state (infeasible),
 * cdpr_get_limit_state, cdpr_get_episode_start and cdpr_step_count.  The residual and the two flags travel with the observables: they
 * are those of the last PUBLISHED step, zero before the first publish and after a model reset.  That is the whole specification.
 *   reason[b]  the OR of the rule's enabled CDPR_DONE_* bits whose condition holds for robot b; every comparison is an ordinary one
 *              (false on NaN), only CDPR_DONE_NONFINITE reports a NaN.  On precision = 64 handles the rule's floats are promoted to
 *              double and compared with the double rows (the residual as cdpr_get_fk_state rounds it: it has no double getter).
 *   mask[b]    reason[b] != 0, written as exactly 0 or 1: what cdpr_reset_robots_device takes.
 *   counts     uint32[CDPR_DONE_COUNTS]: counts[0] = robots done, counts[1 + k] = robots with reason bit k.  Zeroed on the stream in
 *              front of the kernel: consecutive calls do not accumulate.
 * Episode clock: every robot remembers the world step (low 32 bits of cdpr_step_count) of its last model reset - the low word of the
 * origin (0 unless CDPR_STEP_ORIGIN was set, see cdpr_step_count) after cdpr_create and cdpr_reset, the step count at the call after cdpr_reset_robots[_device] / cdpr_reset_done_device took it; uniform handles keep
 * that first value.  cdpr_get_episode_start reads it (uint32[B], waits for the stream).  CDPR_DONE_TIMEOUT compares
 * (uint32_t)(step_count - start) >= max_steps, which survives the wrap of the low word.
 * Any handle: uniform or per-robot commands, any kernel family, any cable count, both precisions (only platform and observable rows
 * are read, never a controller record).  These are not step launches: cdpr_kernel_name keeps naming the last step's kernel.
 * cdpr_evaluate_done_device: device buffers, stream-ordered after every update queued so far; nothing is copied back, nothing is
 *   waited for, only rows [0, B) are written.  d_reason and d_counts may be NULL.
 * cdpr_evaluate_done: host arrays through device scratch of the handle's own; one wait, then the copies.  Any output may be NULL.
 * cdpr_reset_done_device: the verdict into a mask of the handle's own, then the launch of cdpr_reset_robots_device on that mask
 *   (d_pose7 / d_twist6 as there: float[B][7] / float[B][6] or NULL = home_pose / zero), with no host wait in between.  Needs
 *   per_robot_commands = 1, as the reset does.  d_counts may be NULL.
 * Refusals: CDPR_ERR_INVALID for a NULL handle, a NULL rule, a NULL mask (device form) or struct_size != sizeof(cdpr_done_rule_t);
 * CDPR_ERR_UNSUPPORTED for CDPR_DONE_FK_RESIDUAL without CDPR_STAGE_FK, CDPR_DONE_INFEASIBLE without CDPR_STAGE_TD, and for
 * cdpr_reset_done_device on a uniform handle.  A refused call queues nothing. */
#define CDPR_DONE_NONFINITE   0x001u  /* any of the 13 pose / twist values is not finite                                   */
#define CDPR_DONE_WORKSPACE   0x002u  /* p[c] < pos_lo[c] or p[c] > pos_hi[c] on some axis (on the bound: inside)          */
#define CDPR_DONE_TILT        0x004u  /* R33 < min_up,  R33 = 1 - 2 (qx^2 + qy^2) / (q . q)                                */
#define CDPR_DONE_SPEED       0x008u  /* v . v > max_speed^2                                                               */
#define CDPR_DONE_RATE        0x010u  /* w . w > max_rate^2                                                                */
#define CDPR_DONE_FK_RESIDUAL 0x020u  /* fk residual > max_fk_residual              (needs CDPR_STAGE_FK)                  */
#define CDPR_DONE_INFEASIBLE  0x040u  /* tension-distribution infeasible flag       (needs CDPR_STAGE_TD)                  */
#define CDPR_DONE_TRAVEL      0x080u  /* any travel-limit bit                                                              */
#define CDPR_DONE_TIMEOUT     0x100u  /* step_count - episode_start >= max_steps                                           */
#define CDPR_DONE_COUNTS 16           /* counts[0] = robots done, counts[1 + k] = robots with reason bit k                 */

typedef struct cdpr_done_rule {
  uint32_t struct_size, enable;       /* sizeof(cdpr_done_rule_t); the CDPR_DONE_* bits this rule may raise */
  float pos_lo[3], pos_hi[3];
  float min_up, max_speed, max_rate, max_fk_residual;
  uint32_t max_steps, reserved_;
} cdpr_done_rule_t;

size_t cdpr_done_rule_size(void);                    /* sizeof(cdpr_done_rule_t) as compiled */
int cdpr_evaluate_done_device(cdpr_handle_t h, const cdpr_done_rule_t *rule, uint8_t *d_mask, uint32_t *d_reason, uint32_t *d_counts);
int cdpr_evaluate_done(cdpr_handle_t h, const cdpr_done_rule_t *rule, uint8_t *mask, uint32_t *reason, uint32_t *counts);
int cdpr_reset_done_device(cdpr_handle_t h, const cdpr_done_rule_t *rule, const float *d_pose7, const float *d_twist6, uint32_t *d_counts);
int cdpr_get_episode_start(cdpr_handle_t h, uint32_t *start);   /* uint32[B] */

/* The environment view: what a policy or a sampler consumes of the batch - the observation tensor, a tracking reward and the done
 * verdict - computed where the state is, written to caller-owned DEVICE buffers, in ONE launch that reads the platform and observable
 * rows once.  With the done rules, the device resets and the device command setters a loop commands, steps, judges, re-seeds and
 * observes the batch without a host wait.  Like the done rules it reads state and observables only: no bit of any robot changes.
 *   observation  d_obs is float[B][ld], robot-major; ld = 0 means the packed width.  The columns are the fields of `fields` in bit order;
 *                column j of robot b is, to the bit, what the named getter returns for that robot at that point of the stream (on
 *                precision = 64 handles what the FLOAT getters return: the double rounded once).  Only rows [0, B) and columns
 *                [0, width) of a row are written: columns width .. ld - 1 are the caller's own (a goal, say).
 *   verdict      d_mask, d_reason, d_counts: exactly what cdpr_evaluate_done_device(h, &spec->done, ...) writes at the same point of the
 *                stream.  Any of the three may be NULL.
 *   reward       d_reward is float[B], computed in the handle's precision T (float; or double, rounded to float at the store) with
 *                explicit fma, p / q / v / w the current pose and twist, p* / t the target's position and quaternion:
 *                  e = p - p*,  pos = fma(e2, e2, fma(e1, e1, e0 e0))
 *                  c = fma(qw, tw, fma(qz, tz, fma(qy, ty, qx tx))),  qq and tt the same chains on q, q and t, t
 *                  ori = 1 - (c c) / (qq tt)       (sin^2 of half the angle between the attitudes; sign-invariant, no normalisation assumed)
 *                  vv = fma(v2, v2, fma(v1, v1, v0 v0)), ww likewise   (as the done rules form them)
 *                  ee = the fma chain of effort_i^2 from cable 0 up    (the effort of the last PUBLISHED step)
 *                  res = the FK residual as the done rules take it     (of the last published step, rounded to float)
 *                  r = alive;  r = fma(-w_k, term_k, r) for position, orientation, speed, rate, effort, residual in this order;
 *                  r = r - done_penalty where this call's reason word is non-zero.
 *                A term whose weight is exactly 0 is skipped, not multiplied: a non-finite value behind an unused weight does not reach
 *                the reward; one behind a used weight propagates.
 *   d_target7    float[B][7] on the device (x y z qx qy qz qw); NULL = home_pose (rounded to float, as such a buffer would hold it) for
 *                every robot.
 * cdpr_observe_device: the observation alone.  d_row_mask is uint8[B] or NULL; where given, only the rows with a non-zero byte are
 *   written - evaluate, cdpr_reset_robots_device(mask), cdpr_observe_device(mask) leaves every done robot's row at its post-reset
 *   observation and every other row untouched.
 * cdpr_env_evaluate_device: observation (d_obs, spec->fields, spec->ld), reward and verdict; any output may be NULL, not all.
 * cdpr_observation_width: the packed width of `fields` on this handle (7, 6, n, n, n, 7, 1, 1 per field).
 * Both calls are stream-ordered after every update queued so far, copy nothing and wait for nothing.  Any handle: uniform or per-robot
 * commands, any kernel family, 1 .. 12 cables, both precisions.  They are not step launches: cdpr_kernel_name and cdpr_plan_kernel do
 * not see them.
 * Refusals (a refused call queues nothing): CDPR_ERR_INVALID for a NULL handle, a NULL spec, struct_size != sizeof(cdpr_env_spec_t),
 * fields == 0 with d_obs given, an unknown field bit, ld non-zero and below the width, every output NULL; CDPR_ERR_UNSUPPORTED for
 * CDPR_OBS_FK_* or w_fk_residual != 0 without CDPR_STAGE_FK and for whatever cdpr_evaluate_done_device refuses of spec->done. */
#define CDPR_OBS_POSE           0x01u  /* 7: current pose,  as cdpr_get_raw_state (not decimated)             */
#define CDPR_OBS_TWIST          0x02u  /* 6: current twist, as cdpr_get_raw_state                             */
#define CDPR_OBS_JOINT_POSITION 0x04u  /* n: as cdpr_get_joint_states (last published step)                   */
#define CDPR_OBS_JOINT_VELOCITY 0x08u  /* n                                                                   */
#define CDPR_OBS_EFFORT         0x10u  /* n                                                                   */
#define CDPR_OBS_FK_POSE        0x20u  /* 7: as cdpr_get_fk_state        (needs CDPR_STAGE_FK)                */
#define CDPR_OBS_FK_RESIDUAL    0x40u  /* 1: as cdpr_get_fk_state        (needs CDPR_STAGE_FK)                */
#define CDPR_OBS_AGE            0x80u  /* 1: (float)(uint32_t)(step_count - episode_start)                    */

typedef struct cdpr_env_spec {
  uint32_t struct_size, fields;        /* sizeof(cdpr_env_spec_t); CDPR_OBS_* bits, columns in bit order      */
  uint32_t ld, reserved_;              /* floats per row of d_obs; 0 = the packed width                       */
  float w_position, w_orientation, w_speed, w_rate, w_effort, w_fk_residual;
  float alive, done_penalty;
  cdpr_done_rule_t done;               /* as cdpr_evaluate_done_device takes it                               */
} cdpr_env_spec_t;

size_t cdpr_env_spec_size(void);                     /* sizeof(cdpr_env_spec_t) as compiled */
int cdpr_observation_width(cdpr_handle_t h, uint32_t fields, uint32_t *width);
int cdpr_observe_device(cdpr_handle_t h, uint32_t fields, uint32_t ld, const uint8_t *d_row_mask, float *d_obs);
int cdpr_env_evaluate_device(cdpr_handle_t h, const cdpr_env_spec_t *spec, const float *d_target7,
                             float *d_obs, float *d_reward, uint8_t *d_mask, uint32_t *d_reason, uint32_t *d_counts);

/* Replaces cableVelocityCommandCallback / cablePositionCommandCallback
 * (PLG.cpp:67-83).  `count` = number of floats in `axes`: n*B (one Joy per
 * robot) or n (one Joy broadcast to every robot).  Any other count returns
 * CDPR_IGNORED and changes nothing.  The command is latched at the next
 * cdpr_update and zero-order-held until replaced (PLG.cpp:206-219).
 * `axes` is host memory; it is copied before the call returns (the caller may
 * reuse it at once) and travels to the device on a copy stream of the handle's
 * own while earlier launches still run: the call does not wait for them. */
int cdpr_set_velocity_command(cdpr_handle_t h, const float *axes, size_t count);
int cdpr_set_position_command(cdpr_handle_t h, const float *axes, size_t count);
/* Same, from a device buffer already resident in HBM (float[B][n]); the batch is copied (device to device). */
int cdpr_set_velocity_command_device(cdpr_handle_t h, const float *d_axes, size_t count);
int cdpr_set_position_command_device(cdpr_handle_t h, const float *d_axes, size_t count);
/* Zero-copy form for command schedules that live in HBM: the caller's device buffer float[B][n] (count = n*B) IS the
 * latched Joy batch from the next cdpr_update on; nothing is copied or synchronised.  The buffer must stay valid and
 * unchanged until another command of the same kind has been latched.  (The one exception to "no caller pointer is
 * retained": that is its point.) */
int cdpr_bind_velocity_command_device(cdpr_handle_t h, const float *d_axes, size_t count);
int cdpr_bind_position_command_device(cdpr_handle_t h, const float *d_axes, size_t count);
/* Per-robot arrival: the Joy batch reaches only the robots with robot_mask[b] != 0 (uint8[B], host); the others keep
 * their target, their mode and their Pid state, exactly as plugin instances that received nothing before this
 * update() (PLG.cpp:206-219 is per model).  axes: float[B][n] (rows of unmasked robots are ignored) or float[n]
 * broadcast to the masked robots.  Needs cdpr_config_t.per_robot_commands = 1, else CDPR_ERR_UNSUPPORTED. */
int cdpr_set_velocity_command_masked(cdpr_handle_t h, const float *axes, size_t count, const uint8_t *robot_mask);
int cdpr_set_position_command_masked(cdpr_handle_t h, const float *axes, size_t count, const uint8_t *robot_mask);

/* Replaces JointForceCalculator::setForce (JFC.h:92-95; UpdateMode::Force, JFC.h:35-42, JFC.cpp:67-70): the joints are
 * driven open loop, force_i = axes[i], held until another command arrives: `mLastPosition = joint position; force =
 * mForce`, no Pid runs.  This is the mode a JointForceCalculator is constructed in (JFC.h:42); the shipped plugin never
 * calls setForce (no topic reaches it), a tension-distribution / MPC caller does.  Same count rules as the two Joy
 * callbacks (n*B or n, anything else CDPR_IGNORED).  Latched at the next cdpr_update AFTER a pending velocity and a
 * pending position command ([NEW] ordering: the reference has no force callback to order against; the last setter
 * wins).  setForce resets no Pid; leaving Force mode through a velocity / position command resets the Pid of the mode
 * entered (JFC.cpp:99-119), as from any other mode.  The optional stages still apply: tension distribution redistributes
 * the commanded forces, SetForce limits clamp them.  _masked needs per_robot_commands = 1. */
int cdpr_set_force_command(cdpr_handle_t h, const float *axes, size_t count);
int cdpr_set_force_command_device(cdpr_handle_t h, const float *d_axes, size_t count);
int cdpr_bind_force_command_device(cdpr_handle_t h, const float *d_axes, size_t count);
int cdpr_set_force_command_masked(cdpr_handle_t h, const float *axes, size_t count, const uint8_t *robot_mask);

/* Replaces nsteps x { CdprGazeboPlugin::update (PLG.cpp:202-246) followed by
 * the Gazebo/ODE world step }.  Asynchronous: returns once the work is queued
 * on the handle's stream. */
int cdpr_update(cdpr_handle_t h, int nsteps);
/* Same loop with `steps_per_launch` world steps fused into each kernel launch
 * (state stays on chip between them; observables still written every step). */
int cdpr_update_fused(cdpr_handle_t h, int nsteps, int steps_per_launch);
/* Trajectory record: like cdpr_update_fused, but the observables of EVERY step are kept instead of each step
 * overwriting the last (what a subscriber with a deep queue would have collected from jointStates / platformPose at
 * publishPeriod 0).  d_record is a caller-owned DEVICE buffer of nsteps observable images
 * (cdpr_observable_image_bytes each); image j belongs to world step first+j.  Step 0 of a fresh handle is not
 * published (PLG.cpp:237), its image is left untouched.  Decode a downloaded image with cdpr_decode_observables. */
int cdpr_observable_image_bytes(cdpr_handle_t h, size_t *bytes);
int cdpr_update_record(cdpr_handle_t h, int nsteps, int steps_per_launch, void *d_record, size_t record_bytes);
int cdpr_decode_observables(cdpr_handle_t h, const void *image, float *position, float *velocity, float *effort,
                            float *pose7, float *twist6);
/* precision = 64 handles: their images hold doubles (cdpr_observable_image_bytes says how many bytes); this decodes without
 * the rounding to float (cdpr_decode_observables works on them too and rounds).  CDPR_ERR_UNSUPPORTED on fp32 handles. */
int cdpr_decode_observables_f64(cdpr_handle_t h, const void *image, double *position, double *velocity, double *effort,
                                double *pose7, double *twist6);
/* A whole command schedule resident in HBM, queued with one call: what
 *   for j: cableVelocityCommandCallback(batch j); refresh_steps x update()
 * does (the reference's 100 Hz / 10 Hz publishers against the 1 kHz world: a Joy every 10 or 100 world steps, PLG.cpp:206-211
 * + sinevelocitytest.cpp:34-48, squarevelocitytest.cpp:20-34, squarepositiontest.cpp:21-35), for callers whose batch is too
 * small for a launch per step to pay (a 4 096 x 4-cable step is 1.4 us of work behind 3-4 us of launch).
 * d_commands: DEVICE buffer float[ceil(nsteps / refresh_steps)][B][n], batch j is latched at world step first + j *
 * refresh_steps.  d_ready: optional DEVICE-visible mailbox uint32[batches]: batch j is taken only once d_ready[j] != 0 (a
 * host or a producer kernel that fills the schedule while the work runs.  A HOST producer should keep the words in pinned host memory
 * mapped to the device and post them by plain stores: a copy enqueued on another stream can be placed on the hardware queue of the
 * launch that is waiting for it and then never completes);
 * NULL = the whole schedule is there.  The wait is bounded (~2^23 polls, a few seconds): a mailbox that never delivers
 * does not hang the GPU - the handle's status word is raised instead and cdpr_synchronize and the getters return
 * CDPR_ERR_DEVICE until cdpr_reset.  d_record: as cdpr_update_record (every step's observable image kept; needs
 * publish_period == 0), or NULL (each published step overwrites the last, as the topic does).
 * Bit-identical to the call sequence above (tested).  Afterwards the last batch stays latched (on uniform-mode handles it
 * is read in place and must stay valid like a bound buffer).  Asynchronous.
 *
 * cdpr_update_scheduled_kind: the same for any command kind - jointVelocities, jointPositions (squarepositiontest) or
 * setForce (JFC.h:92-95; a tension-distribution / MPC caller) - and, on per_robot_commands handles, with one robot mask per
 * batch (d_robot_masks: DEVICE buffer uint8[batches][B], batch j reaches the robots with mask[j][b] != 0; NULL = every
 * robot), i.e. for j: cdpr_set_<kind>_command_masked(batch j, mask j); refresh_steps x update().
 * Every handle type is served.  Uniform-mode handles on the register-resident path with one or two lanes per robot run the
 * schedule in ONE launch (the lanes read batch j themselves; state, windows and integrals stay on chip); the others
 * (general controller path, per-robot modes, precision = 64, one lane per cable) latch batch j from the caller's buffers in
 * place and queue its steps, batch after batch, without a host round trip.  A command of ANOTHER kind that is pending at
 * the call is latched together with batch 0 in update()'s order (velocity, position, force: PLG.cpp:206-219), exactly as
 * the call sequence would. */
#define CDPR_COMMAND_VELOCITY 0u    /* jointVelocities, cableVelocityCommandCallback (PLG.cpp:67-74) */
#define CDPR_COMMAND_POSITION 1u    /* jointPositions, cablePositionCommandCallback (PLG.cpp:76-83)  */
#define CDPR_COMMAND_FORCE 2u       /* JointForceCalculator::setForce (JFC.h:92-95)                   */
int cdpr_update_scheduled(cdpr_handle_t h, int nsteps, int refresh_steps, const float *d_commands, const uint32_t *d_ready,
                          void *d_record, size_t record_bytes);
int cdpr_update_scheduled_kind(cdpr_handle_t h, uint32_t kind, int nsteps, int refresh_steps, const float *d_commands,
                               const uint32_t *d_ready, const uint8_t *d_robot_masks, void *d_record, size_t record_bytes);
/* Waits until everything queued on the handle has completed.  Every wait of the library polls the stream for up to 2 ms
 * before it blocks (a blocked host thread wakes up 15-25 us late, two step kernels; environment CDPR_SYNC_SPIN_US
 * overrides, 0 = always block). */
int cdpr_synchronize(cdpr_handle_t h);
uint32_t cdpr_mapping(cdpr_handle_t h);              /* CDPR_MAP_* actually in use (what CDPR_MAP_AUTO resolved to) */
/* Which kernel serves a launch - the routing CDPR_MAP_AUTO takes, answered WITHOUT a GPU from the configuration alone (a
 * 256-CU part is assumed; the CDPR_* A/B environment overrides are honoured as cdpr_create honours them).  No counterpart
 * in the reference (one robot, one code path: PLG.cpp:202-246); what it replaces is "run it and read the profiler".
 *   steps_per_launch  world steps of the launch (1 = cdpr_update's launches)
 *   flags             CDPR_PLAN_FIRST_WORLD_STEP: the launch starts at world step 0; CDPR_PLAN_SCHEDULED: cdpr_update_scheduled's
 *                     in-launch form; CDPR_PLAN_ROLLOUT: cdpr_rollout_velocity*; CDPR_PLAN_NOT_STEADY: a derivative window still
 *                     filling, Force mode, publish decimation, pid debug topic, travel flags, velocity limit, unilateral cables
 *                     or a mailbox (launches of several steps on lane-pair handles then keep the general kernel)
 * name receives the kernel's name with its template arguments as rocprofv3 prints the family (NUL-terminated, truncated to
 * len).  Returns CDPR_OK, or the code cdpr_create would return for this configuration (name = the reason).
 * cdpr_kernel_name: the same for the LAST step launch a handle made (what really ran). */
#define CDPR_PLAN_FIRST_WORLD_STEP 1u
#define CDPR_PLAN_SCHEDULED 2u
#define CDPR_PLAN_ROLLOUT 4u
#define CDPR_PLAN_NOT_STEADY 8u
int cdpr_plan_kernel(const cdpr_config_t *cfg, int steps_per_launch, uint32_t flags, char *name, size_t len);
int cdpr_kernel_name(cdpr_handle_t h, char *name, size_t len);
/* The world clock.  cdpr_step_count: the absolute world step, a 64-bit count; sim time = count * dt.  It starts at the handle's ORIGIN
 * and returns there on cdpr_reset: 0, or what the environment variable CDPR_STEP_ORIGIN=<unsigned 64-bit decimal> held when cdpr_create
 * ran (read once; tests and A/B runs put a handle late in the clock with it).  The origin is a pure relabelling of the world steps: a
 * handle created at origin S does at step S + k what a handle created at origin 0 does at step k, to the bit; what names the absolute
 * step differs - cdpr_step_count, the episode starts (the low word of the origin after create and cdpr_reset: age 0) - and where in a
 * ring a sample sits.  "The first update since Load" (PLG.cpp:59: it only stores the joint positions) is step_count == origin.
 * How far each path's clock goes (tests/test_gpu_late_clock.py runs every path across 2^24 and, where it crosses, 2^31 and 2^32):
 *   register-resident paths (every fp32 handle off the general path, uniform or per-robot): cross 2^24, 2^31 and 2^32 - the kernels
 *     see the ring slot alone, a 64-bit modulus taken on the host;
 *   precision = 64, with or without the hold branch: cross 2^24, 2^31 and 2^32 - the Pids' stamps are the low word of the count and
 *     every difference of two stamps is taken modulo 2^32;
 *   general controller path (hold branch, cascades, long windows on fp32 handles) and its rollout: cross 2^24; world-step stamps are
 *     int32 there, so a call that would take the count to 2^31 (step_count + nsteps >= 2^31; the rollout: + horizon) returns
 *     CDPR_ERR_UNSUPPORTED ("general controller path: world-step counter would pass 2^31") before it latches a command or queues a
 *     launch - the handle is bit for bit as it was, pending commands stay pending; cdpr_reset makes it step again;
 *   the episode clock, CDPR_DONE_TIMEOUT and CDPR_OBS_AGE: the low word, differences modulo 2^32, across the wrap on every handle. */
uint64_t cdpr_step_count(cdpr_handle_t h);

/* Replaces publishJointStates (PLG.cpp:248-256): sensor_msgs/JointState
 * position / velocity / effort, float[B][n] each, as of the last published
 * step.  Any pointer may be NULL.  Synchronises the stream. */
int cdpr_get_joint_states(cdpr_handle_t h, float *position, float *velocity, float *effort);
/* Replaces publishPlatformState (PLG.cpp:258-280): cdpr_gazebo/PlatformState
 * pose7[B][7] (x y z qx qy qz qw) and twist6[B][6] (linear, angular), relative
 * to the frame link. */
int cdpr_get_platform_state(cdpr_handle_t h, float *pose7, float *twist6);
/* Both messages of one published step in one device round trip: the five arrays of cdpr_get_joint_states and
 * cdpr_get_platform_state (any of them may be NULL), as of the last published step.  What a per-step caller uses
 * (PLG.cpp:236-242 publishes jointStates and platformPose on every step): one gather launch into a pinned host image and
 * a completion word the host spins on, instead of five gather / copy / wait rounds. */
int cdpr_get_observables(cdpr_handle_t h, float *position, float *velocity, float *effort, float *pose7, float *twist6);
/* Handles created with cdpr_config_t.precision = 64: the same read-outs in double (the float getters work too and round).
 * Any pointer may be NULL.  cdpr_get_raw_state_f64 = the current state (not decimated by publish_period);
 * cdpr_set_platform_state_f64 = cdpr_set_platform_state without the rounding to float.  CDPR_ERR_UNSUPPORTED on fp32 handles. */
int cdpr_get_observables_f64(cdpr_handle_t h, double *position, double *velocity, double *effort, double *pose7, double *twist6);
int cdpr_get_raw_state_f64(cdpr_handle_t h, double *pose7, double *twist6);
int cdpr_set_platform_state_f64(cdpr_handle_t h, const double *pose7, const double *twist6);
/* Replaces the `pid` debug topic (PLG.cpp:193-194,223-227,233-235;
 * Pid.cpp:139-142,158-168): axes9[B][9] = P term, I term before clamp, D term,
 * desired, applied force of cable 0, then four unused zeros.  Needs
 * CDPR_STAGE_PID_DEBUG. */
int cdpr_get_pid_debug(cdpr_handle_t h, float *axes9);
/* Forward-kinematics estimator (CDPR_STAGE_FK): pose7[B][7] = the estimate after the last step; residual[B] =
 * max_i |L*_i - L_i(estimate)| and iterations[B] travel with the observables: as of the last PUBLISHED step. */
int cdpr_get_fk_state(cdpr_handle_t h, float *pose7, float *residual, int32_t *iterations);
/* Tension distribution of the last PUBLISHED step (CDPR_STAGE_TD): tension[B][n] = the force applied to the joints
 * (after the bounds and the SetForce limits: the `effort` observable), infeasible[B] = 1 where a bound was active. */
int cdpr_get_td_state(cdpr_handle_t h, float *tension, int32_t *infeasible);
/* Travel limits (cdpr_config_t.travel_lower / travel_upper; cube.sdf:436-437): cable_mask[B], bit i set where joint i's
 * position was outside [lower, upper] at the last PUBLISHED step (travels with the observables).  All zero when the
 * configuration sets no limits. */
int cdpr_get_limit_state(cdpr_handle_t h, uint32_t *cable_mask);
/* Current platform state (not decimated by publish_period), for checkpoints
 * and tests: pose7[B][7], twist6[B][6]. */
int cdpr_get_raw_state(cdpr_handle_t h, float *pose7, float *twist6);

/* MPC fan-out (BASELINE config 5): from every robot's CURRENT state run `samples` hypothetical trajectories of
 * `horizon` world steps, each driven by its own jointVelocities sequence, and return one cost per trajectory,
 * cost[B][samples] = sum over the horizon of |p(t_{k+1}) - ref_position|^2.  d_commands is a DEVICE buffer
 * float[B][horizon][samples][n] (per robot and step, a batch of `samples` Joy.axes); ref_position[B][3] and cost
 * are host buffers.  The handle's state is not modified; trajectories never leave the chip.  Every stage the
 * handle was created with (FK, TD) runs in every step.  Synchronous. */
int cdpr_rollout_velocity(cdpr_handle_t h, int samples, int horizon, const float *d_commands,
                          const float *ref_position, float *cost);
/* The same rollout split for hosts that drive several GPUs from one thread (one handle per GPU): _launch stages
 * ref_position and queues the kernel on the handle's stream and returns at once (no allocation in steady state: the
 * scratch buffers are persistent); _fetch copies cost[B][samples] of the pending rollout back and synchronises.
 * Launch on every handle first, then fetch from each: all GPUs run concurrently. */
int cdpr_rollout_velocity_launch(cdpr_handle_t h, int samples, int horizon, const float *d_commands,
                                 const float *ref_position);
int cdpr_rollout_velocity_fetch(cdpr_handle_t h, float *cost);
/* Fully device-resident form: reference positions float[B][3] and costs float[B][samples] in caller-owned DEVICE
 * buffers; asynchronous on the handle's stream, nothing copied (an MPC loop that keeps its sampler on the GPU). */
int cdpr_rollout_velocity_device(cdpr_handle_t h, int samples, int horizon, const float *d_commands,
                                 const float *d_ref_position, float *d_cost);

/* Device-buffer helpers for hosts that have no GPU runtime of their own (ctypes):
 * allocate / free / fill a caller-owned device buffer on the handle's GPU, e.g. to keep
 * a schedule of Joy batches resident in HBM for cdpr_set_*_command_device. */
int cdpr_device_malloc(cdpr_handle_t h, size_t bytes, void **out);
int cdpr_device_free(cdpr_handle_t h, void *ptr);
int cdpr_device_upload(cdpr_handle_t h, void *dst, const void *src, size_t bytes);
int cdpr_device_download(cdpr_handle_t h, void *dst, const void *src, size_t bytes);

/* Timing of the step kernel on the handle's own stream with HIP events:
 * begin records an event, end records another, synchronises THE STREAM (on return
 * everything queued on the handle has completed, as after cdpr_synchronize), and
 * returns the elapsed milliseconds and the number of step-kernel launches in between. */
int cdpr_profile_begin(cdpr_handle_t h);
int cdpr_profile_end(cdpr_handle_t h, float *elapsed_ms, uint64_t *kernel_launches);

/* One-shot batched solvers on caller data (host buffers, float32), for
 * callers that want the kinematics without the step loop.
 * IK  (Joint::Position / GetVelocity restated, JFC.cpp:68,75-76): pose7[B][7],
 *     twist6[B][6] -> q[B][n], qdot[B][n], jac[B][n][6]. Outputs may be NULL. */
int cdpr_solve_ik(cdpr_handle_t h, const float *pose7, const float *twist6, float *q, float *qdot, float *jac);
/* FK: lengths[B][n], seed7[B][7] -> pose7[B][7], residual[B], iterations[B]. */
int cdpr_solve_fk(cdpr_handle_t h, const float *lengths, const float *seed7, float *pose7, float *residual,
                  int32_t *iterations);
/* TD: pose7[B][7], wrench6[B][6] (wrench the cables must apply to the
 *     platform) -> tension[B][n], infeasible[B]. */
int cdpr_solve_td(cdpr_handle_t h, const float *pose7, const float *wrench6, float *tension, int32_t *infeasible);

#ifdef __cplusplus
}
#endif
#endif /* CDPR_H_ */
