"""Thin object wrapper over the C-ABI: one `Engine` = one `cdpr_handle_t` on one GPU."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _abi
from ._native import lib
from .config import Config, DoneRule


class CdprError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"cdpr error {code}: {message}")
        self.code = code


def _fp(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def derivative_weights(n: int, degree: int) -> np.ndarray:
    """End-point least-squares derivative weights (closed form of Pid::derive, Pid.cpp:193-247)."""
    w = np.empty(n, dtype=np.float64)
    rc = lib().cdpr_derivative_weights(n, degree, w.ctypes.data_as(C.POINTER(C.c_double)))
    if rc != _abi.OK:
        raise CdprError(rc, "bad (n, degree)")
    return w


def plan_kernel(config: Config, steps_per_launch: int = 1, flags: int = 0) -> str:
    """The kernel CDPR_MAP_AUTO would run a launch of `steps_per_launch` world steps of this configuration on (cdpr_plan_kernel:
    answered from the configuration alone, no GPU needed).  flags: _abi.PLAN_* bits.  Raises CdprError with the reason where
    cdpr_create would refuse the configuration."""
    buf = C.create_string_buffer(256)
    s = config.to_struct()
    rc = lib().cdpr_plan_kernel(C.byref(s), int(steps_per_launch), int(flags), buf, 256)
    if rc != _abi.OK:
        raise CdprError(rc, buf.value.decode())
    return buf.value.decode()


def observation_width(fields: int, n: int) -> int:
    """Columns of the observation tensor for the _abi.OBS_* bits `fields` on a robot of n cables (cdpr_observation_width's arithmetic:
    7, 6, n, n, n, 7, 1, 1 per field, in bit order)."""
    if fields & ~_abi.OBS_ALL:
        raise ValueError("unknown OBS_* bit")
    return sum(w for k, w in enumerate((7, 6, n, n, n, 7, 1, 1)) if (fields >> k) & 1)


class Engine:
    """B independent robots advanced in lock step on one GPU."""

    def __init__(self, config: Config, device: int = 0):
        self.config = config
        self._cfg = config.to_struct()
        self.n = config.n_cables
        self.B = int(config.batch)
        self._h = C.c_void_p()
        self._rollout_pending = None
        rc = lib().cdpr_create(C.byref(self._cfg), int(device), C.byref(self._h))
        if rc != _abi.OK:
            msg = lib().cdpr_last_error(None).decode()
            self._h = C.c_void_p()
            if rc == _abi.ERR_INVALID:
                raise ValueError(msg)  # PLG.cpp:167-168 throws on a bad joint count
            raise CdprError(rc, msg)

    # -- lifecycle
    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().cdpr_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int) -> int:
        if rc < 0:
            raise CdprError(rc, lib().cdpr_last_error(self._h).decode())
        return rc

    def reset(self) -> None:
        self._check(lib().cdpr_reset(self._h))

    # -- inputs
    def set_platform_state(self, pose7=None, twist6=None) -> None:
        p = None if pose7 is None else np.ascontiguousarray(pose7, dtype=np.float32).reshape(self.B, 7)
        t = None if twist6 is None else np.ascontiguousarray(twist6, dtype=np.float32).reshape(self.B, 6)
        self._check(lib().cdpr_set_platform_state(self._h, _fp(p), _fp(t)))

    def reset_robots(self, mask, pose7=None, twist6=None) -> None:
        """Model reset of the robots with mask[b] != 0 (Config.perRobotCommands) while the others run on (cdpr_reset_robots):
        platform at pose7[b] / twist6[b] (None: the home pose / zero; rows of the other robots are ignored), controller as after
        Load (JFC.h:69-73, PLG.cpp:153-157).  The world clock, the other robots and every pending command stay as they are.
        Queued on the engine's stream: after every update so far, before every later one; the arrays may be reused at once."""
        m = np.ascontiguousarray(mask, dtype=np.uint8).reshape(self.B)
        p = None if pose7 is None else np.ascontiguousarray(pose7, dtype=np.float32).reshape(self.B, 7)
        t = None if twist6 is None else np.ascontiguousarray(twist6, dtype=np.float32).reshape(self.B, 6)
        self._check(lib().cdpr_reset_robots(self._h, m.ctypes.data_as(C.POINTER(C.c_uint8)), _fp(p), _fp(t)))

    def reset_robots_device(self, d_mask: int, d_pose7: int = 0, d_twist6: int = 0) -> None:
        """The same from device buffers (uint8[B], float[B][7], float[B][6]; 0 = home pose / zero twist): nothing is copied or
        synchronised, the buffers must stay valid until the stream has passed the reset (cdpr_reset_robots_device)."""
        self._check(lib().cdpr_reset_robots_device(self._h, C.c_void_p(d_mask) if d_mask else None, C.c_void_p(d_pose7) if d_pose7 else None,
                                                   C.c_void_p(d_twist6) if d_twist6 else None))

    def copy_robots(self, source) -> None:
        """Fork robots (cdpr_copy_robots): robot r with 0 <= source[r] < B, source[r] != r continues from where robot source[r] is now -
        every getter returns for r what it returns for its source, to the bit, and the two advance identically while they get the same
        commands.  A negative entry or r itself leaves r untouched; a source must itself be untouched and in range (else
        CdprError ERR_INVALID, nothing changed).  Pending commands stay with their index.  Needs Config.perRobotCommands.  Queued on the
        engine's stream; the array may be reused at once."""
        s = np.ascontiguousarray(source, dtype=np.int32).reshape(self.B)
        self._check(lib().cdpr_copy_robots(self._h, s.ctypes.data_as(C.POINTER(C.c_int32))))

    def copy_robots_device(self, d_source: int, d_status: int = 0) -> None:
        """The same from a device map int32[B]: nothing is copied or synchronised (cdpr_copy_robots_device).  A destination whose source
        is out of range or is itself a destination is skipped; d_status (device uint32[2], 0 = no counting) receives
        [robots copied, destinations skipped]."""
        self._check(lib().cdpr_copy_robots_device(self._h, C.c_void_p(d_source) if d_source else None, C.c_void_p(d_status) if d_status else None))

    # -- resampling: weights to the fork's map, on the device
    def resample_map_device(self, spec: _abi.ResampleSpec, d_weights: int, d_source: int, d_words: int = 0, d_ess: int = 0, d_status: int = 0) -> None:
        """Systematic resampling per group of spec.group_size consecutive robots (cdpr_resample_map_device): device float[B] weights to the
        device int32[B] map copy_robots_device takes; nothing is copied or synchronised.  d_words: device uint32[G], one random word per
        group (0 = 2^31 for every group); d_ess: device float[G], the groups' effective sample sizes; d_status: device
        uint32[_abi.RESAMPLE_STATUS]; 0 = not wanted.  Any handle: no robot state is read."""
        vp = lambda x: C.c_void_p(x) if x else None  # noqa: E731
        self._check(lib().cdpr_resample_map_device(self._h, C.byref(spec), vp(d_weights), vp(d_words), vp(d_source), vp(d_ess), vp(d_status)))

    def resample_device(self, spec: _abi.ResampleSpec, d_weights: int, d_source: int = 0, d_words: int = 0, d_ess: int = 0, d_status: int = 0) -> None:
        """The map and the copy on it, back to back on the engine's stream (cdpr_resample_device).  d_source 0: a buffer of the engine's
        own.  Needs Config.perRobotCommands."""
        vp = lambda x: C.c_void_p(x) if x else None  # noqa: E731
        self._check(lib().cdpr_resample_device(self._h, C.byref(spec), vp(d_weights), vp(d_words), vp(d_source), vp(d_ess), vp(d_status)))

    def resample(self, weights, words=None, group_size: int = 0, ess_gate: float = 2.0, copy: bool = True):
        """(source int32[B], ess float32[G], status uint32[_abi.RESAMPLE_STATUS]) on the host: the weights (and words, uint32[G], or None)
        go up, resample_device (copy=True) or resample_map_device (copy=False) runs into scratch buffers, the results come down."""
        P = int(group_size) or self.B
        if P < 1 or self.B % P:
            raise ValueError("resample: the batch is not a whole number of groups")
        G = self.B // P
        w = np.ascontiguousarray(weights, dtype=np.float32).reshape(self.B)
        u = None if words is None else np.ascontiguousarray(words, dtype=np.uint32).reshape(G)
        spec = _abi.ResampleSpec(group_size, ess_gate)

        def body(ptrs):
            d_w, d_u, d_source, d_ess, d_status = ptrs
            self.device_upload_into(d_w, w)
            if u is not None:
                self.device_upload_into(d_u, u)
            if copy:
                self.resample_device(spec, d_w, d_source, d_u, d_ess, d_status)
            else:
                self.resample_map_device(spec, d_w, d_source, d_u, d_ess, d_status)
            return (self.device_download(d_source, self.B, np.int32), self.device_download(d_ess, G, np.float32),
                    self.device_download(d_status, _abi.RESAMPLE_STATUS, np.uint32))

        return self._with_scratch([4 * self.B, None if u is None else 4 * G, 4 * self.B, 4 * G, 4 * _abi.RESAMPLE_STATUS], body)

    # -- MPPI around the rollout: the command batch from the plan, the costs into the next plan, on the device
    def mppi_sample_device(self, spec: _abi.MppiSpec, iteration: int, d_nominal: int, d_commands: int) -> None:
        """The perturbed command batch float[B][H][S][n] rollout_velocity_device reads, from the nominal plan float[B][H][n]
        (cdpr_mppi_sample_device): Philox normals scaled by spec.sigma around every nominal command, clamped under MPPI_CLAMP, sample 0
        the nominal itself under MPPI_NOMINAL_FIRST.  Device buffers; queued on the engine's stream, nothing copied or waited for."""
        vp = lambda x: C.c_void_p(x) if x else None  # noqa: E731
        self._check(lib().cdpr_mppi_sample_device(self._h, C.byref(spec), int(iteration) & 0xFFFFFFFF, vp(d_nominal), vp(d_commands)))

    def mppi_update_device(self, spec: _abi.MppiSpec, d_cost: int, d_commands: int, d_nominal: int, d_action: int = 0, d_weights: int = 0,
                           d_ess: int = 0, d_status: int = 0) -> None:
        """The rollout's costs float[B][S] folded into the plan (cdpr_mppi_update_device): d_nominal float[B][H][n] becomes the
        exp(-(c - c_min) / temperature)-weighted mean of the commands (moved one step on under MPPI_SHIFT), d_action float[B][n] its
        first row - what set_velocity_command_device takes; d_weights float[B][S], d_ess float[B], d_status uint32[_abi.MPPI_STATUS]; 0 =
        not wanted.  Queued on the engine's stream, nothing copied or waited for."""
        vp = lambda x: C.c_void_p(x) if x else None  # noqa: E731
        self._check(lib().cdpr_mppi_update_device(self._h, C.byref(spec), vp(d_cost), vp(d_commands), vp(d_nominal), vp(d_action), vp(d_weights),
                                                  vp(d_ess), vp(d_status)))

    def mppi_sample(self, nominal, spec: _abi.MppiSpec, iteration: int) -> np.ndarray:
        """commands float32[B, H, S, n] on the host: the nominal plan [B, H, n] goes up, mppi_sample_device runs into a scratch buffer, the
        batch comes down."""
        H, S = int(spec.horizon), int(spec.samples)
        u = np.ascontiguousarray(nominal, dtype=np.float32).reshape(self.B, H, self.n)

        def body(ptrs):
            self.device_upload_into(ptrs[0], u)
            self.mppi_sample_device(spec, iteration, ptrs[0], ptrs[1])
            return self.device_download(ptrs[1], (self.B, H, S, self.n), np.float32)

        return self._with_scratch([u.nbytes, 4 * self.B * H * S * self.n], body)

    def mppi_update(self, cost, commands, nominal, spec: _abi.MppiSpec):
        """(nominal float32[B, H, n], action float32[B, n], weights float32[B, S], ess float32[B], status uint32[_abi.MPPI_STATUS]) on the
        host: cost [B, S], commands [B, H, S, n] and the nominal plan go up, mppi_update_device runs on scratch buffers, the results come
        down."""
        H, S = int(spec.horizon), int(spec.samples)
        c = np.ascontiguousarray(cost, dtype=np.float32).reshape(self.B, S)
        v = np.ascontiguousarray(commands, dtype=np.float32).reshape(self.B, H, S, self.n)
        u = np.ascontiguousarray(nominal, dtype=np.float32).reshape(self.B, H, self.n)

        def body(ptrs):
            d_c, d_v, d_u, d_action, d_w, d_ess, d_status = ptrs
            for d, a in ((d_c, c), (d_v, v), (d_u, u)):
                self.device_upload_into(d, a)
            self.mppi_update_device(spec, d_c, d_v, d_u, d_action, d_w, d_ess, d_status)
            return (self.device_download(d_u, (self.B, H, self.n), np.float32), self.device_download(d_action, (self.B, self.n), np.float32),
                    self.device_download(d_w, (self.B, S), np.float32), self.device_download(d_ess, self.B, np.float32),
                    self.device_download(d_status, _abi.MPPI_STATUS, np.uint32))

        return self._with_scratch([c.nbytes, v.nbytes, u.nbytes, 4 * self.B * self.n, c.nbytes, 4 * self.B, 4 * _abi.MPPI_STATUS], body)

    # -- CEM around the rollout: the command batch from a mean and a sigma plan, both refitted to the best samples, on the device
    def cem_sample_device(self, spec: _abi.CemSpec, iteration: int, d_mean: int, d_sigma: int, d_commands: int) -> None:
        """The command batch float[B][H][S][n] rollout_velocity_device reads, from the mean plan and the sigma plan float[B][H][n]
        (cdpr_cem_sample_device): mppi_sample_device's normals, each scaled by its own sigma entry, clamped under CEM_CLAMP, sample 0
        the mean itself under CEM_NOMINAL_FIRST.  Device buffers; queued on the engine's stream, nothing copied or waited for."""
        vp = lambda x: C.c_void_p(x) if x else None  # noqa: E731
        self._check(lib().cdpr_cem_sample_device(self._h, C.byref(spec), int(iteration) & 0xFFFFFFFF, vp(d_mean), vp(d_sigma), vp(d_commands)))

    def cem_update_device(self, spec: _abi.CemSpec, d_cost: int, d_commands: int, d_mean: int, d_sigma: int, d_action: int = 0, d_elite: int = 0,
                          d_best: int = 0, d_status: int = 0) -> None:
        """The rollout's costs float[B][S] turned into the next plans (cdpr_cem_update_device): every robot's spec.elites best samples
        are picked, d_mean and d_sigma float[B][H][n] become the elites' mean and standard deviation blended by spec.alpha into the old
        plans (moved one step on under CEM_SHIFT), d_action float[B][n] the new mean's first row - what set_velocity_command_device
        takes; d_elite float[B][S] (1 for an elite), d_best int32[B], d_status uint32[_abi.CEM_STATUS]; 0 = not wanted.  Queued on the
        engine's stream, nothing copied or waited for."""
        vp = lambda x: C.c_void_p(x) if x else None  # noqa: E731
        self._check(lib().cdpr_cem_update_device(self._h, C.byref(spec), vp(d_cost), vp(d_commands), vp(d_mean), vp(d_sigma), vp(d_action),
                                                 vp(d_elite), vp(d_best), vp(d_status)))

    def cem_sample(self, mean, sigma, spec: _abi.CemSpec, iteration: int) -> np.ndarray:
        """commands float32[B, H, S, n] on the host: the mean and sigma plans [B, H, n] go up, cem_sample_device runs into a scratch
        buffer, the batch comes down."""
        H, S = int(spec.horizon), int(spec.samples)
        m = np.ascontiguousarray(mean, dtype=np.float32).reshape(self.B, H, self.n)
        g = np.ascontiguousarray(sigma, dtype=np.float32).reshape(self.B, H, self.n)

        def body(ptrs):
            self.device_upload_into(ptrs[0], m)
            self.device_upload_into(ptrs[1], g)
            self.cem_sample_device(spec, iteration, ptrs[0], ptrs[1], ptrs[2])
            return self.device_download(ptrs[2], (self.B, H, S, self.n), np.float32)

        return self._with_scratch([m.nbytes, g.nbytes, 4 * self.B * H * S * self.n], body)

    def cem_update(self, cost, commands, mean, sigma, spec: _abi.CemSpec):
        """(mean float32[B, H, n], sigma float32[B, H, n], action float32[B, n], elite float32[B, S], best int32[B], status
        uint32[_abi.CEM_STATUS]) on the host: cost [B, S], commands [B, H, S, n] and both plans go up, cem_update_device runs on scratch
        buffers, the results come down."""
        H, S = int(spec.horizon), int(spec.samples)
        c = np.ascontiguousarray(cost, dtype=np.float32).reshape(self.B, S)
        v = np.ascontiguousarray(commands, dtype=np.float32).reshape(self.B, H, S, self.n)
        m = np.ascontiguousarray(mean, dtype=np.float32).reshape(self.B, H, self.n)
        g = np.ascontiguousarray(sigma, dtype=np.float32).reshape(self.B, H, self.n)

        def body(ptrs):
            d_c, d_v, d_m, d_g, d_action, d_elite, d_best, d_status = ptrs
            for d, a in ((d_c, c), (d_v, v), (d_m, m), (d_g, g)):
                self.device_upload_into(d, a)
            self.cem_update_device(spec, d_c, d_v, d_m, d_g, d_action, d_elite, d_best, d_status)
            return (self.device_download(d_m, (self.B, H, self.n), np.float32), self.device_download(d_g, (self.B, H, self.n), np.float32),
                    self.device_download(d_action, (self.B, self.n), np.float32), self.device_download(d_elite, (self.B, S), np.float32),
                    self.device_download(d_best, self.B, np.int32), self.device_download(d_status, _abi.CEM_STATUS, np.uint32))

        return self._with_scratch([c.nbytes, v.nbytes, m.nbytes, g.nbytes, 4 * self.B * self.n, c.nbytes, 4 * self.B, 4 * _abi.CEM_STATUS], body)

    # -- done rules: who should be put back, decided on the device
    @staticmethod
    def _rule(rule):
        """a DoneRule, or its struct built once (DoneRule.to_struct()) by a loop that calls every step"""
        return rule if isinstance(rule, _abi.DoneRuleStruct) else rule.to_struct()

    def evaluate_done(self, rule: DoneRule) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The verdict of `rule` on the state the engine holds now (cdpr_evaluate_done): mask uint8[B] (0 or 1), reason uint32[B] (the
        rule's enabled _abi.DONE_* bits that hold for the robot), counts uint32[_abi.DONE_COUNTS] (counts[0] robots done, counts[1 + k]
        robots with reason bit k).  A pure function of raw_state, fk_state (residual), td_state (infeasible), limit_state,
        episode_start and step_count.  Waits for the stream once."""
        mask, reason, counts = np.empty(self.B, dtype=np.uint8), np.empty(self.B, dtype=np.uint32), np.empty(_abi.DONE_COUNTS, dtype=np.uint32)
        s = self._rule(rule)
        u32 = C.POINTER(C.c_uint32)
        self._check(lib().cdpr_evaluate_done(self._h, C.byref(s), mask.ctypes.data_as(C.POINTER(C.c_uint8)), reason.ctypes.data_as(u32), counts.ctypes.data_as(u32)))
        return mask, reason, counts

    def evaluate_done_device(self, rule: DoneRule, d_mask: int, d_reason: int = 0, d_counts: int = 0) -> None:
        """The same into device buffers (uint8[B], uint32[B], uint32[_abi.DONE_COUNTS]; 0 = not wanted): queued on the engine's stream,
        nothing copied back or waited for (cdpr_evaluate_done_device).  d_mask is what reset_robots_device takes."""
        s = self._rule(rule)
        self._check(lib().cdpr_evaluate_done_device(self._h, C.byref(s), C.c_void_p(d_mask) if d_mask else None, C.c_void_p(d_reason) if d_reason else None,
                                                    C.c_void_p(d_counts) if d_counts else None))

    def reset_done_device(self, rule: DoneRule, d_pose7: int = 0, d_twist6: int = 0, d_counts: int = 0) -> None:
        """Evaluate `rule` and reset the robots it finds done, with no host wait in between (cdpr_reset_done_device): d_pose7 / d_twist6
        as for reset_robots_device, d_counts receives the verdict's counts.  Needs Config.perRobotCommands."""
        s = self._rule(rule)
        self._check(lib().cdpr_reset_done_device(self._h, C.byref(s), C.c_void_p(d_pose7) if d_pose7 else None, C.c_void_p(d_twist6) if d_twist6 else None,
                                                 C.c_void_p(d_counts) if d_counts else None))

    def episode_start(self) -> np.ndarray:
        """uint32[B]: the world step (low 32 bits of step_count) of every robot's last model reset; after create and reset() the low word of the
        clock's origin (0 unless CDPR_STEP_ORIGIN was set at create: include/cdpr.h, cdpr_step_count)."""
        start = np.empty(self.B, dtype=np.uint32)
        self._check(lib().cdpr_get_episode_start(self._h, start.ctypes.data_as(C.POINTER(C.c_uint32))))
        return start

    # -- the environment view: observation tensor, reward and verdict where the state is
    def observation_width(self, fields: int) -> int:
        """Columns of the observation tensor for the _abi.OBS_* bits `fields` on this handle (cdpr_observation_width)."""
        w = C.c_uint32()
        self._check(lib().cdpr_observation_width(self._h, int(fields), C.byref(w)))
        return int(w.value)

    def observe_device(self, fields: int, d_obs: int, ld: int = 0, d_row_mask: int = 0) -> None:
        """The observation tensor float[B][ld] (ld = 0: packed) into the device buffer d_obs, queued on the engine's stream, nothing copied
        back or waited for (cdpr_observe_device).  Column j of robot b is to the bit what the field's getter returns.  d_row_mask: device
        uint8[B], only the rows with a non-zero byte are written (after reset_robots_device(mask): the done robots' fresh observation)."""
        self._check(lib().cdpr_observe_device(self._h, int(fields), int(ld), C.c_void_p(d_row_mask) if d_row_mask else None, C.c_void_p(d_obs) if d_obs else None))

    def env_evaluate_device(self, spec: _abi.EnvSpec, d_target7: int = 0, d_obs: int = 0, d_reward: int = 0, d_mask: int = 0, d_reason: int = 0, d_counts: int = 0) -> None:
        """Observation (float[B][spec.ld]), tracking reward (float[B]) and the verdict of spec.done (as evaluate_done_device) in one launch
        into device buffers; 0 = not wanted, not all of them (cdpr_env_evaluate_device).  d_target7: device float[B][7], 0 = the home pose."""
        vp = lambda x: C.c_void_p(x) if x else None  # noqa: E731
        self._check(lib().cdpr_env_evaluate_device(self._h, C.byref(spec), vp(d_target7), vp(d_obs), vp(d_reward), vp(d_mask), vp(d_reason), vp(d_counts)))

    def _with_scratch(self, sizes, body):
        """body(pointers) with one device buffer per entry of `sizes` (bytes; None: no buffer, 0); every buffer is freed afterwards, on an
        exception too."""
        ptrs = []
        try:
            for nbytes in sizes:
                ptrs.append(0 if nbytes is None else self.device_alloc(nbytes))
            return body(ptrs)
        finally:
            for p in ptrs:
                if p:
                    lib().cdpr_device_free(self._h, C.c_void_p(p))

    def observe(self, fields: int) -> np.ndarray:
        """The packed observation tensor float32[B, width] on the host: observe_device into a scratch buffer, then one download."""
        width = self.observation_width(fields)

        def body(ptrs):
            self.observe_device(fields, ptrs[0])
            return self.device_download(ptrs[0], (self.B, width), np.float32)

        return self._with_scratch([4 * self.B * max(width, 1)], body)

    def env_evaluate(self, spec: _abi.EnvSpec, target7=None):
        """(obs float32[B, width] or None where spec.fields is 0, reward float32[B], mask uint8[B], reason uint32[B], counts
        uint32[_abi.DONE_COUNTS]) on the host: env_evaluate_device into scratch buffers, then the downloads.  target7: [B, 7] or None."""
        width = self.observation_width(spec.fields)
        ld = int(spec.ld) or width
        tgt = None if target7 is None else np.ascontiguousarray(target7, dtype=np.float32).reshape(self.B, 7)

        def body(ptrs):
            d_obs, d_reward, d_mask, d_reason, d_counts, d_target = ptrs
            if tgt is not None:
                self.device_upload_into(d_target, tgt)
            self.env_evaluate_device(spec, d_target, d_obs, d_reward, d_mask, d_reason, d_counts)
            obs = self.device_download(d_obs, (self.B, ld), np.float32)[:, :width].copy() if d_obs else None
            return (obs, self.device_download(d_reward, self.B, np.float32), self.device_download(d_mask, self.B, np.uint8),
                    self.device_download(d_reason, self.B, np.uint32), self.device_download(d_counts, _abi.DONE_COUNTS, np.uint32))

        return self._with_scratch([4 * self.B * ld if width else None, 4 * self.B, self.B, 4 * self.B, 4 * _abi.DONE_COUNTS, None if tgt is None else tgt.nbytes], body)

    def _command(self, fn, fn_masked, axes, mask) -> int:
        a = np.ascontiguousarray(axes, dtype=np.float32).ravel()
        if mask is None:
            return self._check(fn(self._h, _fp(a), a.size))
        m = np.ascontiguousarray(mask, dtype=np.uint8).reshape(self.B)
        return self._check(fn_masked(self._h, _fp(a), a.size, m.ctypes.data_as(C.POINTER(C.c_uint8))))

    def set_velocity_command(self, axes, mask=None) -> int:
        """Joy on `jointVelocities`.  mask[B] (Config.perRobotCommands): only these robots receive it, the others keep
        their target, mode and Pid state (what independent plugin instances do, PLG.cpp:206-219)."""
        return self._command(lib().cdpr_set_velocity_command, lib().cdpr_set_velocity_command_masked, axes, mask)

    def set_position_command(self, axes, mask=None) -> int:
        return self._command(lib().cdpr_set_position_command, lib().cdpr_set_position_command_masked, axes, mask)

    def set_force_command(self, axes, mask=None) -> int:
        """JointForceCalculator::setForce on every joint (JFC.h:92-95): open-loop forces, held until another command of
        any kind arrives; no Pid runs (JFC.cpp:67-70).  Latched after a pending velocity / position command."""
        return self._command(lib().cdpr_set_force_command, lib().cdpr_set_force_command_masked, axes, mask)

    def set_force_command_device(self, dptr: int, count: int) -> int:
        return self._check(lib().cdpr_set_force_command_device(self._h, C.c_void_p(dptr), count))

    def bind_force_command_device(self, dptr: int, count: int) -> int:
        return self._check(lib().cdpr_bind_force_command_device(self._h, C.c_void_p(dptr), count))

    def bind_velocity_command_device(self, dptr: int, count: int) -> int:
        """Zero-copy: the device buffer float[B][n] at dptr is the latched Joy batch from the next update on; it must stay
        valid and unchanged until another velocity command has been latched."""
        return self._check(lib().cdpr_bind_velocity_command_device(self._h, C.c_void_p(dptr), count))

    def bind_position_command_device(self, dptr: int, count: int) -> int:
        return self._check(lib().cdpr_bind_position_command_device(self._h, C.c_void_p(dptr), count))

    def set_velocity_command_device(self, dptr: int, count: int) -> int:
        return self._check(lib().cdpr_set_velocity_command_device(self._h, C.c_void_p(dptr), count))

    def set_position_command_device(self, dptr: int, count: int) -> int:
        return self._check(lib().cdpr_set_position_command_device(self._h, C.c_void_p(dptr), count))

    # -- stepping
    def update(self, nsteps: int = 1, steps_per_launch: int = 1) -> None:
        if steps_per_launch == 1:
            self._check(lib().cdpr_update(self._h, int(nsteps)))
        else:
            self._check(lib().cdpr_update_fused(self._h, int(nsteps), int(steps_per_launch)))

    def observable_image_bytes(self) -> int:
        nbytes = C.c_size_t()
        self._check(lib().cdpr_observable_image_bytes(self._h, C.byref(nbytes)))
        return int(nbytes.value)

    def update_record_device(self, nsteps: int, steps_per_launch: int, d_record: int, record_bytes: int) -> None:
        """As update_record, into a caller-owned device buffer (nothing is copied back)."""
        self._check(lib().cdpr_update_record(self._h, int(nsteps), int(steps_per_launch), C.c_void_p(d_record), record_bytes))

    def update_scheduled(self, nsteps: int, refresh_steps: int, d_commands: int, d_record: int = 0, record_bytes: int = 0, d_ready: int = 0,
                         kind: str = "velocity", d_robot_masks: int = 0) -> None:
        """A whole command schedule resident in HBM, queued with one call: Joy batch j (device buffer float[batches][B][n] at
        d_commands) is latched at step j * refresh_steps as a `kind` command ("velocity" = jointVelocities, "position" =
        jointPositions, "force" = setForce); every step's observables go to the record (device buffer) if one is given.
        d_ready: optional device-visible uint32[batches] mailbox (batch j is taken once d_ready[j] != 0).  d_robot_masks
        (Config.perRobotCommands): device buffer uint8[batches][B], batch j reaches only the robots of its mask.
        Uniform-mode handles on the register-resident path run it in ONE launch; every other handle as a chain of launches
        queued back to back (same results: cdpr_update_scheduled_kind)."""
        k = {"velocity": _abi.COMMAND_VELOCITY, "position": _abi.COMMAND_POSITION, "force": _abi.COMMAND_FORCE}[kind]
        self._check(lib().cdpr_update_scheduled_kind(self._h, k, int(nsteps), int(refresh_steps), C.c_void_p(d_commands), C.c_void_p(d_ready) if d_ready else None,
                                                     C.c_void_p(d_robot_masks) if d_robot_masks else None, C.c_void_p(d_record) if d_record else None, int(record_bytes)))

    def update_record(self, nsteps: int, steps_per_launch: int = 10):
        """Advance nsteps world steps (fused launches) and return the observables of EVERY step:
        dict of arrays position/velocity/effort [nsteps, B, n], pose [nsteps, B, 7], twist [nsteps, B, 6]."""
        nbytes = C.c_size_t()
        self._check(lib().cdpr_observable_image_bytes(self._h, C.byref(nbytes)))
        image = int(nbytes.value)
        dptr = C.c_void_p()
        self._check(lib().cdpr_device_malloc(self._h, image * nsteps, C.byref(dptr)))
        try:
            self._check(lib().cdpr_update_record(self._h, int(nsteps), int(steps_per_launch), dptr, image * nsteps))
            raw = np.empty(image * nsteps, dtype=np.uint8)
            self._check(lib().cdpr_device_download(self._h, raw.ctypes.data_as(C.c_void_p), dptr, raw.nbytes))
        finally:
            lib().cdpr_device_free(self._h, dptr)
        f64 = int(self.config.precision) == 64  # precision = 64 handles record doubles and hand out float64 arrays
        out = {k: np.empty((nsteps, self.B, w), dtype=np.float64 if f64 else np.float32) for k, w in (("position", self.n), ("velocity", self.n), ("effort", self.n), ("pose", 7), ("twist", 6))}
        for j in range(nsteps):
            img = raw[j * image:(j + 1) * image]
            if f64:
                self._check(lib().cdpr_decode_observables_f64(self._h, img.ctypes.data_as(C.c_void_p), self._dp(out["position"][j]), self._dp(out["velocity"][j]),
                                                              self._dp(out["effort"][j]), self._dp(out["pose"][j]), self._dp(out["twist"][j])))
            else:
                self._check(lib().cdpr_decode_observables(self._h, img.ctypes.data_as(C.c_void_p), _fp(out["position"][j]), _fp(out["velocity"][j]),
                                                          _fp(out["effort"][j]), _fp(out["pose"][j]), _fp(out["twist"][j])))
        return out

    def decode_observables(self, image: np.ndarray):
        """One downloaded observable image (uint8[observable_image_bytes]) -> (position, velocity, effort, pose7, twist6)."""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        out = [np.empty((self.B, w), dtype=np.float32) for w in (self.n, self.n, self.n, 7, 6)]
        self._check(lib().cdpr_decode_observables(self._h, img.ctypes.data_as(C.c_void_p), *[_fp(o) for o in out]))
        return tuple(out)

    def synchronize(self) -> None:
        self._check(lib().cdpr_synchronize(self._h))

    @property
    def step_count(self) -> int:
        return int(lib().cdpr_step_count(self._h))

    @property
    def kernel_name(self) -> str:
        """The kernel the last step launch of this handle ran on (cdpr_kernel_name)."""
        buf = C.create_string_buffer(256)
        self._check(lib().cdpr_kernel_name(self._h, buf, 256))
        return buf.value.decode()

    @property
    def last_variant(self) -> int:
        """Which instantiation of `kernel_name` the last step launch took (cdpr_debug_last_variant, a debug getter outside the
        C-ABI header): 1 = the role-split kernel with its steady-state controller wave, 0 = the kernel as named."""
        fn = lib().cdpr_debug_last_variant
        fn.argtypes, fn.restype = [C.c_void_p], C.c_int
        return int(fn(self._h))

    @property
    def mapping(self) -> str:
        return {_abi.MAP_LANE_PER_ROBOT: "lane-per-robot", _abi.MAP_LANE_PAIR: "lane-pair", _abi.MAP_LANE_PER_CABLE: "lane-per-cable"}.get(int(lib().cdpr_mapping(self._h)), "auto")

    @property
    def sim_time(self) -> float:
        return self.step_count * self.config.dt

    # -- observables
    def joint_states(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        q, qd, e = (np.empty((self.B, self.n), dtype=np.float32) for _ in range(3))
        self._check(lib().cdpr_get_joint_states(self._h, _fp(q), _fp(qd), _fp(e)))
        return q, qd, e

    def platform_state(self) -> Tuple[np.ndarray, np.ndarray]:
        p, t = np.empty((self.B, 7), dtype=np.float32), np.empty((self.B, 6), dtype=np.float32)
        self._check(lib().cdpr_get_platform_state(self._h, _fp(p), _fp(t)))
        return p, t

    def observables(self):
        """JointState + PlatformState arrays of the last published step in one device round trip (cdpr_get_observables):
        position, velocity, effort [B, n], pose [B, 7], twist [B, 6]."""
        q, qd, e = (np.empty((self.B, self.n), dtype=np.float32) for _ in range(3))
        p, t = np.empty((self.B, 7), dtype=np.float32), np.empty((self.B, 6), dtype=np.float32)
        self._check(lib().cdpr_get_observables(self._h, _fp(q), _fp(qd), _fp(e), _fp(p), _fp(t)))
        return q, qd, e, p, t

    # -- handles created with Config.precision = 64: the same read-outs in double
    @staticmethod
    def _dp(a: Optional[np.ndarray]):
        return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))

    def observables_f64(self):
        """position, velocity, effort [B, n], pose [B, 7], twist [B, 6] of the last published step, float64."""
        q, qd, e = (np.empty((self.B, self.n), dtype=np.float64) for _ in range(3))
        p, t = np.empty((self.B, 7), dtype=np.float64), np.empty((self.B, 6), dtype=np.float64)
        self._check(lib().cdpr_get_observables_f64(self._h, self._dp(q), self._dp(qd), self._dp(e), self._dp(p), self._dp(t)))
        return q, qd, e, p, t

    def raw_state_f64(self) -> Tuple[np.ndarray, np.ndarray]:
        p, t = np.empty((self.B, 7), dtype=np.float64), np.empty((self.B, 6), dtype=np.float64)
        self._check(lib().cdpr_get_raw_state_f64(self._h, self._dp(p), self._dp(t)))
        return p, t

    def set_platform_state_f64(self, pose7=None, twist6=None) -> None:
        p = None if pose7 is None else np.ascontiguousarray(pose7, dtype=np.float64).reshape(self.B, 7)
        t = None if twist6 is None else np.ascontiguousarray(twist6, dtype=np.float64).reshape(self.B, 6)
        self._check(lib().cdpr_set_platform_state_f64(self._h, self._dp(p), self._dp(t)))

    def raw_state(self) -> Tuple[np.ndarray, np.ndarray]:
        p, t = np.empty((self.B, 7), dtype=np.float32), np.empty((self.B, 6), dtype=np.float32)
        self._check(lib().cdpr_get_raw_state(self._h, _fp(p), _fp(t)))
        return p, t

    def pid_debug(self) -> np.ndarray:
        d = np.empty((self.B, _abi.PID_DEBUG_AXES), dtype=np.float32)
        self._check(lib().cdpr_get_pid_debug(self._h, _fp(d)))
        return d

    def fk_state(self):
        p, r, it = np.empty((self.B, 7), dtype=np.float32), np.empty(self.B, dtype=np.float32), np.empty(self.B, dtype=np.int32)
        self._check(lib().cdpr_get_fk_state(self._h, _fp(p), _fp(r), it.ctypes.data_as(C.POINTER(C.c_int32))))
        return p, r, it

    def td_state(self):
        t, f = np.empty((self.B, self.n), dtype=np.float32), np.empty(self.B, dtype=np.int32)
        self._check(lib().cdpr_get_td_state(self._h, _fp(t), f.ctypes.data_as(C.POINTER(C.c_int32))))
        return t, f

    def limit_state(self) -> np.ndarray:
        """Travel limits (Model.travel_lower / travel_upper; cube.sdf:436-437): uint32[B], bit i set where joint i's
        position was outside the range at the last published step."""
        m = np.empty(self.B, dtype=np.uint32)
        self._check(lib().cdpr_get_limit_state(self._h, m.ctypes.data_as(C.POINTER(C.c_uint32))))
        return m

    # -- one-shot batched kinematics on caller data
    def solve_ik(self, pose7, twist6=None):
        """Joint::Position / GetVelocity restated: q[B,n], qdot[B,n], J[B,n,6] for the given poses (and twists)."""
        p = np.ascontiguousarray(pose7, dtype=np.float32).reshape(self.B, 7)
        t = None if twist6 is None else np.ascontiguousarray(twist6, dtype=np.float32).reshape(self.B, 6)
        q, qd = np.empty((self.B, self.n), dtype=np.float32), np.empty((self.B, self.n), dtype=np.float32)
        jac = np.empty((self.B, self.n, 6), dtype=np.float32)
        self._check(lib().cdpr_solve_ik(self._h, _fp(p), _fp(t), _fp(q), _fp(qd), _fp(jac)))
        return q, qd, jac

    def solve_fk(self, lengths, seed7):
        """Newton-Raphson forward kinematics: pose7[B,7], residual[B], iterations[B]."""
        ln = np.ascontiguousarray(lengths, dtype=np.float32).reshape(self.B, self.n)
        sd = np.ascontiguousarray(seed7, dtype=np.float32).reshape(self.B, 7)
        pose, res, it = np.empty((self.B, 7), dtype=np.float32), np.empty(self.B, dtype=np.float32), np.empty(self.B, dtype=np.int32)
        self._check(lib().cdpr_solve_fk(self._h, _fp(ln), _fp(sd), _fp(pose), _fp(res), it.ctypes.data_as(C.POINTER(C.c_int32))))
        return pose, res, it

    def solve_td(self, pose7, wrench6):
        """Tension distribution for the wrench the cables must apply: tension[B,n], infeasible[B]."""
        p = np.ascontiguousarray(pose7, dtype=np.float32).reshape(self.B, 7)
        w = np.ascontiguousarray(wrench6, dtype=np.float32).reshape(self.B, 6)
        t, f = np.empty((self.B, self.n), dtype=np.float32), np.empty(self.B, dtype=np.int32)
        self._check(lib().cdpr_solve_td(self._h, _fp(p), _fp(w), _fp(t), f.ctypes.data_as(C.POINTER(C.c_int32))))
        return t, f

    # -- MPC fan-out
    def rollout_launch(self, commands, ref_position):
        """Queue one rollout and return at once (cdpr_rollout_velocity_launch): commands[B, H, S, n] as a host array
        (uploaded here, freed by rollout_fetch) or a (device_pointer, S, H) tuple for a buffer already in HBM."""
        if self._rollout_pending is not None:
            raise RuntimeError("rollout_launch: the previous rollout has not been fetched (call rollout_fetch first)")
        ref = np.ascontiguousarray(ref_position, dtype=np.float32).reshape(self.B, 3)
        if isinstance(commands, tuple):
            dptr, S, H = commands
            owned = None
        else:
            c = np.ascontiguousarray(commands, dtype=np.float32)
            assert c.ndim == 4 and c.shape[0] == self.B and c.shape[3] == self.n, "commands must be [B, H, S, n]"
            H, S = int(c.shape[1]), int(c.shape[2])
            dptr = owned = self.device_upload(c)
        try:
            self._check(lib().cdpr_rollout_velocity_launch(self._h, int(S), int(H), C.c_void_p(dptr), _fp(ref)))
        except Exception:
            if owned is not None:
                self.device_free(owned)
            raise
        self._rollout_pending = (int(S), owned)

    def rollout_fetch(self) -> np.ndarray:
        """cost[B, S] of the rollout queued by rollout_launch (synchronises the stream)."""
        if self._rollout_pending is None:
            raise RuntimeError("rollout_fetch: no rollout pending (call rollout_launch first)")
        S, owned = self._rollout_pending
        cost = np.empty((self.B, S), dtype=np.float32)
        try:
            self._check(lib().cdpr_rollout_velocity_fetch(self._h, _fp(cost)))
        finally:
            self._rollout_pending = None
            if owned is not None:
                self.device_free(owned)
        return cost

    def rollout_discard(self) -> None:
        """Drop a launched rollout without reading its costs (waits for it; frees an uploaded command buffer)."""
        if self._rollout_pending is None:
            return
        _, owned = self._rollout_pending
        self._rollout_pending = None
        try:
            self.synchronize()
        finally:
            if owned is not None:
                self.device_free(owned)

    def rollout_velocity(self, commands, ref_position) -> np.ndarray:
        """commands[B, H, S, n] (host array, or a (device_pointer, S, H) tuple for a buffer already in HBM),
        ref_position[B, 3] -> cost[B, S]; the engine's own state is left untouched."""
        self.rollout_launch(commands, ref_position)
        return self.rollout_fetch()

    def rollout_velocity_device(self, d_commands: int, samples: int, horizon: int, d_ref: int, d_cost: int) -> None:
        """Device-resident rollout: nothing copied, asynchronous on the engine's stream."""
        self._check(lib().cdpr_rollout_velocity_device(self._h, int(samples), int(horizon), C.c_void_p(d_commands), C.c_void_p(d_ref),
                                                       C.c_void_p(d_cost)))

    # -- caller-owned device buffers (e.g. a schedule of Joy batches resident in HBM)
    def device_upload(self, array: np.ndarray) -> int:
        a = np.ascontiguousarray(array)
        ptr = C.c_void_p()
        self._check(lib().cdpr_device_malloc(self._h, a.nbytes, C.byref(ptr)))
        self._check(lib().cdpr_device_upload(self._h, ptr, a.ctypes.data_as(C.c_void_p), a.nbytes))
        return int(ptr.value)

    def device_upload_into(self, dptr: int, array: np.ndarray) -> None:
        """Host array into an existing device buffer, on THIS handle's stream.  (Not the way to post the mailbox of a schedule that is
        already waiting: the copy may share the waiting launch's hardware queue - keep such words in mapped pinned host memory.)"""
        a = np.ascontiguousarray(array)
        self._check(lib().cdpr_device_upload(self._h, C.c_void_p(dptr), a.ctypes.data_as(C.c_void_p), a.nbytes))

    def device_alloc(self, nbytes: int) -> int:
        ptr = C.c_void_p()
        self._check(lib().cdpr_device_malloc(self._h, int(nbytes), C.byref(ptr)))
        return int(ptr.value)

    def device_download(self, dptr: int, shape, dtype=np.float32) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        self._check(lib().cdpr_device_download(self._h, out.ctypes.data_as(C.c_void_p), C.c_void_p(dptr), out.nbytes))
        return out

    def device_free(self, dptr: int) -> None:
        self._check(lib().cdpr_device_free(self._h, C.c_void_p(dptr)))

    # -- timing (HIP events on the engine's own stream)
    def profile_begin(self) -> None:
        self._check(lib().cdpr_profile_begin(self._h))

    def profile_end(self) -> Tuple[float, int]:
        ms, n = C.c_float(), C.c_uint64()
        self._check(lib().cdpr_profile_end(self._h, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def bytes_per_state_step(self) -> int:
        return int(lib().cdpr_bytes_per_state_step(C.byref(self._cfg)))
