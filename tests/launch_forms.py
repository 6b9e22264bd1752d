"""What tests/test_launch_form_inputs.py (CPU) and tests/test_gpu_launch_forms_after_robot_ops.py (GPU) share: the launch forms a
per-robot handle can be stepped in, the script that puts a reset or a copy between segments stepped in ONE form, the rollout inputs,
and the "half recipe" - a reset that forgets the controller - which the CPU module uses to show that the script can tell.

A Player is one simulator (an Engine, or an OracleSim as form "oracle") that runs every segment of k world steps in its form:

  one      update(1) x k, the observables read after every step
  fused10  update(k, 10)
  fused3   update(k, 3)             (30 steps: ten launches of three, the captured graph of the register-resident kinds)
  rec      update_record(k, 10)     (every step's image kept)
  long     update(k, min(k, 64))    (one launch per segment)
  sched    as long; a Joy segment goes in as a one-batch schedule update_scheduled(k, k, rows, kind, masks), the engine's own
           set_*_command is not called for it
  oracle   update(1) x k, platform_state + joint_states kept after every step

A Scenario is the engines (one Player per form), the oracle Player, the op and the after-script of one case; its `make` lets
tests/test_gpu_padded_stride.py put the same case on handles with a padded row stride.

B = 130: two full wavefronts and a ragged one, stride 192.
"""
import numpy as np

import copy_robots as cr
import robot_histories as ri
from parity import engines, observed, oracle_at, rollout_cost_tol
from per_robot_kinds import ALL, config_of

B = ri.B
KINDS = ALL + ["general_one_wave"]
GENERAL = ["general_n8", "general_lean_hot", "general_long", "general_one_wave"]  # per-wave tier decisions: exact only lane for lane
FORMS = ("one", "fused10", "fused3", "rec", "long", "sched")
SAMPLES = 3  # trajectories per robot in a rollout: a wave mixes those of reset and of untouched robots
SETTER = {"velocity": "set_velocity_command", "position": "set_position_command", "force": "set_force_command"}
# the after-script: (checkpoint, the masked Joy in front of the segment or None, its key in after_inputs, steps)
SEGMENTS = (
    ("13 steps after the op", None, None, 13),
    ("30 steps after the masked velocity Joy", "velocity", "v", 30),
    ("25 steps after the masked position Joy", "position", "p", 25),
    ("12 steps after the masked force Joy", "force", "f", 12),
)


def steps_of_the_last_launch(form, k):
    """world steps of the last launch of a segment of k steps (what kernel_name then speaks of)"""
    spl = {"one": 1, "fused10": 10, "fused3": 3, "rec": 10}.get(form, min(k, 64))
    return k % spl or spl


class Player:
    def __init__(self, sim, form, cfg):
        assert form in FORMS + ("oracle",)
        self.sim, self.form, self.cfg = sim, form, cfg
        self.steps = []     # forms one, rec, oracle: readout after every world step
        self.record = None  # form rec: what the last update_record returned
        self.launches = []  # engines: (form's steps in the last launch of the segment, kernel_name after it)

    def run(self, k):
        s, form = self.sim, self.form
        if form in ("one", "oracle"):
            for _ in range(k):
                s.update(1)
                self.steps.append(observed(s, self.cfg.precision == 64))
        elif form == "rec":
            self.record = r = s.update_record(k, 10)
            self.steps += [(r["pose"][j], r["twist"][j], r["position"][j], r["velocity"][j], r["effort"][j]) for j in range(k)]
        else:
            s.update(k, {"fused10": 10, "fused3": 3}.get(form, min(k, 64)))
        self._log(k)

    def joy(self, kind, rows, mask, k):
        """the masked Joy `kind`, then k steps"""
        if self.form != "sched":
            assert getattr(self.sim, SETTER[kind])(rows, mask=mask) == 0
            return self.run(k)
        s = self.sim
        batch = self.cfg.batch
        d_rows = s.device_upload(np.ascontiguousarray(rows, dtype=np.float32).reshape(1, batch, -1))
        d_mask = s.device_upload(np.ascontiguousarray(mask, dtype=np.uint8).reshape(1, batch))
        s.update_scheduled(k, k, d_rows, kind=kind, d_robot_masks=d_mask)
        s.synchronize()
        s.device_free(d_rows), s.device_free(d_mask)
        self._log(k)

    def _log(self, k):
        if self.form != "oracle":
            self.launches.append((steps_of_the_last_launch(self.form, k), self.sim.kernel_name))

    def close(self):
        self.sim.close()


class Scenario:
    """Engines (one per form) and, with an oracle, its Player at the end of the history; the op; the after-script.  On a copy the oracle
    is the twin from birth and the after-script's input rows of every destination are those of its source.  make(cfg, pose, forms):
    the engines at `pose`, one per form (default: parity.engines; tests/padded_stride.py passes handles on a padded row stride)."""

    def __init__(self, pkg, oracle, monkeypatch, kind, op, forms, seed, shift=0, make=None):
        self.pkg, self.kind, self.op = pkg, kind, op
        self.cfg = cfg = config_of(pkg, kind, monkeypatch)
        self.source = None if op == "reset" else cr.copy_map() if op == "copy" else cr.aligned_map()
        self.mask = ri.reset_mask()
        self.touched = self.mask.astype(bool) if op == "reset" else cr.destinations_of(self.source)
        self.h, self.a = ri.history_inputs(cfg.model, seed, shift), after_inputs(cfg.model, 77)
        twinned = (lambda x: x) if op == "reset" else (lambda x: cr.twin_rows(x, self.source))
        self.ht, self.at = twinned(self.h), twinned(self.a)
        made = engines(pkg, cfg, self.h["pose"], len(forms)) if make is None else make(cfg, self.h["pose"], forms)
        self.players = [Player(e, form, cfg) for e, form in zip(made, forms)]
        self.ora = Player(oracle_at(oracle, cfg, self.ht["pose"]), "oracle", cfg) if oracle is not None else None
        play_history(self.players, self.h)
        if self.ora:
            play_history([self.ora], self.ht)

    def everyone(self):
        return self.players + ([self.ora] if self.ora else [])

    def apply(self):
        for p in self.players:
            p.sim.reset_robots(self.mask, self.a["pose"]) if self.op == "reset" else p.sim.copy_robots(self.source)
        if self.ora and self.op == "reset":
            ri.oracle_reset(self.ora.sim, self.mask, self.a["pose"])
        for p in self.everyone():
            p.steps.clear()

    def play_after(self, check):
        play_after(self.everyone(), self.at, check)

    def close(self):
        for p in self.everyone():
            p.close()


def after_inputs(model, seed, batch=B):
    """ri.after_inputs and the force Joy of the last segment: around what holds the platform, for every fifth robot"""
    a = ri.after_inputs(model, seed, batch)
    a["f"] = ri.forces(model.n_cables, np.random.default_rng(9), batch)
    a["f_mask"] = (np.arange(batch) % 5 == 0).astype(np.uint8)
    return a


def play_history(players, h, steps=ri.HISTORY):
    """ri.play_history, every player in its own form"""
    for p in players:
        assert p.sim.set_position_command(h["p"], mask=(h["group"] == 0).astype(np.uint8)) == 0
        assert p.sim.set_velocity_command(h["v"], mask=(h["group"] == 1).astype(np.uint8)) == 0
        assert p.sim.set_force_command(h["f"], mask=(h["group"] == 2).astype(np.uint8)) == 0
        p.run(steps)


def play_after(players, a, check):
    """The script behind the op; check(label, steps of the segment) after each segment."""
    for label, kind, key, k in SEGMENTS:
        for p in players:
            p.run(k) if kind is None else p.joy(kind, a[key], a[key + "_mask"], k)
        check(label, k)


def half_reset(ora, mask, pose7):
    """The half recipe: pose and twist rows of the mask through set_platform_state only; the Pids keep their past (mode, target,
    integral, derivative window, call count).  What a launch form that ignored the reset's call count would resemble."""
    m = np.asarray(mask).astype(bool)
    p, t = ora.raw_state()
    p[m] = np.asarray(pose7, dtype=np.float32).astype(np.float64)[m]
    t[m] = 0.0
    ora.set_platform_state(pose7=p, twist6=t)


def window_of(cfg):
    return max(cfg.velocityController.dBufferLength, cfg.positionController.dBufferLength)


def rollout_inputs(cfg, pose, seed):
    """cmds [B, H, SAMPLES, n] with H = nbuf + 3 (the window of a robot whose Pid starts at the rollout's first Joy fills inside the
    rollout), ref [B, 3] = `pose` plus (0, 0, 0.01)"""
    rng = np.random.default_rng(seed)
    H, n = window_of(cfg) + 3, cfg.n_cables
    cmds = (rng.uniform(-0.03, 0.03, (B, H, 1, n)) + rng.normal(0.0, 0.01, (B, H, SAMPLES, n))).astype(np.float32)
    return dict(cmds=cmds, ref=(pose[:, :3].astype(np.float32) + np.float32([0.0, 0.0, 0.01])).astype(np.float32))


def rollout_tolerance(cfg, general, oc):
    """the suite's own: test_gpu_fp64.test_fp64_rollout_on_per_robot_handles, test_gpu_general_matrix,
    test_gpu_parity.test_per_robot_rollout_record_and_fused_updates_against_the_oracle"""
    if cfg.precision == 64:
        return 3e-7 * float(np.abs(oc).max())
    return rollout_cost_tol(oc, 1e-9 if general else 1e-6)
