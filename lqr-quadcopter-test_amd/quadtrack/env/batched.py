"""Batched quadcopter environment on the GPU.

`BatchedQuadcopterEnv(n, config)` holds n independent episodes in HBM and
exposes the reference's reset / step API (env/quadcopter_env.py:111-232) on
tensors.  Each call is one kernel launch (include/quadtrack.h ABI 9):

  reset(seeds)   qt_seed_draws + qt_frame_reset (numpy default_rng(seed)'s
                 draws on the device, quadcopter_env.py:111-150)
  step(actions)  qt_frame_step: action validation, RK4 / Euler, state
                 constraints, post-step tracking error, reward, termination,
                 info, for every episode (quadcopter_env.py:152-293)
  step_closed(controller)
                 qt_frame_closed_step: the controller's compute_action on the
                 current observation, then the step, in one launch (a
                 BatchedDeepPolicy: two launches, qt_policy_action then the step,
                 and a lean env's expand launch before them)

Every step writes an observation frame (quadtrack.step.Frame); the returned
observation / reward / done / info tensors are views of it.  No later step
writes a frame whose tensors the caller still holds (Frame.recyclable), so
what the caller keeps stays as it was, as the reference's observation arrays
are fresh copies (quadcopter_env.py:481-486); a loop that drops them cycles
through a small pool of frames.  The next step reads its state from the last
frame, so writing into the returned tensors in place would change the
environment: the env detects that (the views share one version counter) and
raises instead.

`lean=True` (ABI 10) runs the same calls on lean frames (qt_lean_reset /
qt_lean_step / qt_lean_closed_step: 286 B instead of 462 B per closed-loop
env-step) and builds what a lean frame does not hold on first use
(qt_lean_expand); see the class doc.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _abi, core
from .._abi import FB_DONE, FC_STEP, FR_X, MOTIONS, check, on_device, raw_stream
from ..controllers.deep import BatchedDeepPolicy
from ..step import Frame, FramePool, LeanFrame, LeanSource, TimeTable, action_tensor
from . import seeding
from .config import as_env_config

F64 = torch.float64


def motion_indices(motion, n: int) -> np.ndarray:
    """Per-episode motion names / indices -> int8 array of enum qt_motion."""
    if isinstance(motion, (np.ndarray, torch.Tensor)) and not (isinstance(motion, np.ndarray)
                                                                and motion.dtype.kind in "UOS"):
        a = np.asarray(motion.cpu() if isinstance(motion, torch.Tensor) else motion).reshape(-1)
        if a.size != n:
            raise ValueError(f"{a.size} motion types for {n} episodes")
        if a.size and (a.min() < 0 or a.max() >= len(MOTIONS)):
            raise ValueError(f"Invalid motion type index in {sorted(set(a.tolist()))[:8]}")
        return a.astype(np.int8)
    out = np.empty(n, dtype=np.int8)
    vals = list(motion)
    if len(vals) != n:
        raise ValueError(f"{len(vals)} motion types for {n} episodes")
    for i, m in enumerate(vals):
        if isinstance(m, str):
            if m.lower() not in MOTIONS:
                raise ValueError(f"Invalid motion type: {m}. Valid types: {set(MOTIONS)}")
            out[i] = MOTIONS.index(m.lower())
        else:
            if not 0 <= int(m) < len(MOTIONS):
                raise ValueError(f"Invalid motion type index: {m}")
            out[i] = int(m)
    return out


class BatchedQuadcopterEnv:
    """n QuadcopterEnv episodes stepped together.

    motion      per-episode motion types (names or enum indices; default the config's)
    mass        per-episode plant mass (default the config's)
    freeze_done True (default): an episode that is done is not stepped again,
                its observation and info stay those of its last step (the
                Evaluator stops stepping at done, eval.py:119-165); False:
                every episode is stepped on every call, as the reference's
                env steps after done.
    lean        False (default): every step writes a full observation frame
                (229 B per episode).  True: steps read and write lean frames
                (quadtrack.step.LeanFrame: state, reward, counters, flags,
                121 B per episode; qt_lean_* of ABI 10) with the same results
                bit for bit.  reward, done, info["action"] and
                obs["quadcopter"] are served from the lean frame; the first
                read of anything else a step returned (obs["target"],
                obs["time"], obs.frame, any other info value) expands that
                step's full frame, one launch (`expand_launches` counts them).
    """

    STATE_DIM = 12
    ACTION_DIM = 4

    def __init__(self, num_envs: int, config=None, device=None, motion=None, mass=None, freeze_done: bool = True,
                 lean: bool = False):
        if num_envs < 0:
            raise ValueError("num_envs must be >= 0")
        self.config = as_env_config(config)
        self.params = self.config.to_params()
        self.num_envs = int(num_envs)
        self.device = _abi.require_gpu(device)
        self.freeze_done = bool(freeze_done)
        n, dev = self.num_envs, self.device
        self.motion = None
        if motion is not None:
            self.motion = torch.as_tensor(motion_indices(motion, n), device=dev)
        self.plant_mass = None if mass is None else core.to_device(np.broadcast_to(np.asarray(mass, float), (n,)), dev)
        self.pattern: torch.Tensor | None = None
        self.offset: torch.Tensor | None = None
        self._frame: Frame | None = None
        self.lean = bool(lean)
        self._pool = FramePool(self.num_envs, self.device, kind=LeanFrame if self.lean else None)  # the frames steps write
        self._expands = [0]  # qt_lean_expand launches (LeanSource.count)
        if self.lean:
            # the time table (quadtrack.h ABI 10): an episode's length in steps plus slack; extended on demand
            p = self.params
            self._table = TimeTable(p.dt, int(np.ceil(p.max_episode_time / p.dt)) + 3, dev)
            self._steps = 0  # steps since reset: the bound on every episode's step count
            self._source: LeanSource | None = None
        self._env_ref = C.byref(self.params)
        self._batch = None
        self._closed = None  # (controller, its qt_batch, byref) of step_closed

    # ---------------------------------------------------------------- reset
    def reset_from_draws(self, pattern, offset):
        """Reset every episode from explicit draws: pattern [4, n], offset [3, n]."""
        n, dev = self.num_envs, self.device
        self.pattern = core.to_device(pattern, dev)
        self.offset = core.to_device(offset, dev)
        core._check_cols("pattern", self.pattern, 4, n)
        core._check_cols("offset", self.offset, 3, n)
        b = _abi.Batch()
        b.n = n
        b.motion = None if self.motion is None else self.motion.data_ptr()
        b.pattern = self.pattern.data_ptr()
        b.plant_mass = None if self.plant_mass is None else self.plant_mass.data_ptr()
        self._batch = b
        self._batch_ref = C.byref(b)
        self._closed = None
        self._frame = None
        fr = self._next_frame()
        reset = _abi.load().qt_lean_reset if self.lean else _abi.load().qt_frame_reset
        with torch.cuda.device(dev):
            check(reset(self._env_ref, self._batch_ref, self.offset.data_ptr(), fr.ptr, raw_stream(dev)),
                  "qt_lean_reset" if self.lean else "qt_frame_reset")
        self._frame = fr.seal()
        if self.lean:
            self._steps = 0
            self._source = LeanSource(self._env_ref, self._batch_ref,
                                      (self.params, b, self.pattern, self.motion, self.plant_mass), self._table, dev,
                                      self._expands)
            return fr.observation(self._source)
        return fr.observation()

    def reset(self, seeds=None):
        """QuadcopterEnv.reset(seed) for every episode: seeds [n] (default
        config.seed + arange(n)).  Returns the observation dict ([n, 3] tensors)."""
        if seeds is None:
            seeds = self.config.seed + np.arange(self.num_envs)
        seeds = np.asarray(seeds.cpu() if isinstance(seeds, torch.Tensor) else seeds, dtype=np.int64).reshape(-1)
        if seeds.size != self.num_envs:
            raise ValueError(f"{seeds.size} seeds for {self.num_envs} episodes")
        kinds = self.motion if self.motion is not None else self.config.motion_index()
        pat, off = seeding.draws(kinds, seeds, self.device)
        return self.reset_from_draws(pat, off)

    # ----------------------------------------------------------------- step
    def _next_frame(self) -> Frame:
        """The frame the next step writes (FramePool.take: never one the caller
        holds, nor the current one, which the step reads)."""
        return self._pool.take(self._frame)

    def _current(self) -> Frame:
        fr = self._frame
        if fr is None:
            raise RuntimeError("Environment not initialized. Call reset() first.")
        fr.check_intact()
        return fr

    def step(self, actions):
        """actions [n, 4] (thrust, roll, pitch, yaw rates; any strides, e.g. a
        controller's output) or a dict of [n] tensors -> (obs, reward [n],
        done [n] bool, info dict of [n] tensors)."""
        fr = self._current()
        n, dev = self.num_envs, self.device
        a = action_tensor(actions, n, dev)
        if self.lean:
            return self._lean_step(fr, a)
        out = self._next_frame()
        with on_device(dev):
            check(_abi.load().qt_frame_step(self._env_ref, self._batch_ref, fr.ptr,
                                            _abi.View(a.data_ptr(), a.stride(1), a.stride(0)), out.ptr,
                                            int(self.freeze_done), raw_stream(dev)), "qt_frame_step")
        self._frame = out.seal()
        return out.step_result()

    def step_closed(self, controller):
        """One closed-loop step in ONE launch: `controller.compute_action` on
        the current observation, then `step` with its command
        (qt_frame_closed_step).  Same results as
        `env.step(controller.compute_action(obs))`; info["action"] holds the
        command ([n, 4]).  With freeze_done, a done episode's controller state
        is not advanced.  A BatchedDeepPolicy takes two launches instead
        (qt_policy_action on the observation, then the step), three on a lean
        env, whose target observation the policy reads and which is therefore
        expanded first (qt_lean_expand); the results are those of
        `env.step(policy.compute_action(obs))` bit for bit."""
        fr = self._current()
        n, dev = self.num_envs, self.device
        if controller.device != dev:
            raise ValueError(f"the controller is on {controller.device}, the environment on {dev}")
        if isinstance(controller, BatchedDeepPolicy):
            return self._step_policy(fr, controller)
        cb = self._closed_batch(controller)
        integ = controller._state_for(n)
        if self.lean:
            return self._lean_step_closed(fr, controller, cb, integ)
        out = self._next_frame()
        with on_device(dev):
            check(_abi.load().qt_frame_closed_step(
                self._env_ref, controller._ctrl_ref, cb, fr.ptr, None if integ is None else integ.data_ptr(),
                out.ptr, out.act_ptr, int(self.freeze_done), raw_stream(dev)), "qt_frame_closed_step")
        self._frame = out.seal()
        return out.step_result(with_action=True)

    def _step_policy(self, fr, policy):
        """step_closed with a deep policy: its action launch on the current
        observation, then the step launch.  With freeze_done a done episode's
        action row is 0, as the one-launch closed step gives it.  The policy
        reads the target's position and velocity, which a lean frame does not
        hold: on a lean env the observation is expanded first (one more launch
        and the full frame's bytes per step; `expand_launches` counts it)."""
        a = policy.compute_action(self.observation(), fr.b[FB_DONE] if self.freeze_done else None)
        obs, reward, done, info = self.step(a)
        info["action"] = a
        return obs, reward, done, info

    def _lean_step(self, fr: LeanFrame, a: torch.Tensor):
        """step on lean frames (qt_lean_step)."""
        dev, tab = self.device, self._table
        tab.cover(self._steps)
        out = self._next_frame()
        with on_device(dev):
            check(_abi.load().qt_lean_step(self._env_ref, self._batch_ref, tab.ptr, tab.len, self._steps, fr.ptr,
                                           _abi.View(a.data_ptr(), a.stride(1), a.stride(0)), out.ptr,
                                           int(self.freeze_done), raw_stream(dev)), "qt_lean_step")
        self._steps += 1
        self._frame = out.seal()
        return out.step_result(self._source)

    def _lean_step_closed(self, fr: LeanFrame, controller, cb, integ):
        """step_closed on lean frames (qt_lean_closed_step)."""
        dev, tab = self.device, self._table
        tab.cover(self._steps)
        out = self._next_frame()
        with on_device(dev):
            check(_abi.load().qt_lean_closed_step(
                self._env_ref, controller._ctrl_ref, cb, tab.ptr, tab.len, self._steps, fr.ptr,
                None if integ is None else integ.data_ptr(), out.ptr, out.act_ptr, int(self.freeze_done),
                raw_stream(dev)), "qt_lean_closed_step")
        self._steps += 1
        self._frame = out.seal()
        return out.step_result(self._source, with_action=True)

    @property
    def expand_launches(self) -> int:
        """qt_lean_expand launches since construction (0 for a default env)."""
        return self._expands[0]

    def _closed_batch(self, controller):
        """qt_batch of the env's episodes with the controller's gains (cached)."""
        controller.c_batch(self.num_envs)
        key = (controller, controller._cb)
        if self._closed is None or self._closed[0] != key:
            b = _abi.Batch()
            C.memmove(C.addressof(b), C.addressof(controller._cb), C.sizeof(b))  # gains, hover, feed-forward
            b.n = self.num_envs
            b.motion, b.pattern, b.plant_mass = self._batch.motion, self._batch.pattern, self._batch.plant_mass
            self._closed = (key, b, C.byref(b))
        return self._closed[2]

    # ---------------------------------------------------------- observation
    def observation(self) -> dict:
        """The current observation (views of the last frame)."""
        fr = self._current()
        return fr.observation(self._source) if self.lean else fr.observation()

    @property
    def done(self) -> torch.Tensor:
        return self._current().b[FB_DONE].view(torch.bool)

    def get_state_vector(self) -> torch.Tensor:
        return self._current().f[FR_X:FR_X + 12].T.clone()

    def set_state_vector(self, x) -> None:
        """Replace every episode's 12-state (the observation after this call sees it)."""
        fr = self._current()
        x = torch.as_tensor(x, dtype=F64, device=self.device)
        if x.shape != (self.num_envs, self.STATE_DIM):
            raise ValueError(f"State must have shape ({self.num_envs}, {self.STATE_DIM}), got {tuple(x.shape)}")
        out = (LeanFrame if self.lean else Frame)(self.num_envs, self.device)
        out.buf.copy_(fr.buf)
        out.f[FR_X:FR_X + 12].copy_(x.T)
        self._frame = out.seal()

    @property
    def frame(self) -> Frame:
        """The last step's Frame (a lean env expands it on first use)."""
        fr = self._current()
        return self._source.frame_of(fr) if self.lean else fr

    @property
    def time(self) -> torch.Tensor:
        fr = self._current()
        if self.lean:  # an episode's time is the table's entry at its step count
            return self._table.dev[fr.c[FC_STEP].long()]
        return fr.f[_abi.FR_TIME].clone()

    @property
    def dt(self) -> float:
        return self.config.simulation.dt
