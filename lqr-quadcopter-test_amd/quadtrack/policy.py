"""The fused closed loop with a deep tracking policy as the controller.

`run_policy_loop` and `evaluate_policy` mirror `rollout.run_closed_loop` and
`eval.evaluate_batched`: the same seeds, reset draws, metric accumulators and
numpy-exact summary, with `qt_policy_rollout` (csrc/qt_policy.hip: the
policy's f32 forward pass on the MFMA, then the exact env step, per step, in
one kernel) in place of the classical controllers' rollout.
"""

from __future__ import annotations

import numpy as np
import torch

from . import _abi, core
from .controllers.deep import BatchedDeepPolicy, DeepTrackingPolicy, extract_features, pack_params, policy_tiles
from .env.config import as_env_config
from .rollout import F64, RolloutResult, _criteria, build_batch, max_steps_for
from .utils.metrics import EvaluationSummary, SuccessCriteria

__all__ = ["BatchedDeepPolicy", "DeepTrackingPolicy", "run_policy_loop", "evaluate_policy", "policy_batch",
           "pack_params", "policy_tiles", "extract_features"]


class _NoGains:
    """The controller half of an EpisodeBatch for a run without a classical
    controller: the batch containers want a gain tensor, the policy rollout
    never reads it (qt_policy_rollout takes batch->K = NULL)."""

    per_episode = False
    num_problems = 1
    k_cols = 6
    k_structured = False
    hover = None

    def __init__(self, device):
        self.device = device
        self.K = torch.zeros(24, 1, dtype=F64, device=device)


def policy_batch(env_config, n: int, device, seeds=None, motion=None, plant_mass=None, draws=None) -> core.EpisodeBatch:
    """Device inputs of `n` episodes for the policy rollout: build_batch's reset
    draws, motions and plant masses, in episode order (no motion grouping)."""
    return build_batch(_NoGains(_abi.require_gpu(device)), as_env_config(env_config), n, seeds=seeds, motion=motion,
                       plant_mass=plant_mass, draws=draws, group_motion=False)


def _as_batched(policy) -> BatchedDeepPolicy:
    if isinstance(policy, DeepTrackingPolicy):
        return policy.to_batched()
    if isinstance(policy, dict):
        return DeepTrackingPolicy(policy).to_batched()
    if not isinstance(policy, BatchedDeepPolicy):
        raise TypeError(f"expected a DeepTrackingPolicy, a BatchedDeepPolicy or a config dict, got {type(policy).__name__}")
    return policy


def run_policy_loop(policy, env_config=None, n: int | None = None, seeds=None, motion=None, plant_mass=None,
                    criteria=None, draws=None, max_steps: int | None = None, chunk: int | None = None,
                    record: bool = False) -> RolloutResult:
    """Run `n` closed-loop episodes of the policy to termination (or `max_steps`).

    policy    a BatchedDeepPolicy, a DeepTrackingPolicy or its config dict
    seeds     per-episode reset seeds (default 0..n-1); draws=(pattern, offset) overrides them
    motion    per-episode motion types (default: the config's)
    plant_mass per-episode plant mass
    criteria  the Evaluator's SuccessCriteria (default utils.metrics defaults)
    chunk     steps per kernel launch (default: the whole episode in one launch)
    record    keep every step's state and the policy's command ([steps, 16, n])

    The result's trajectories() / episode_data() re-run the selected episodes
    through the policy rollout with recording on."""
    policy = _as_batched(policy)
    cfg = as_env_config(env_config)
    env = cfg.to_params()
    if n is None:
        n = len(seeds) if seeds is not None else 1
    batch = policy_batch(cfg, n, policy.device, seeds=seeds, motion=motion, plant_mass=plant_mass, draws=draws)
    crit = _criteria(criteria)
    st = core.RolloutState.empty(n, batch.device)
    core.validate(batch, st)
    total = max_steps if max_steps is not None else max_steps_for(env)
    step = chunk or total
    rec = torch.full((total, 16, n), float("nan"), dtype=F64, device=batch.device) if record else None
    core.reset(env, batch, st)
    done = 0
    while done < total:
        k = min(step, total - done)
        policy.rollout(env, crit, batch, st, k, None if rec is None else rec[done:done + k])
        done += k
    met = core.episode_metrics(crit, st)
    return RolloutResult(metrics=met, state=st, batch=batch, criteria=crit, record=rec, env=env, policy=policy)


def evaluate_policy(policy, env_config=None, num_episodes: int = 10, base_seed: int = 42,
                    criteria: SuccessCriteria | None = None, motion=None, plant_mass=None,
                    max_steps_per_episode: int | None = None, with_episode_metrics: bool = True,
                    group=None, global_offset: int = 0) -> EvaluationSummary:
    """Evaluator.evaluate's summary (eval.py:170-268) for the policy, every
    episode in one fused launch: seeds base_seed + i, as evaluate_batched."""
    seeds = base_seed + global_offset + np.arange(num_episodes)
    res = run_policy_loop(policy, env_config, n=num_episodes, seeds=seeds, motion=motion, plant_mass=plant_mass,
                          criteria=criteria, max_steps=max_steps_per_episode)
    summary = res.summary(group=group, global_offset=global_offset)
    if with_episode_metrics:
        summary.episode_metrics = res.episode_metrics()
    return summary
