"""The fused closed loop with a deep tracking policy as the controller.

`run_policy_loop` and `evaluate_policy` mirror `rollout.run_closed_loop` and
`eval.evaluate_batched`: the same seeds, reset draws, metric accumulators and
numpy-exact summary, with `qt_policy_rollout` (csrc/qt_policy.hip: the
policy's f32 forward pass on the MFMA, then the exact env step, per step, in
one kernel) in place of the classical controllers' rollout.

`run_policy_population` / `evaluate_population` run many networks of one shape
(`PolicyPopulation`) in one launch, each member on its own episodes
(`qt_policy_population_rollout`, csrc/qt_policy_population.hip): the batch
evaluator of gradient-free search (`quadtrack.train.search_policy`).

`run_policy_supervised` flies the policy while a classical teacher labels
every visited state (`qt_policy_supervised_rollout`,
csrc/qt_policy_supervised.hip): the data source of imitation training
(`quadtrack.train.train_imitation`).

`imitation_gradient` is that training's loss and gradient on the forward
pass's MFMA path (`qt_policy_imitation_grad`, csrc/qt_policy_grad.hip): the
backward pass of `train_imitation(..., backend="hip")`.

`PolicyOptimizer` (controllers/deep.py) is that training's clip + optimiser
step and packing in one launch (`qt_policy_optim_step`) and a whole minibatch
pass enqueued by one call (`qt_policy_imitation_fit`,
csrc/qt_policy_optim.hip): `train_imitation(..., backend="hip_fused")`.
"""

from __future__ import annotations

import numpy as np
import torch

from . import _abi, core
from dataclasses import dataclass

from .controllers.deep import (BatchedDeepPolicy, DeepTrackingPolicy, PolicyOptimizer, PolicyPopulation,
                               extract_features, pack_index, pack_params, policy_tiles)
from .env.batched import motion_indices
from .env.config import as_env_config
from .rollout import F64, RolloutResult, _criteria, build_batch, max_steps_for
from .utils.metrics import EvaluationSummary, SuccessCriteria

__all__ = ["BatchedDeepPolicy", "DeepTrackingPolicy", "run_policy_loop", "evaluate_policy", "policy_batch",
           "pack_params", "policy_tiles", "extract_features", "PolicyPopulation", "PopulationResult", "pack_index",
           "run_policy_population", "evaluate_population", "run_policy_supervised", "SupervisedResult",
           "sample_steps", "imitation_gradient", "PolicyOptimizer"]


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


def imitation_gradient(policy, features, targets, index=None, weight: float = 1.0, *, grad=None, pred=None):
    """BatchedDeepPolicy.imitation_gradient for a BatchedDeepPolicy, a
    DeepTrackingPolicy or its config dict: (loss [1] float64, grad [flat_size]
    float32) of weight * F.mse_loss(network(features), targets) on the device
    (qt_policy_imitation_grad, csrc/qt_policy_grad.hip)."""
    return _as_batched(policy).imitation_gradient(features, targets, index, weight, grad=grad, pred=pred)


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


# ------------------------------------------------------------------ supervised rollout

def sample_steps(n: int, S: int, horizon: int, seed: int = 0) -> np.ndarray:
    """int32 [S, n]: the step indices at which each of n episodes fills its S
    sample slots.  Slot j is drawn uniformly from the stratum
    [floor(j H / S), floor((j + 1) H / S)) of the horizon H with
    np.random.default_rng(seed) (one [S, n] block of uniforms), so an
    episode's steps are ascending and distinct by construction and the result
    is a function of the four arguments only.  S > H is refused (a stratum
    would be empty).

    The reference's trainer draws an unseeded np.random.choice over the
    REALISED episode length after the episode (train.py:756-757).  Here the
    steps are fixed before the launch, over the horizon: an episode that ends
    early leaves its later slots unfilled (SupervisedResult.valid), and a run
    is reproducible from its seed."""
    n, S, H = int(n), int(S), int(horizon)
    if n < 0 or S < 0 or H < 0:
        raise ValueError(f"n, S and horizon must be >= 0, got {n}, {S}, {H}")
    if S > H:
        raise ValueError(f"{S} sample slots do not fit a horizon of {H} steps")
    j = np.arange(S, dtype=np.int64)
    lo, hi = j * H // max(S, 1), (j + 1) * H // max(S, 1)
    r = np.random.default_rng(seed).random((S, n))
    k = np.minimum(np.floor(r * (hi - lo)[:, None]).astype(np.int64), (hi - lo - 1)[:, None])
    return (lo[:, None] + k).astype(np.int32)


@dataclass
class SupervisedResult(RolloutResult):
    """A supervised run: run_policy_loop's result (the flight is the policy's,
    bit for bit) plus the teacher's labels."""

    loss: torch.Tensor | None = None            # [n] float64: sum over the flown steps of |u - fl32(s)|^2
    sample: torch.Tensor | None = None          # [S, 26, n] float32, NaN where a slot was not reached
    steps_sampled: torch.Tensor | None = None   # [S, n] int32: the slots' step indices (sample_steps)
    teacher_record: torch.Tensor | None = None  # [steps, 4, n] float64: the teacher's command at every step
    supervisor: object = None

    @property
    def features(self) -> torch.Tensor:
        """[S, n, 18] float32 view: the policy's input at the sampled steps."""
        return self.sample[:, :18].permute(0, 2, 1)

    @property
    def targets(self) -> torch.Tensor:
        """[S, n, 4] float32 view: the teacher's command, the imitation label."""
        return self.sample[:, 18:22].permute(0, 2, 1)

    @property
    def commands(self) -> torch.Tensor:
        """[S, n, 4] float32 view: the policy's own command at the sampled steps."""
        return self.sample[:, 22:26].permute(0, 2, 1)

    @property
    def valid(self) -> torch.Tensor:
        """[S, n] bool: the episode reached the slot's step (sample_steps < steps)."""
        return self.steps_sampled.to(F64) < self.state.acc[_abi.ACC_STEPS][None, :]

    def dataset(self):
        """(features [m, 18], targets [m, 4]): the valid pairs, compact, on the device."""
        v = self.valid
        return self.features[v], self.targets[v]

    def imitation_loss(self) -> torch.Tensor:
        """[n] float64: loss / (4 steps), the F.mse_loss of the episode's f32
        policy commands against its f32 labels over the WHOLE flown episode."""
        return self.loss / (4.0 * self.state.acc[_abi.ACC_STEPS])


def _as_supervisor(supervisor, config, device):
    if isinstance(supervisor, str):
        from .controllers import batched_controller

        return batched_controller(supervisor, config, device=device)
    if not all(hasattr(supervisor, k) for k in ("K", "k_cols", "ctrl", "per_episode")):
        raise TypeError(f"expected a BatchedRiccatiLQR, BatchedLQR or BatchedPID (or a controller type name), "
                        f"got {type(supervisor).__name__}")
    return supervisor


def run_policy_supervised(policy, supervisor="riccati_lqr", env_config=None, n: int | None = None, seeds=None,
                          motion=None, plant_mass=None, criteria=None, draws=None, max_steps: int | None = None,
                          chunk: int | None = None, record: bool = False, samples_per_episode: int = 32,
                          sample_seed: int = 0, teacher_record: bool = False,
                          supervisor_config: dict | None = None) -> SupervisedResult:
    """run_policy_loop with a classical teacher labelling every visited state
    (qt_policy_supervised_rollout, csrc/qt_policy_supervised.hip): the policy
    flies, the supervisor is asked what it would have commanded on the same
    observation, and the launch keeps the per-episode imitation loss and
    `samples_per_episode` (features, teacher command) pairs per episode.

    supervisor  a BatchedRiccatiLQR / BatchedLQR / BatchedPID (shared or
                per-episode gains), or a controller type name with
                supervisor_config (controllers.batched_controller).  A fresh
                supervisor per episode (integral zeroed at reset, train.py:669).
                Feed-forward supervisors are out of scope (ValueError).
    samples_per_episode, sample_seed  the slots' steps: sample_steps(n, S, max_steps, sample_seed)
    teacher_record  keep the teacher's FP64 command of every step ([steps, 4, n])
    The other arguments and the flight itself are run_policy_loop's."""
    policy = _as_batched(policy)
    sup = _as_supervisor(supervisor, supervisor_config, policy.device)
    if sup.ctrl.feedforward_enabled or getattr(sup, "ff", None) is not None:
        raise ValueError("feed-forward supervisors are out of scope of the supervised rollout")
    cfg = as_env_config(env_config)
    env = cfg.to_params()
    if n is None:
        n = sup.num_problems if sup.per_episode else (len(seeds) if seeds is not None else 1)
    batch = build_batch(sup, cfg, n, seeds=seeds, motion=motion, plant_mass=plant_mass, draws=draws,
                        device=policy.device, group_motion=False)
    crit = _criteria(criteria)
    st = core.RolloutState.empty(n, batch.device)
    core.validate(batch, st)
    total = max_steps if max_steps is not None else max_steps_for(env)
    step = chunk or total
    dev = batch.device
    S = int(samples_per_episode)
    steps_dev = torch.as_tensor(sample_steps(n, S, total, sample_seed), device=dev)
    nan = float("nan")
    sample = torch.full((S, _abi.SUP_ROWS, n), nan, dtype=torch.float32, device=dev)
    loss = torch.zeros(n, dtype=F64, device=dev)
    rec = torch.full((total, 16, n), nan, dtype=F64, device=dev) if record else None
    trec = torch.full((total, 4, n), nan, dtype=F64, device=dev) if teacher_record else None
    core.reset(env, batch, st)  # the teacher's integral rows too (PID: no previous observation time)
    done = 0
    while done < total:
        k = min(step, total - done)
        policy.rollout_supervised(env, sup.ctrl, crit, batch, st, k, loss, steps_dev if S else None,
                                  sample if S else None, None if rec is None else rec[done:done + k],
                                  None if trec is None else trec[done:done + k])
        done += k
    met = core.episode_metrics(crit, st)
    return SupervisedResult(metrics=met, state=st, batch=batch, criteria=crit, record=rec, env=env, ctrl=sup.ctrl,
                            policy=policy, loss=loss, sample=sample, steps_sampled=steps_dev, teacher_record=trec,
                            supervisor=sup)


# ------------------------------------------------------------------ populations

@dataclass
class PopulationResult(RolloutResult):
    """A population run: n = members * episodes_per_member compact columns,
    member m owning episodes [m E, (m + 1) E)."""

    population: PolicyPopulation | None = None
    members: int = 1
    episodes_per_member: int = 1

    def member_metrics(self) -> torch.Tensor:
        """The metrics as a [rows, M, E] view."""
        return self.metrics.view(self.metrics.shape[0], self.members, self.episodes_per_member)

    def member_summary(self, m: int) -> EvaluationSummary:
        """The numpy-exact EvaluationSummary of member m's episodes: what
        evaluate_policy gives for that member alone on the same episodes."""
        from .parallel import reduce_summary

        if not 0 <= int(m) < self.members:
            raise IndexError(f"member {m} of a population of {self.members}")
        E = self.episodes_per_member
        return reduce_summary(self.metrics[:, int(m) * E:(int(m) + 1) * E].contiguous(), self.criteria)

    def fitness(self, kind="tracking_error") -> torch.Tensor:
        """[M] device tensor, larger is better.  "tracking_error": minus the mean
        over a member's episodes of mean_tracking_error; "on_target": the mean
        on_target_ratio; a callable gets member_metrics() and returns [M]."""
        mm = self.member_metrics()
        if callable(kind):
            return kind(mm)
        if kind == "tracking_error":
            return -mm[_abi.MET["mean_tracking_error"]].mean(dim=1)
        if kind == "on_target":
            return mm[_abi.MET["on_target_ratio"]].mean(dim=1)
        raise ValueError(f"Unknown fitness: {kind}. Valid: 'tracking_error', 'on_target' or a callable")

    def trajectories(self, episodes=None) -> dict:
        raise ValueError("a population run keeps no single policy to re-run: use run_policy_loop on "
                         "population.member(m) for a member's trajectories")


def _per_member(values, M: int, E: int, what: str, convert) -> np.ndarray:
    """An [E] (shared by every member) or [M, E] input as n = M E values, member-major."""
    if isinstance(values, torch.Tensor):
        values = values.cpu().numpy()
    a = np.asarray(values)
    if a.shape == (M, E):
        return convert(a.reshape(-1), M * E)
    if a.shape == (E,):
        return np.tile(convert(a, E), M)
    raise ValueError(f"{what} must have shape [{E}] or [{M}, {E}], got {list(a.shape)}")


def run_policy_population(population: PolicyPopulation, env_config=None, episodes_per_member: int = 1, seeds=None,
                          motion=None, plant_mass=None, criteria=None, max_steps: int | None = None,
                          chunk: int | None = None, record: bool = False) -> PopulationResult:
    """Every member of the population on its own `episodes_per_member` episodes,
    in one fused launch (qt_policy_population_rollout): n = M E.

    seeds / motion / plant_mass take shape [E] or [M, E]; an [E] input is
    shared by every member (common random numbers).  Default seeds: 0..E-1 for
    each member.  The other arguments are run_policy_loop's.  A member's
    results are bit for bit those of run_policy_loop on population.member(m)
    with the same inputs."""
    if not isinstance(population, PolicyPopulation):
        raise TypeError(f"expected a PolicyPopulation, got {type(population).__name__}")
    M, E = population.members, int(episodes_per_member)
    if E < 1:
        raise ValueError("episodes_per_member must be >= 1")
    n = M * E
    cfg = as_env_config(env_config)
    env = cfg.to_params()
    ints = lambda a, k: np.asarray(a, dtype=np.int64).reshape(k)  # noqa: E731
    seeds = _per_member(np.arange(E) if seeds is None else seeds, M, E, "seeds", ints)
    if motion is not None:
        motion = _per_member(motion, M, E, "motion", motion_indices)
    if plant_mass is not None:
        plant_mass = _per_member(plant_mass, M, E, "plant_mass", lambda a, k: np.asarray(a, dtype=np.float64).reshape(k))
    batch = policy_batch(cfg, n, population.device, seeds=seeds, motion=motion, plant_mass=plant_mass)
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
        population.rollout(env, crit, batch, st, k, E, None if rec is None else rec[done:done + k])
        done += k
    met = core.episode_metrics(crit, st)
    return PopulationResult(metrics=met, state=st, batch=batch, criteria=crit, record=rec, env=env,
                            population=population, members=M, episodes_per_member=E)


def evaluate_population(population: PolicyPopulation, env_config=None, num_episodes: int = 10, base_seed: int = 42,
                        criteria: SuccessCriteria | None = None, motion=None, plant_mass=None,
                        max_steps_per_episode: int | None = None, with_episode_metrics: bool = True) -> list:
    """evaluate_policy's summary for every member, all members in one fused
    launch on the same episodes (seeds base_seed + i for each member)."""
    res = run_policy_population(population, env_config, episodes_per_member=num_episodes,
                                seeds=base_seed + np.arange(num_episodes), motion=motion, plant_mass=plant_mass,
                                criteria=criteria, max_steps=max_steps_per_episode)
    out = [res.member_summary(m) for m in range(population.members)]
    if with_episode_metrics:
        em = res.episode_metrics()
        for m, s in enumerate(out):
            s.episode_metrics = em[m * num_episodes:(m + 1) * num_episodes]
    return out
