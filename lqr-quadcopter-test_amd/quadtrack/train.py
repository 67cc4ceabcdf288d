"""The trainer's classical evaluation epoch on the fused device rollout.

Reference: `Trainer._evaluate_epoch` (train.py:578-652), which the trainer
runs instead of a training epoch for the classical controllers (PID, LQR,
Riccati-LQR; train.py:394-429): episodes_per_epoch episodes, reset seeds
`env_seed + epoch * 1000 + episode`, `controller.reset()` before each (a fresh
controller per episode), at most max_steps_per_episode env steps, and per
episode the sum of env.step's rewards (-post-step tracking error,
quadcopter_env.py:198-199, 504-511) and the last step's info on-target ratio
and tracking error (quadcopter_env.py:205-220); the epoch returns their
np.mean and difficulty 1.0.

Here every episode of the epoch runs in one exact-step rollout launch
(`qt_rollout_rewards`, which keeps the reward sum and the last post-step error
per episode) and the three means are numpy's, bit for bit, from the
block-pairwise summary kernel (`qt_summary_numpy`).  The env is built as the
Trainer builds it (train.py:306-312): EnvConfig defaults with the
TrainingConfig's seed, episode length, motion type and target radius.
`train_imitation` is the trainer's imitation mode (train.py:654-862) on the
supervised rollout: per epoch one fused launch in which the policy flies and a
classical supervisor labels every visited state, then torch autograd (or, with
backend="hip", the HIP backward pass of csrc/qt_policy_grad.hip) on the
sampled (features, label) pairs.  The trainer's other modes are out of scope.
`search_policy` is a gradient-free counterpart on the population rollout:
evolution strategies over a policy's flat weight vector, one fused launch of
every candidate per generation.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _abi, core
from .controllers import batched_controller
from .env.config import EnvConfig

F64 = torch.float64

CLASSICAL = ("pid", "lqr", "riccati_lqr")


@dataclass
class EpochResult:
    """`_evaluate_epoch`'s dict plus the per-episode values it averages."""

    mean_reward: float
    mean_on_target_ratio: float
    mean_tracking_error: float
    difficulty: float
    episode_reward: torch.Tensor           # [E] sum of rewards
    episode_on_target_ratio: torch.Tensor  # [E] last step's info["on_target_ratio"]
    episode_tracking_error: torch.Tensor   # [E] last step's info["tracking_error"]
    episode_steps: torch.Tensor            # [E] env steps taken

    def as_dict(self) -> dict:
        return {"mean_reward": self.mean_reward, "mean_on_target_ratio": self.mean_on_target_ratio,
                "mean_tracking_error": self.mean_tracking_error, "difficulty": self.difficulty}


def env_config_for(env_seed=42, target_motion_type="circular", episode_length=30.0, target_radius=0.5) -> EnvConfig:
    """The Trainer's env (train.py:306-312)."""
    return EnvConfig.from_dict({"seed": env_seed, "simulation": {"max_episode_time": episode_length},
                                "target": {"motion_type": target_motion_type},
                                "success_criteria": {"target_radius": target_radius}})


def _np_means(rows: torch.Tensor) -> list[float]:
    """np.mean of each of three [3, E] device rows, bit for bit: the
    qt_summary_numpy kernel sums (numpy's block-pairwise order) of a
    metrics-shaped tensor carrying the rows in its three summed slots."""
    n = rows.shape[1]
    met = torch.zeros(_abi.MET_ROWS, n, dtype=F64, device=rows.device)
    met[_abi.MET["on_target_ratio"]] = rows[0]
    met[_abi.MET["mean_tracking_error"]] = rows[1]
    met[_abi.MET["mean_control_effort"]] = rows[2]
    blocks = core.summary_numpy_blocks(met, 0).cpu().numpy()
    return [core.np_fold(blocks[i]) / n for i in range(3)]


def evaluate_epoch(config=None, epoch: int = 0, *, controller: str = "riccati_lqr",
                   controller_config: dict | None = None, episodes_per_epoch: int = 10,
                   max_steps_per_episode: int = 3000, env_seed: int = 42, target_motion_type: str = "circular",
                   episode_length: float = 30.0, target_radius: float = 0.5, device=None) -> EpochResult:
    """One classical evaluation epoch (train.py:578-652) in one launch.

    `config` may be a TrainingConfig-like object (attributes controller,
    episodes_per_epoch, max_steps_per_episode, env_seed, target_motion_type,
    episode_length, target_radius and optionally full_config, whose entry
    under the controller type holds its settings, train.py:394-429); the
    keyword arguments are used otherwise."""
    if config is not None:
        controller = config.controller
        episodes_per_epoch = config.episodes_per_epoch
        max_steps_per_episode = config.max_steps_per_episode
        env_seed, target_motion_type = config.env_seed, config.target_motion_type
        episode_length, target_radius = config.episode_length, config.target_radius
        controller_config = dict(getattr(config, "full_config", {}) or {}).get(controller, {})
    if controller not in CLASSICAL:
        raise ValueError(f"evaluation epochs run the classical controllers {CLASSICAL}, not '{controller}'")
    if episodes_per_epoch < 1 or max_steps_per_episode < 1:
        raise ValueError("episodes_per_epoch and max_steps_per_episode must be >= 1")
    dev = _abi.require_gpu(device)
    cfg = env_config_for(env_seed, target_motion_type, episode_length, target_radius)
    env = cfg.to_params()
    ctl = batched_controller(controller, dict(controller_config or {}), device=dev)
    seeds = env_seed + epoch * 1000 + np.arange(episodes_per_epoch)
    from .rollout import build_batch

    batch = build_batch(ctl, cfg, episodes_per_epoch, seeds=seeds)
    st = core.RolloutState.empty(episodes_per_epoch, dev)
    core.validate(batch, st)
    core.reset(env, batch, st)
    reward = torch.zeros(2, episodes_per_epoch, dtype=F64, device=dev)
    crit = core.criteria(target_radius=target_radius)
    core.rollout_rewards(env, ctl.ctrl, crit, batch, st, int(max_steps_per_episode), reward)
    steps = st.acc[_abi.ACC_STEPS]
    ratio = st.acc[_abi.ACC_ON_POST] / steps  # on_target_count / total_steps (quadcopter_env.py:215-219)
    mean_ratio, mean_err, mean_reward = _np_means(torch.stack([ratio, reward[1], reward[0]]))
    return EpochResult(mean_reward=mean_reward, mean_on_target_ratio=mean_ratio, mean_tracking_error=mean_err,
                       difficulty=1.0, episode_reward=reward[0].clone(), episode_on_target_ratio=ratio,
                       episode_tracking_error=reward[1].clone(), episode_steps=steps.to(torch.int64))


# ------------------------------------------------------------------ imitation training

@dataclass
class ImitationResult:
    """train_imitation's history (host tensors, one entry per epoch) and the trained weights."""

    mean_reward: torch.Tensor            # [E] the three means of _train_epoch's dict (train.py:737-749)
    mean_on_target_ratio: torch.Tensor   # [E]
    mean_tracking_error: torch.Tensor    # [E]
    imitation_loss: torch.Tensor         # [E] mean over the episodes of SupervisedResult.imitation_loss()
    dataset_loss_before: torch.Tensor    # [E] imitation_weight * mse over the epoch's data set, before its updates
    dataset_loss_after: torch.Tensor     # [E] the same after them
    dataset_size: torch.Tensor           # [E] int64 valid (features, target) pairs
    state_dict: dict                     # the final weights (host), also loaded into policy.network
    policy: object                       # the DeepTrackingPolicy that was trained
    datasets: list | None = None         # keep_datasets: per epoch (features [m, 18], targets [m, 4]) on the device


def _make_optimizer(name: str, params, learning_rate: float, weight_decay: float):
    """Trainer._create_optimizer (train.py:476-500)."""
    name = name.lower()
    if name == "adam":
        return torch.optim.Adam(params, lr=learning_rate, weight_decay=weight_decay)
    if name == "sgd":
        return torch.optim.SGD(params, lr=learning_rate, weight_decay=weight_decay, momentum=0.9)
    if name == "adamw":
        return torch.optim.AdamW(params, lr=learning_rate, weight_decay=weight_decay)
    raise ValueError(f"Unknown optimizer: {name}")


def train_imitation(policy, supervisor="riccati_lqr", supervisor_config: dict | None = None, env_config=None, *,
                    epochs: int, episodes_per_epoch: int, samples_per_episode: int = 32, batch_size: int = 256,
                    learning_rate: float = 1e-3, optimizer: str = "adam", grad_clip: float = 1.0,
                    imitation_weight: float = 1.0, weight_decay: float = 0.0, env_seed: int = 42, seed: int = 0,
                    max_steps: int | None = None, motion=None, keep_datasets: bool = False,
                    device=None, backend: str = "torch") -> ImitationResult:
    """Imitation training of a DeepTrackingPolicy on the supervised rollout
    (the imitation mode of the reference's trainer, train.py:654-862).

    Per epoch e: ONE fused launch (policy.run_policy_supervised) flies
    `episodes_per_epoch` episodes of the current policy on the trainer's reset
    seeds env_seed + e * 1000 + j (train.py:662) while the supervisor labels
    every visited state, and keeps `samples_per_episode` (features, teacher
    command) pairs per episode at the steps sample_steps(..., seed + e).  Then
    minibatch steps of torch autograd (one pass over the epoch's data set in a
    seeded random order, `batch_size` pairs per step) minimise
    imitation_weight * F.mse_loss(net(features), targets), with the trainer's
    optimisers (train.py:476-500) and clip_grad_norm_ (train.py:831-834;
    grad_clip <= 0: none).  The forward pass is policy.network's own modules
    followed by the sigmoid / output-bounds stage; the new weights are packed
    again for the next epoch's launch and stay in policy.network.

    The reference updates once per EPISODE from an unseeded sample of that
    episode's steps; here the update follows the epoch's launch and its order
    is a function of `seed`.  mean_reward is the epoch mean of minus the sum of
    an episode's post-step tracking errors, formed from the rollout's
    accumulators (sum of pre-step errors - the first + the last post-step one).

    backend="torch" (the default) computes loss and gradient with torch's
    modules and autograd.  backend="hip" computes them with
    qt_policy_imitation_grad (csrc/qt_policy_grad.hip) on the rollout's own
    MFMA forward pass, at exactly the commands the rollout flies: per
    minibatch one device gather of the current parameters into the packed
    block (pack_index), one call of the gradient entry with the minibatch's
    index into the epoch's data set (no index_select copies), each
    parameter's .grad a view of the flat gradient, then the same
    clip_grad_norm_ and torch optimiser; dataset_loss_before / after come from
    the same entry over the whole data set.  Nothing in the minibatch loop
    synchronises with the host.  The epoch's rollout, seeds and sampling are
    the same under every backend.

    backend="hip_fused" keeps the parameters, the optimiser state and the
    packed block on the device in a PolicyOptimizer and runs the epoch's whole
    minibatch pass as ONE call of qt_policy_imitation_fit
    (csrc/qt_policy_optim.hip): per minibatch the gradient entry's three
    launches and one launch that clips, steps the optimiser and repacks the
    block, enqueued from C with no Python in between.  The same launch, seeds,
    sampling, randperm order and dataset_loss_before / after as backend="hip";
    the update's arithmetic is torch's formulas in f32 with the norm summed in
    a fixed order, so the weights agree with backend="hip" to rounding, not
    bit for bit.  The weights are copied back into policy.network at the end.
    Measured per minibatch on 65,536 pairs (scripts/bench_policy.py --fit,
    profiles/r17/policy_fit.jsonl): [64, 64] at batch 256 0.067 ms against
    0.226 ms for backend="hip" and 0.618 ms for backend="torch"; at batch
    4,096 0.085 / 0.231 / 0.627 ms; [128, 128, 128, 128] at batch 256 0.344 /
    0.348 / 0.794 ms (the one-workgroup step takes 0.055 ms there: a tie).

    Out of scope: the tracking and control-effort terms of utils/losses.py
    (tracking_weight is taken as 0), curriculum, diagnostics, NaN recovery,
    checkpoint cadence, the reward_weighted mode, learning-rate schedules,
    graph capture of the fused pass, a population form of the gradient or of
    the optimiser, reading the
    rollout's [S][26][n] sample block in place (the valid pairs are compacted
    first), and an exact host model of the gradient's summation order."""
    from .controllers.deep import (BatchedDeepPolicy, DeepTrackingPolicy, PolicyOptimizer, PolicyPopulation, _bounds,
                                   flat_size, policy_tiles, unflatten)
    from .policy import _as_supervisor, run_policy_supervised

    if not isinstance(policy, DeepTrackingPolicy):
        raise TypeError(f"expected a DeepTrackingPolicy, got {type(policy).__name__}")
    if backend not in ("torch", "hip", "hip_fused"):
        raise ValueError(f"Unknown backend: {backend}. Valid: 'torch', 'hip', 'hip_fused'")
    if epochs < 1 or episodes_per_epoch < 1 or batch_size < 1 or samples_per_episode < 1:
        raise ValueError("epochs, episodes_per_epoch, samples_per_episode and batch_size must be >= 1")
    net = policy.network
    opt_probe = _make_optimizer(optimizer, [torch.nn.Parameter(torch.zeros(1))], learning_rate, weight_decay)
    del opt_probe  # an unknown optimizer is refused before any GPU work
    dev = _abi.require_gpu(device if device is not None else (policy.device if policy.device.type == "cuda" else None))
    sup = _as_supervisor(supervisor, supervisor_config, dev)
    home = next(net.parameters()).device
    net.to(dev)
    opt = _make_optimizer(optimizer, list(net.parameters()), learning_rate, weight_decay)
    _, lo, hi = _bounds(net.output_bounds)
    scale = torch.tensor([h - l for l, h in zip(lo, hi)], dtype=torch.float32, device=dev)  # (float)(hi - lo)
    low = torch.tensor(lo, dtype=torch.float32, device=dev)

    def forward(f):  # PolicyNetwork.forward (deep_tracking_policy.py): sigmoid(raw) * (hi - lo) + lo
        return torch.sigmoid(net.output_layer(net.feature_extractor(f))) * scale + low

    def mse(f, y):
        return imitation_weight * torch.nn.functional.mse_loss(forward(f), y)

    hip = None
    if backend == "hip":
        sizes, params = list(net.hidden_sizes), list(net.parameters())
        gather, _ = PolicyPopulation._device_index(sizes, dev)
        src = torch.zeros(flat_size(sizes) + 1, dtype=torch.float32, device=dev)  # [theta, the padding's zero]
        block = torch.empty(_abi.policy_block_floats(len(sizes), policy_tiles(sizes)), dtype=torch.float32, device=dev)
        flat_grad = torch.zeros(flat_size(sizes), dtype=torch.float32, device=dev)
        hip = BatchedDeepPolicy.from_block(block, sizes, net.activation_name, net.output_bounds)
        views = unflatten(flat_grad, sizes)
        grad_views = [views[name] for name, _ in net.named_parameters()]

        def pack():  # the current parameters into the packed block: one device gather
            with torch.no_grad():
                torch.cat([p.reshape(-1) for p in params], out=src[:-1])
                torch.index_select(src, 0, gather, out=block)

        def hip_loss(f, y):
            pack()
            return hip.imitation_gradient(f, y, None, imitation_weight, grad=flat_grad)[0][0]

    fused = None
    if backend == "hip_fused":
        fused = PolicyOptimizer(policy, optimizer, learning_rate, weight_decay, grad_clip, device=dev)
        hip = fused.policy
        flat_grad = torch.empty(flat_size(list(net.hidden_sizes)), dtype=torch.float32, device=dev)

        def hip_loss(f, y):  # the optimiser's block already holds the current parameters
            return hip.imitation_gradient(f, y, None, imitation_weight, grad=flat_grad)[0][0]

    hist = {k: [] for k in ("reward", "ratio", "err", "imit", "before", "after", "size")}
    datasets = [] if keep_datasets else None
    gen = torch.Generator(device=dev)
    try:
        for e in range(epochs):
            E = int(episodes_per_epoch)
            res = run_policy_supervised(hip if fused is not None else policy.to_batched(dev), sup, env_config, n=E,
                                        seeds=generation_seeds(env_seed, e, E), motion=motion, max_steps=max_steps,
                                        samples_per_episode=samples_per_episode, sample_seed=seed + e)
            st = res.state
            steps = st.acc[_abi.ACC_STEPS]
            d = st.x[0:3] - st.target[0:3]
            last = torch.sqrt((d * d).sum(dim=0))  # the last step's info["tracking_error"]
            first = torch.sqrt((res.batch.offset * res.batch.offset).sum(dim=0))
            hist["reward"].append(-(st.acc[_abi.ACC_SUM_ERR] - first + last).mean())
            hist["ratio"].append((st.acc[_abi.ACC_ON_POST] / steps).mean())
            hist["err"].append(last.mean())
            hist["imit"].append(res.imitation_loss().mean())
            feats, targets = res.dataset()
            if keep_datasets:
                datasets.append((feats, targets))
            m = feats.shape[0]
            hist["size"].append(torch.tensor(m))
            if hip is not None:
                feats, targets = feats.contiguous(), targets.contiguous()
                hist["before"].append(hip_loss(feats, targets))
            else:
                with torch.no_grad():
                    hist["before"].append(mse(feats, targets).to(torch.float64))
            gen.manual_seed(int(seed) + e)
            order = torch.randperm(m, generator=gen, device=dev)
            if fused is not None:  # the whole pass from C; the Python loop below has nothing left to do
                fused.fit(feats, targets, order, int(batch_size), imitation_weight)
            for k in range(0, 0 if fused is not None else m, int(batch_size)):
                idx = order[k:k + int(batch_size)]
                if hip is not None:
                    pack()
                    hip.imitation_gradient(feats, targets, idx, imitation_weight, grad=flat_grad)
                    for p, g in zip(params, grad_views):
                        p.grad = g
                else:
                    loss = mse(feats.index_select(0, idx), targets.index_select(0, idx))
                    opt.zero_grad()
                    loss.backward()
                if grad_clip > 0:
                    torch.nn.utils.clip_grad_norm_(net.parameters(), grad_clip)
                opt.step()
            if hip is not None:
                hist["after"].append(hip_loss(feats, targets))
            else:
                with torch.no_grad():
                    hist["after"].append(mse(feats, targets).to(torch.float64))
        if fused is not None:
            net.load_state_dict(fused.network_state_dict())
    finally:
        net.to(home)
    policy._batched = None  # compute_action packs the new weights
    stack = lambda k: torch.stack([v.detach().cpu() for v in hist[k]])  # noqa: E731
    return ImitationResult(mean_reward=stack("reward"), mean_on_target_ratio=stack("ratio"),
                           mean_tracking_error=stack("err"), imitation_loss=stack("imit"),
                           dataset_loss_before=stack("before"), dataset_loss_after=stack("after"),
                           dataset_size=stack("size"),
                           state_dict={k: v.detach().cpu().clone() for k, v in net.state_dict().items()},
                           policy=policy, datasets=datasets)


# ------------------------------------------------------------------ policy search

@dataclass
class SearchResult:
    """search_policy's history (host tensors, one entry per generation) and its best policy."""

    centre_fitness: torch.Tensor      # [G] fitness of the unperturbed centre (member 0)
    best_fitness: torch.Tensor        # [G] fitness of the generation's best member (the incumbent included)
    mean_fitness: torch.Tensor        # [G] mean fitness of the perturbed members
    incumbent_fitness: torch.Tensor   # [G] the best member so far, re-run on this generation's seeds
    best_index: torch.Tensor          # [G] int64 member index of the generation's best
    generation_best: torch.Tensor     # [G, P] float32 flat vector of the generation's best member
    best_theta: torch.Tensor          # [P] float32: the last generation's best (the best so far)
    centre: torch.Tensor              # [P] float32: the centre after the last update
    best_policy: object               # DeepTrackingPolicy holding best_theta (save_checkpoint: reference format)
    generations: int = 0
    population: int = 0
    episodes_per_member: int = 0


def generation_seeds(env_seed: int, generation: int, episodes: int) -> np.ndarray:
    """The reference trainer's reset seeds (train.py:662): env_seed + generation * 1000 + episode."""
    return env_seed + generation * 1000 + np.arange(episodes)


def centred_ranks(fitness: torch.Tensor) -> torch.Tensor:
    """Ranks of a [K] fitness vector scaled to [-0.5, 0.5] (best: +0.5; NaN
    ranks lowest; ties in index order: the sort is stable)."""
    k = fitness.numel()
    order = torch.argsort(torch.nan_to_num(fitness, nan=float("-inf")), stable=True)
    ranks = torch.empty(k, dtype=torch.float32, device=fitness.device)
    ranks[order] = torch.arange(k, dtype=torch.float32, device=fitness.device)
    return ranks / max(k - 1, 1) - 0.5


def search_policy(template=None, env_config=None, *, population: int = 16, sigma: float = 0.05,
                  learning_rate: float = 0.05, generations: int = 10, episodes_per_member: int = 8,
                  max_steps: int | None = None, env_seed: int = 42, seed: int = 0, fitness="tracking_error",
                  criteria=None, motion=None, device=None) -> SearchResult:
    """Evolution strategies over a deep policy's weights on the population rollout.

    template  a DeepTrackingPolicy or its config dict: the shape, and the
              starting centre (its weights)
    Per generation g: `population` antithetic Gaussian perturbations (sigma;
    noise from a torch.Generator on the device seeded with `seed`) of the
    centre, the unperturbed centre as member 0 and the best member so far as
    the last member: population + 2 members in one fused launch on the reset
    seeds env_seed + g * 1000 + j, shared by all members.  The centre moves by
    learning_rate / (population * sigma) * sum(centred rank * perturbation).
    The best member so far is the generation's best, the re-run incumbent
    included, so the comparison is on the same episodes.  Nothing here leaves
    the device until the history is returned."""
    from .controllers.deep import DeepTrackingPolicy, PolicyPopulation
    from .policy import run_policy_population

    if population < 2 or population % 2:
        raise ValueError(f"population must be a positive even number (antithetic pairs), got {population}")
    if not sigma > 0.0:
        raise ValueError(f"sigma must be positive, got {sigma}")
    if episodes_per_member < 1:
        raise ValueError(f"episodes_per_member must be >= 1, got {episodes_per_member}")
    if generations < 1:
        raise ValueError(f"generations must be >= 1, got {generations}")
    dev = _abi.require_gpu(device)
    if not isinstance(template, DeepTrackingPolicy):
        template = DeepTrackingPolicy(dict(template or {}), device="cpu")
    with torch.no_grad():
        centre = torch.nn.utils.parameters_to_vector(template.network.parameters()).detach().to(dev, torch.float32)
    gen = torch.Generator(device=dev).manual_seed(int(seed))
    half, E = population // 2, int(episodes_per_member)
    best = centre.clone()
    hist = {k: [] for k in ("centre", "best", "mean", "incumbent", "index", "theta")}
    for g in range(generations):
        eps = torch.randn(half, centre.numel(), generator=gen, device=dev, dtype=torch.float32)
        eps = torch.cat([eps, -eps])
        theta = torch.cat([centre[None], centre[None] + sigma * eps, best[None]])
        res = run_policy_population(PolicyPopulation.from_flat(template, theta), env_config, episodes_per_member=E,
                                    seeds=generation_seeds(env_seed, g, E), motion=motion, criteria=criteria,
                                    max_steps=max_steps)
        fit = res.fitness(fitness).to(torch.float64)
        order = torch.nan_to_num(fit, nan=float("-inf"))
        # the incumbent wins ties (it is searched first), then the lowest index
        idx = torch.argmax(torch.cat([order[-1:], order[:-1]]))
        idx = torch.where(idx == 0, torch.full_like(idx, theta.shape[0] - 1), idx - 1)
        best = theta.index_select(0, idx.reshape(1))[0]
        hist["centre"].append(fit[0])
        hist["best"].append(fit.index_select(0, idx.reshape(1))[0])
        hist["mean"].append(fit[1:-1].mean())
        hist["incumbent"].append(fit[-1])
        hist["index"].append(idx)
        hist["theta"].append(best)
        w = centred_ranks(fit[1:-1])
        centre = centre + (learning_rate / (population * sigma)) * (w[:, None] * eps).sum(dim=0)
    best_host = best.cpu()
    cfg = dict(template.config or {})
    cfg.pop("checkpoint_path", None)
    net = template.network
    cfg.update(hidden_sizes=list(net.hidden_sizes), activation=net.activation_name,
               output_bounds=dict(net.output_bounds))
    policy = DeepTrackingPolicy(cfg, device=str(template.device))
    with torch.no_grad():
        torch.nn.utils.vector_to_parameters(best_host.clone(), policy.network.parameters())
    stack = lambda k: torch.stack(hist[k]).cpu()  # noqa: E731
    return SearchResult(centre_fitness=stack("centre"), best_fitness=stack("best"), mean_fitness=stack("mean"),
                        incumbent_fitness=stack("incumbent"), best_index=stack("index"),
                        generation_best=stack("theta"), best_theta=best_host, centre=centre.cpu(),
                        best_policy=policy, generations=generations, population=population, episodes_per_member=E)
