#!/usr/bin/env python
"""Deep tracking policy: the fused rollout against the per-step baseline.

  python scripts/bench_policy.py [--episodes 65536] [--steps 3000] [--passes 10] [--hidden 64,64] [--out FILE]
      qt_policy_rollout, a relu network of the --hidden sizes (torch.manual_seed(0)
      Xavier weights): best pass of --passes by HIP events around the rollout launch
      (the reset is outside the events).  Reports ms per pass, ns per executed
      env-step and the fraction of the 157.3 TF f32 peak, counting 2 flops per
      multiply-add of the unpadded layers ([64, 64]: 2 x 5,504 per env-step).

  python scripts/bench_policy.py --baseline [--episodes 65536] [--steps 300]
      The only way to run such a policy without the policy kernels:
      torch.nn.Sequential on the device, the 18 features built with torch
      ops, BatchedQuadcopterEnv.step, one step at a time; wall time between
      two synchronisations, best of --passes (default 3).  Imports nothing
      the policy feature added, so it also runs on a checkout without it.

  python scripts/bench_policy.py --members 1024 [--per-member 64] [--sample 32] [--steps 300] [--passes 10]
      Policy populations: (a) one qt_policy_population_rollout launch of
      members x per-member episodes, (c) one qt_policy_rollout launch of as
      many episodes with shared weights, and with --sample K
      (b) the per-member way: K members' single-policy launches, scaled by
      members / K.  HIP events, best of --passes.

  python scripts/bench_policy.py --supervised [--episodes 65536] [--steps 300] [--samples 32] [--passes 10]
      The supervised rollout (Riccati-LQR teacher): (a) one
      qt_policy_supervised_rollout launch, (c) qt_policy_rollout on the same
      inputs (the floor), both by HIP events, best of --passes, and (b) the
      per-step way to the same labels (policy action + teacher action +
      env.step, three launches per step), by the wall clock, best of 3.

  python scripts/bench_policy.py --grad [--sizes 256,65536,2097152] [--passes 10]
      The imitation loss and its gradient for minibatches drawn through an
      index from a seeded synthetic data set of 2,097,152 pairs, one line per
      size: (a) BatchedDeepPolicy.imitation_gradient (qt_policy_imitation_grad)
      by HIP events, best of --passes; (b) what train_imitation's torch backend
      does for the same minibatch (index_select, forward, mse_loss, zero_grad,
      backward): at 256 by the wall clock between two synchronisations over
      100 steps (host-bound, as --baseline), at the larger sizes by HIP events;
      (c) the floor from the flop count, 3 x 2 x the multiply-adds per sample
      at 157.3 TF.

  python scripts/bench_policy.py --fit [--pairs 65536] [--sizes 256,4096] [--passes 10]
      One pass of Adam minibatch steps (clip 1.0) over a seeded synthetic data
      set, one line per minibatch size, wall time per minibatch between two
      synchronisations around the whole pass, best of --passes, the three
      ways alternating inside every pass: (a) PolicyOptimizer.fit
      (qt_policy_imitation_fit: four launches per minibatch enqueued from C),
      (b) the minibatch loop of train_imitation(backend="hip") (pack,
      imitation_gradient, .grad views, clip_grad_norm_, torch's Adam), (c) the
      torch backend's loop (index_select, autograd, clip_grad_norm_, Adam).

Each run prints one JSON line (--grad, --fit: one per size) and appends it to --out when given.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lqr-quadcopter-test_amd"))


def flops_per_step(hidden):
    dims = [18] + list(hidden) + [4]
    return 2 * sum(a * b for a, b in zip(dims[:-1], dims[1:]))  # [64, 64]: 11,008


PEAK_F32 = 157.3e12
ENV_CFG = {"target": {"motion_type": "circular"}}


def network(device, hidden=(64, 64)):
    torch.manual_seed(0)
    layers, prev = [], 18
    for h in hidden:
        layers += [torch.nn.Linear(prev, h), torch.nn.ReLU()]
        prev = h
    layers.append(torch.nn.Linear(prev, 4))
    for m in layers:
        if isinstance(m, torch.nn.Linear):
            torch.nn.init.xavier_uniform_(m.weight)
            torch.nn.init.zeros_(m.bias)
    return torch.nn.Sequential(*layers).to(device).eval()


def fused(args):
    import quadtrack
    from quadtrack import core
    from quadtrack.env.config import as_env_config
    from quadtrack.policy import policy_batch

    dev = torch.device("cuda:0")
    net = network("cpu", args.hidden)
    sd = {}
    for i in range(len(args.hidden)):
        sd[f"feature_extractor.{2 * i}.weight"], sd[f"feature_extractor.{2 * i}.bias"] = net[2 * i].weight, net[2 * i].bias
    sd["output_layer.weight"], sd["output_layer.bias"] = net[-1].weight, net[-1].bias
    pol = quadtrack.BatchedDeepPolicy.from_state_dict(sd, args.hidden, "relu", device=dev)
    cfg = as_env_config(ENV_CFG)
    env, crit, n = cfg.to_params(), core.criteria(), args.episodes
    batch = policy_batch(cfg, n, dev, seeds=np.arange(n))
    st = core.RolloutState.empty(n, dev)
    times = []
    for _ in range(args.passes + 1):  # the first pass warms up
        core.reset(env, batch, st)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        pol.rollout(env, crit, batch, st, args.steps)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    times = times[1:]
    env_steps = float(st.acc[quadtrack._abi.ACC_STEPS].sum())
    best = min(times)
    flops = flops_per_step(args.hidden)
    return {"what": "policy_rollout_fused", "network": f"{list(args.hidden)} relu", "episodes": n, "steps": args.steps,
            "passes": args.passes, "ms_per_pass_best": best, "ms_per_pass_all": [round(t, 3) for t in times],
            "env_steps_per_pass": env_steps, "ns_per_env_step": best * 1e6 / env_steps,
            "flops_per_env_step": flops, "fraction_of_f32_peak": env_steps * flops / (best * 1e-3) / PEAK_F32,
            "timer": "HIP events around the rollout launch"}


def _event_ms(launch, before, passes):
    """Best of `passes` HIP-event times of launch(); before() runs outside the events; the first pass warms up."""
    times = []
    for _ in range(passes + 1):
        before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return min(times[1:]), [round(t, 3) for t in times[1:]]


def population(args):
    """(a) one population launch of --members x --per-member episodes; (c) one single-policy launch of the
    same number of episodes (shared weights, read from global memory); with --sample K > 0 also (b) the same work as
    per-member launches: K members' --per-member-episode single-policy launches back to back inside one
    pair of events, scaled by members / K (stated in the line)."""
    import quadtrack
    from quadtrack import core
    from quadtrack.env.config import as_env_config
    from quadtrack.policy import policy_batch, run_policy_loop

    dev = torch.device("cuda:0")
    net = network("cpu", args.hidden)
    template = quadtrack.DeepTrackingPolicy({"hidden_sizes": args.hidden, "activation": "relu"}, device="cpu")
    centre = torch.nn.utils.parameters_to_vector(net.parameters()).detach()
    M, E = args.members, args.per_member
    g = torch.Generator().manual_seed(1)
    theta = centre[None] + 0.05 * torch.randn(M, centre.numel(), generator=g)
    theta[0] = centre
    pop = quadtrack.PolicyPopulation.from_flat(template, theta, device=dev)
    cfg = as_env_config(ENV_CFG)
    env, crit, n = cfg.to_params(), core.criteria(), M * E
    seeds = np.tile(np.arange(E), M)  # common random numbers
    batch = policy_batch(cfg, n, dev, seeds=seeds)
    st = core.RolloutState.empty(n, dev)
    reset = lambda: core.reset(env, batch, st)  # noqa: E731
    a_best, a_all = _event_ms(lambda: pop.rollout(env, crit, batch, st, args.steps, E), reset, args.passes)
    a_steps = float(st.acc[quadtrack._abi.ACC_STEPS].sum())
    shared = pop.member(0)
    c_best, c_all = _event_ms(lambda: shared.rollout(env, crit, batch, st, args.steps), reset, args.passes)
    c_steps = float(st.acc[quadtrack._abi.ACC_STEPS].sum())
    waves = M * ((E + 63) // 64)
    line = {"what": "policy_population", "network": f"{list(args.hidden)} relu", "members": M, "episodes_per_member": E,
            "episodes": n, "steps": args.steps, "passes": args.passes, "waves": waves,
            "lane_utilisation": n / (64.0 * waves), "block_bytes_per_member": 4 * pop.block_floats,
            # weights run from LDS when four waves' blocks fit 160 KiB, unless QT_POPULATION_STAGE=0
            "staged_in_lds": 4 * 4 * ((pop.block_floats + 63) // 64 * 64) <= 160 * 1024
            and not os.environ.get("QT_POPULATION_STAGE", "1").startswith("0"),
            "a_population_ms_best": a_best, "a_population_ms_all": a_all, "a_env_steps": a_steps,
            "a_ns_per_env_step": a_best * 1e6 / a_steps,
            "c_shared_weights_ms_best": c_best, "c_shared_weights_ms_all": c_all, "c_env_steps": c_steps,
            "a_over_c": a_best / c_best, "timer": "HIP events around the rollout launch (the reset is outside)"}
    K = min(args.sample, M)
    if K > 0:
        members = [pop.member(m) for m in range(K)]
        sub = policy_batch(cfg, E, dev, seeds=np.arange(E))
        states = [core.RolloutState.empty(E, dev) for _ in range(K)]

        def reset_all():
            for s in states:
                core.reset(env, sub, s)

        def launch_all():
            for p, s in zip(members, states):
                p.rollout(env, crit, sub, s, args.steps)

        b_best, b_all = _event_ms(launch_all, reset_all, args.passes)
        # the whole of run_policy_loop per member (batch, reset, launch, metrics), wall clock: what a caller pays
        walls = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for p in members:
                run_policy_loop(p, cfg, n=E, seeds=np.arange(E), max_steps=args.steps)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        line.update({"b_sample_members": K, "b_sample_launches_ms_best": b_best, "b_sample_launches_ms_all": b_all,
                     "b_per_member_launches_ms_scaled": b_best * M / K, "a_over_b": a_best / (b_best * M / K),
                     "b_run_policy_loop_wall_ms_scaled": min(walls) * M / K,
                     "a_over_b_run_policy_loop_wall": a_best / (min(walls) * M / K),
                     "b_note": f"{K} of {M} members timed ({E}-episode qt_policy_rollout launches back to back in one "
                               f"event pair; run_policy_loop calls by wall clock, best of 3), scaled by {M}/{K}"})
    return line


def supervised(args):
    """(a) one qt_policy_supervised_rollout launch (Riccati-LQR teacher, --samples slots per episode);
    (c) qt_policy_rollout on the same inputs, the floor; (b) the way to the same labels without the
    supervised kernel: BatchedDeepPolicy.compute_action + BatchedRiccatiLQR.compute_action + env.step, one
    step at a time, by the wall clock between two synchronisations (best of 3, as --baseline)."""
    import quadtrack
    from quadtrack import core
    from quadtrack.controllers import BatchedRiccatiLQR
    from quadtrack.env.config import as_env_config
    from quadtrack.policy import sample_steps
    from quadtrack.rollout import build_batch

    dev = torch.device("cuda:0")
    net = network("cpu", args.hidden)
    sd = {}
    for i in range(len(args.hidden)):
        sd[f"feature_extractor.{2 * i}.weight"], sd[f"feature_extractor.{2 * i}.bias"] = net[2 * i].weight, net[2 * i].bias
    sd["output_layer.weight"], sd["output_layer.bias"] = net[-1].weight, net[-1].bias
    pol = quadtrack.BatchedDeepPolicy.from_state_dict(sd, args.hidden, "relu", device=dev)
    sup = BatchedRiccatiLQR({"dt": 0.01}, device=dev)
    cfg = as_env_config(ENV_CFG)
    env, crit, n, S = cfg.to_params(), core.criteria(), args.episodes, args.samples
    batch = build_batch(sup, cfg, n, seeds=np.arange(n), group_motion=False)
    st = core.RolloutState.empty(n, dev)
    steps = torch.as_tensor(sample_steps(n, S, args.steps, 0), device=dev)
    sample = torch.empty(S, quadtrack._abi.SUP_ROWS, n, dtype=torch.float32, device=dev)
    loss = torch.zeros(n, dtype=torch.float64, device=dev)

    def reset():
        core.reset(env, batch, st)
        loss.zero_()
        sample.fill_(float("nan"))

    a_best, a_all = _event_ms(lambda: pol.rollout_supervised(env, sup.ctrl, crit, batch, st, args.steps, loss, steps,
                                                             sample), reset, args.passes)
    a_steps = float(st.acc[quadtrack._abi.ACC_STEPS].sum())
    mse = float((loss / (4.0 * st.acc[quadtrack._abi.ACC_STEPS])).mean())
    filled = float((~torch.isnan(sample[:, 0])).double().mean())
    c_best, c_all = _event_ms(lambda: pol.rollout(env, crit, batch, st, args.steps), reset, args.passes)
    c_steps = float(st.acc[quadtrack._abi.ACC_STEPS].sum())
    benv = quadtrack.BatchedQuadcopterEnv(n, ENV_CFG, device=dev)
    walls = []
    for _ in range(4):  # the first pass warms up
        obs = benv.reset(np.arange(n))
        sup.reset(n)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            act = pol.compute_action(obs)
            sup.compute_action(obs)  # the label of this step (a caller would keep it)
            obs, _, _, _ = benv.step(act)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    b_best = min(walls[1:])
    return {"what": "policy_supervised", "network": f"{list(args.hidden)} relu", "teacher": "riccati_lqr dt 0.01",
            "episodes": n, "steps": args.steps, "samples_per_episode": S, "passes": args.passes,
            "a_supervised_ms_best": a_best, "a_supervised_ms_all": a_all, "a_env_steps": a_steps,
            "a_ns_per_env_step": a_best * 1e6 / a_steps, "mean_imitation_loss": mse, "sample_slots_filled": filled,
            "c_policy_rollout_ms_best": c_best, "c_policy_rollout_ms_all": c_all, "c_env_steps": c_steps,
            "a_over_c": a_best / c_best,
            "b_per_step_api_wall_ms_best": b_best, "b_per_step_api_wall_ms_all": [round(t, 3) for t in walls[1:]],
            "a_over_b": a_best / b_best,
            "b_path": "BatchedDeepPolicy.compute_action + BatchedRiccatiLQR.compute_action + BatchedQuadcopterEnv.step, "
                      "three launches per step, wall clock between synchronisations, best of 3 (labels only: no "
                      "loss, no samples kept)",
            "timer": "HIP events around the rollout launch (reset, loss and sample pre-fill outside) for (a) and (c)"}


def baseline(args):
    import quadtrack

    dev = torch.device("cuda:0")
    net = network(dev, args.hidden)
    n = args.episodes
    env = quadtrack.BatchedQuadcopterEnv(n, ENV_CFG, device=dev)
    lo = torch.tensor([0.0, -3.0, -3.0, -3.0], dtype=torch.float32, device=dev)
    scale = torch.tensor([20.0, 6.0, 6.0, 6.0], dtype=torch.float32, device=dev)
    times = []
    with torch.no_grad():
        for _ in range(args.passes + 1):
            obs = env.reset(np.arange(n))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                q, tg = obs["quadcopter"], obs["target"]
                f = torch.cat([tg["position"] - q["position"], tg["velocity"] - q["velocity"], q["attitude"],
                               q["angular_velocity"], tg["position"], tg["velocity"]], dim=1).float()
                a = (torch.sigmoid(net(f)) * scale + lo).double()
                obs, _, _, _ = env.step(a)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
    times = times[1:]
    best = min(times)
    env_steps = float(n * args.steps)
    return {"what": "policy_rollout_baseline", "network": f"{list(args.hidden)} relu", "episodes": n, "steps": args.steps,
            "passes": args.passes, "ms_per_pass_best": best, "ms_per_pass_all": [round(t, 3) for t in times],
            "env_steps_per_pass": env_steps, "ns_per_env_step": best * 1e6 / env_steps,
            "timer": "wall clock between synchronisations",
            "path": "torch.nn.Sequential + torch feature build + BatchedQuadcopterEnv.step, one step at a time"}


def grad(args):
    """(a) the HIP loss + gradient entry, (b) the torch backend's minibatch step without the optimiser,
    (c) the flop floor; one line per minibatch size."""
    import quadtrack

    dev = torch.device("cuda:0")
    net = network(dev, args.hidden).train()
    sd = {}
    for i in range(len(args.hidden)):
        sd[f"feature_extractor.{2 * i}.weight"], sd[f"feature_extractor.{2 * i}.bias"] = net[2 * i].weight, net[2 * i].bias
    sd["output_layer.weight"], sd["output_layer.bias"] = net[-1].weight, net[-1].bias
    pol = quadtrack.BatchedDeepPolicy.from_state_dict(sd, args.hidden, "relu", device=dev)
    rows = max(max(args.sizes), 1 << 21)
    gen = torch.Generator(device=dev).manual_seed(0)
    feats = torch.randn(rows, 18, generator=gen, device=dev, dtype=torch.float32) * 2.0
    lo = torch.tensor([0.0, -3.0, -3.0, -3.0], device=dev)
    scale = torch.tensor([20.0, 6.0, 6.0, 6.0], device=dev)
    targets = torch.rand(rows, 4, generator=gen, device=dev, dtype=torch.float32) * scale + lo
    params = list(net.parameters())

    def torch_step(idx):  # train_imitation's torch backend up to the clip
        loss = torch.nn.functional.mse_loss(torch.sigmoid(net(feats.index_select(0, idx))) * scale + lo,
                                            targets.index_select(0, idx))
        for p in params:
            p.grad = None
        loss.backward()
        return loss

    lines = []
    for m in args.sizes:
        idx = torch.randperm(rows, generator=gen, device=dev)[:m].contiguous()
        out = torch.empty(sum(p.numel() for p in params), dtype=torch.float32, device=dev)
        hip_ms, hip_all = _event_ms(lambda: pol.imitation_gradient(feats, targets, idx, 1.0, grad=out), lambda: None,
                                    args.passes)
        loss_hip = float(pol.imitation_gradient(feats, targets, idx, 1.0, grad=out)[0][0])
        loss_torch = float(torch_step(idx))
        flat = torch.cat([p.grad.reshape(-1) for p in params])
        if m <= 4096:  # host-bound: wall clock over 100 steps between two synchronisations, best of 3
            best = float("inf")
            for _ in range(4):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(100):
                    torch_step(idx)
                torch.cuda.synchronize()
                best = min(best, (time.perf_counter() - t0) * 10.0)  # ms per step
            torch_ms, torch_timer = best, "wall clock over 100 steps between two synchronisations, best of 4"
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(100):
                pol.imitation_gradient(feats, targets, idx, 1.0, grad=out)
            torch.cuda.synchronize()
            hip_wall = (time.perf_counter() - t0) * 10.0
        else:
            torch_ms, _ = _event_ms(lambda: torch_step(idx), lambda: None, args.passes)
            torch_timer, hip_wall = "HIP events, best of passes", None
        floor_ms = 3 * flops_per_step(args.hidden) * m / PEAK_F32 * 1e3
        lines.append({"what": "policy_imitation_gradient", "network": f"{list(args.hidden)} relu", "samples": m,
                      "passes": args.passes, "hip_ms_best": hip_ms, "hip_ms_all": hip_all,
                      "hip_ms_wall_per_call": hip_wall, "torch_ms": torch_ms, "torch_timer": torch_timer,
                      "torch_over_hip": torch_ms / (hip_wall if hip_wall is not None else hip_ms),
                      "floor_ms": floor_ms, "hip_over_floor": hip_ms / floor_ms,
                      "loss_hip": loss_hip, "loss_torch": loss_torch,
                      "max_abs_grad_difference": float((flat - out).abs().max()),
                      "max_abs_grad": float(flat.abs().max()),
                      "timer": "HIP events around the three launches of the entry, best of passes"})
    return lines


def fit(args):
    """(a) the fused pass, (b) the hip backend's minibatch loop, (c) the torch backend's; one line per batch size."""
    import quadtrack
    from quadtrack import _abi
    from quadtrack.controllers.deep import PolicyPopulation, flat_size, policy_tiles, unflatten

    dev = torch.device("cuda:0")
    sizes, rows = list(args.hidden), args.pairs
    gen = torch.Generator(device=dev).manual_seed(0)
    feats = torch.randn(rows, 18, generator=gen, device=dev, dtype=torch.float32) * 2.0
    lo = torch.tensor([0.0, -3.0, -3.0, -3.0], device=dev)
    scale = torch.tensor([20.0, 6.0, 6.0, 6.0], device=dev)
    targets = torch.rand(rows, 4, generator=gen, device=dev, dtype=torch.float32) * scale + lo
    order = torch.randperm(rows, generator=gen, device=dev)
    names = [f"feature_extractor.{2 * i}" for i in range(len(sizes))] + ["output_layer"]

    def state_dict(net):
        lin = [m for m in net if isinstance(m, torch.nn.Linear)]
        return {f"{n}.{k}": getattr(m, k).detach() for n, m in zip(names, lin) for k in ("weight", "bias")}

    def adam(net):
        return torch.optim.Adam(net.parameters(), lr=1e-3)

    lines = []
    for batch in args.sizes:
        # (a)
        start = quadtrack.BatchedDeepPolicy.from_state_dict(state_dict(network("cpu", sizes)), sizes, "relu", device=dev)
        fused_opt = quadtrack.PolicyOptimizer(start, "adam", learning_rate=1e-3, grad_clip=1.0)
        # (b): train_imitation(backend="hip")'s minibatch loop
        net_b = network(dev, sizes).train()
        params_b, opt_b = list(net_b.parameters()), adam(net_b)
        gather, _ = PolicyPopulation._device_index(sizes, dev)
        src = torch.zeros(flat_size(sizes) + 1, dtype=torch.float32, device=dev)
        block = torch.empty(_abi.policy_block_floats(len(sizes), policy_tiles(sizes)), dtype=torch.float32, device=dev)
        flat_grad = torch.zeros(flat_size(sizes), dtype=torch.float32, device=dev)
        hip = quadtrack.BatchedDeepPolicy.from_block(block, sizes, "relu")
        views = unflatten(flat_grad, sizes)
        grad_views = [views[f"{n}.{k}"] for n in names for k in ("weight", "bias")]

        def pass_b():
            for k in range(0, rows, batch):
                idx = order[k:k + batch]
                with torch.no_grad():
                    torch.cat([p.reshape(-1) for p in params_b], out=src[:-1])
                    torch.index_select(src, 0, gather, out=block)
                hip.imitation_gradient(feats, targets, idx, 1.0, grad=flat_grad)
                for p, g in zip(params_b, grad_views):
                    p.grad = g
                torch.nn.utils.clip_grad_norm_(params_b, 1.0)
                opt_b.step()

        # (c): the torch backend's loop
        net_c = network(dev, sizes).train()
        params_c, opt_c = list(net_c.parameters()), adam(net_c)

        def pass_c():
            for k in range(0, rows, batch):
                idx = order[k:k + batch]
                loss = torch.nn.functional.mse_loss(torch.sigmoid(net_c(feats.index_select(0, idx))) * scale + lo,
                                                    targets.index_select(0, idx))
                opt_c.zero_grad()
                loss.backward()
                torch.nn.utils.clip_grad_norm_(params_c, 1.0)
                opt_c.step()

        ways = {"fit": lambda: fused_opt.fit(feats, targets, order, batch), "hip_loop": pass_b, "torch_loop": pass_c}
        steps = -(-rows // batch)
        times = {k: [] for k in ways}
        for _ in range(args.passes + 1):  # the first pass warms up
            for k, run in ways.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3 / steps)
        best = {k: min(v[1:]) for k, v in times.items()}
        # the clip + optimiser + pack launch alone: HIP events around 200 back-to-back steps, best of passes
        g = torch.randn(flat_size(sizes), generator=gen, device=dev, dtype=torch.float32) * 1e-2

        def steps_200():
            for _ in range(200):
                fused_opt.step(g)

        step_ms = _event_ms(steps_200, lambda: None, args.passes)[0] / 200.0
        lines.append({"what": "policy_imitation_fit", "network": f"{sizes} relu", "pairs": rows, "batch": batch,
                      "steps_per_pass": steps, "passes": args.passes, "optimizer": "adam lr 1e-3, clip 1.0",
                      "fit_ms_per_minibatch": best["fit"], "hip_loop_ms_per_minibatch": best["hip_loop"],
                      "torch_loop_ms_per_minibatch": best["torch_loop"],
                      "hip_loop_over_fit": best["hip_loop"] / best["fit"],
                      "torch_loop_over_fit": best["torch_loop"] / best["fit"],
                      "optim_step_ms_events_200_back_to_back": step_ms,
                      "all_ms_per_minibatch": {k: [round(t, 5) for t in v[1:]] for k, v in times.items()},
                      "timer": "wall clock between two synchronisations around one pass over the data set, "
                               "divided by its minibatches; best of passes, the three ways alternating"})
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--episodes", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--passes", type=int, default=None)
    ap.add_argument("--hidden", default="64,64", help="hidden layer sizes, comma-separated")
    ap.add_argument("--out", default=None)
    ap.add_argument("--members", type=int, default=0, help="population mode: members of one fused launch")
    ap.add_argument("--per-member", type=int, default=64, help="population mode: episodes per member")
    ap.add_argument("--sample", type=int, default=0,
                    help="population mode: members whose single-policy launches are timed and scaled (0: skip)")
    ap.add_argument("--supervised", action="store_true", help="the supervised rollout against its floor and the per-step way")
    ap.add_argument("--samples", type=int, default=32, help="supervised mode: sample slots per episode")
    ap.add_argument("--grad", action="store_true", help="the imitation gradient against the torch backend's step")
    ap.add_argument("--sizes", default=None,
                    help="--grad: minibatch sizes, comma-separated (default 256,65536,2097152); --fit: default 256,4096")
    ap.add_argument("--fit", action="store_true", help="the fused minibatch pass against the hip and torch backends' loops")
    ap.add_argument("--pairs", type=int, default=65536, help="--fit: pairs of the synthetic data set")
    args = ap.parse_args()
    args.sizes = [int(v) for v in (args.sizes or ("256,4096" if args.fit else "256,65536,2097152")).split(",")]
    args.hidden = [int(v) for v in args.hidden.split(",")]
    if args.steps is None:
        args.steps = 300 if args.baseline or args.members or args.supervised else 3000
    if args.passes is None:
        args.passes = 3 if args.baseline else 10
    line = (fit(args) if args.fit else grad(args) if args.grad else supervised(args) if args.supervised else population(args) if args.members
            else baseline(args) if args.baseline else fused(args))
    lines = line if isinstance(line, list) else [line]
    for ln in lines:
        ln["device"] = torch.cuda.get_device_name(0)
    text = "\n".join(json.dumps(ln) for ln in lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
