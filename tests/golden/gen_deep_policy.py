"""Generate tests/golden/deep_policy.npz from the reference's DeepTrackingPolicy.

Test infrastructure only (build container, reference mounted read-only; the
same no-op `python-dotenv` stand-in as gen_golden.py).  Every value comes from
the reference's own DeepTrackingPolicy, QuadcopterEnv and Evaluator on the CPU.

Networks (torch.manual_seed, Xavier weights as the reference initialises them;
the random ones get small random biases so that the bias path is exercised):
  n0 [64, 64] relu        n1 [32, 32] tanh      n2 [64, 64] elu
  n3 [32, 64, 16] leaky_relu                    n4 [7] relu
  n5 [128, 128] tanh      n6 [64, 64] relu with non-default output_bounds
  lqr: the reference's Riccati LQR (dt 0.01) embedded in a [64, 64] relu
       network: first-layer rows +-K, identity on those 8 units, output
       weights +-1 / ((hi - lo) s0 (1 - s0)), output bias logit(s0), s0 the
       hover point; around hover it commands what the LQR does.

Per network: the state dict, the reference's f32 actions on 512 shared
observations (zeros, +-large values that saturate the sigmoid, boundary-sized
values, random ones), and the actions of the same network in float64
(copy.deepcopy(net).double()) on the same float32 features.

Closed loop (networks lqr, n0, n1, n3; stationary and circular targets; 8
seeds x 300 steps): the reference's states at steps 50 / 100 / 200 / 300 with
the f32 policy, and per component and horizon the largest |f32 run - float64
run| over all seeds and all steps up to that horizon (the tolerance rule's
input; the float64 run steps its own env with the float64 network).  For the
lqr network also the reference Evaluator's per-episode metrics and summary.
The generator asserts that no step of a stored run has a tracking error within
1e-4 of the 0.5 m radius, and that no run ends before step 300 (it moves on to
other seeds otherwise), so on-target counts are exact on both sides.

Usage:  python tests/golden/gen_deep_policy.py [--out tests/golden]
"""

from __future__ import annotations

import argparse
import copy
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import import_reference  # noqa: E402

NETS = [
    {"name": "n0", "hidden_sizes": [64, 64], "activation": "relu", "seed": 100},
    {"name": "n1", "hidden_sizes": [32, 32], "activation": "tanh", "seed": 101},
    {"name": "n2", "hidden_sizes": [64, 64], "activation": "elu", "seed": 102},
    {"name": "n3", "hidden_sizes": [32, 64, 16], "activation": "leaky_relu", "seed": 103},
    {"name": "n4", "hidden_sizes": [7], "activation": "relu", "seed": 104},
    {"name": "n5", "hidden_sizes": [128, 128], "activation": "tanh", "seed": 105},
    {"name": "n6", "hidden_sizes": [64, 64], "activation": "relu", "seed": 106,
     "output_bounds": {"thrust": [2.0, 15.0], "roll_rate": [-1.5, 2.5], "pitch_rate": [-2.0, 2.0],
                       "yaw_rate": [-0.5, 0.25]}},
    {"name": "lqr", "hidden_sizes": [64, 64], "activation": "relu", "seed": 107, "embed_lqr": True},
]
CLOSED = ["lqr", "n0", "n1", "n3"]
MOTIONS = ["stationary", "circular"]
EPISODES, STEPS, CHECKPOINTS = 8, 300, [50, 100, 200, 300]
BOUNDS = {"thrust": (0.0, 20.0), "roll_rate": (-3.0, 3.0), "pitch_rate": (-3.0, 3.0), "yaw_rate": (-3.0, 3.0)}
KEYS = ["thrust", "roll_rate", "pitch_rate", "yaw_rate"]
FIELDS = ["episode_duration", "on_target_ratio", "mean_tracking_error", "max_tracking_error",
          "rms_tracking_error", "total_control_effort", "mean_control_effort", "overshoot_count",
          "max_overshoot", "success"]
SUMMARY = ["total_episodes", "successful_episodes", "success_rate", "mean_on_target_ratio", "std_on_target_ratio",
           "mean_tracking_error", "std_tracking_error", "mean_control_effort", "best_episode_idx",
           "worst_episode_idx", "meets_criteria"]


def make_policy(spec):
    import torch
    from quadcopter_tracking.controllers.deep_tracking_policy import DeepTrackingPolicy
    from quadcopter_tracking.controllers.riccati_lqr import RiccatiLQRController

    torch.manual_seed(spec["seed"])
    cfg = {"hidden_sizes": list(spec["hidden_sizes"]), "activation": spec["activation"]}
    if "output_bounds" in spec:
        cfg["output_bounds"] = {k: tuple(v) for k, v in spec["output_bounds"].items()}
    pol = DeepTrackingPolicy(config=cfg, device="cpu")
    net = pol.network
    with torch.no_grad():
        if spec.get("embed_lqr"):
            ctl = RiccatiLQRController(config={"dt": 0.01})
            K = torch.tensor(np.asarray(ctl.get_gain_matrix(), dtype=np.float64))  # [4, 6] on (pos, vel) error
            l0, l1, lo = net.feature_extractor[0], net.feature_extractor[2], net.output_layer
            for lin in (l0, l1, lo):
                lin.weight.zero_()
                lin.bias.zero_()
            l0.weight[0:4, 0:6] = K.float()
            l0.weight[4:8, 0:6] = -K.float()
            for i in range(8):
                l1.weight[i, i] = 1.0
            hover = [ctl.hover_thrust, 0.0, 0.0, 0.0]
            for i, k in enumerate(KEYS):
                a, b = BOUNDS[k]
                s0 = (hover[i] - a) / (b - a)
                c = 1.0 / ((b - a) * s0 * (1.0 - s0))
                lo.weight[i, i] = c
                lo.weight[i, i + 4] = -c
                lo.bias[i] = float(np.log(s0 / (1.0 - s0)))
        else:
            g = torch.Generator().manual_seed(spec["seed"] + 1000)
            for m in net.modules():
                if isinstance(m, torch.nn.Linear):
                    m.bias.copy_((torch.rand(m.bias.shape, generator=g) - 0.5) * 0.2)
    return pol


def observations(rng):
    """512 observations as [512, 6, 3]: quad position, velocity, attitude, angular velocity, target position, velocity."""
    o = rng.normal(size=(512, 6, 3)) * np.array([2.0, 1.5, 0.4, 1.0, 2.0, 1.0])[None, :, None]
    o[0] = 0.0
    o[1] = 1e4          # large: saturates the sigmoid one way or the other
    o[2] = -1e4
    o[3, 0], o[3, 4] = 1e6, -1e6
    o[4, 0], o[4, 4] = -1e6, 1e6
    o[5] = 1e-30        # tiny
    o[6] = [[100.0] * 3, [20.0] * 3, [np.pi / 3] * 3, [10.0] * 3, [-100.0] * 3, [-20.0] * 3]  # boundary-sized
    o[7] = -o[6]
    o[8, 2] = [np.pi, -np.pi, np.pi]
    o[9:40] *= 25.0     # wide range
    o[40:60] *= 1e-3    # near zero
    return o


def obs_dict(row):
    return {"quadcopter": {"position": row[0], "velocity": row[1], "attitude": row[2], "angular_velocity": row[3]},
            "target": {"position": row[4], "velocity": row[5]}}


class Double:
    """The same policy with its network in float64 (on the float32 features)."""

    def __init__(self, pol):
        self.pol = pol
        self.net = copy.deepcopy(pol.network).double()

    def compute_action(self, observation):
        import torch

        f = self.pol._extract_features(observation)
        with torch.no_grad():
            a = self.net(torch.tensor(f, dtype=torch.float32).double().unsqueeze(0)).numpy().squeeze()
        return {k: float(a[i]) for i, k in enumerate(KEYS)}


def closed_loop(ctl, motion, seed):
    """300 steps of the reference env under ctl: states [300, 12] after each step, actions [300, 4], pre- and
    post-step tracking errors, first done step (or -1)."""
    from quadcopter_tracking.env import QuadcopterEnv

    env = QuadcopterEnv({"target": {"motion_type": motion}, "logging": {"enabled": False}})
    obs = env.reset(seed=seed)
    X, U, E, first_done = [], [], [], -1
    for k in range(STEPS):
        q, t = obs["quadcopter"], obs["target"]
        E.append(float(np.linalg.norm(np.asarray(t["position"]) - np.asarray(q["position"]))))
        a = ctl.compute_action(obs)
        obs, _, done, info = env.step(a)
        E.append(float(info["tracking_error"]))
        X.append(env.get_state_vector().copy())
        U.append([a[k2] for k2 in KEYS])
        if done and first_done < 0:
            first_done = k
    return np.array(X), np.array(U), np.array(E), first_done


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.dirname(os.path.abspath(__file__)))
    args = ap.parse_args()
    import_reference()
    import torch
    from quadcopter_tracking.env.config import EnvConfig
    from quadcopter_tracking.eval import Evaluator
    from quadcopter_tracking.utils.metrics import compute_episode_metrics

    torch.set_num_threads(1)
    out = {}
    obs = observations(np.random.default_rng(2024))
    out["obs"] = obs
    pols = {}
    for spec in NETS:
        pol = make_policy(spec)
        pols[spec["name"]] = pol
        for k, v in pol.network.state_dict().items():
            out[f"{spec['name']}/sd/{k}"] = v.numpy().copy()
        dbl = Double(pol)
        a32 = np.array([[pol.compute_action(obs_dict(r))[k] for k in KEYS] for r in obs])
        a64 = np.array([[dbl.compute_action(obs_dict(r))[k] for k in KEYS] for r in obs])
        out[f"{spec['name']}/act32"] = a32
        out[f"{spec['name']}/act64"] = a64
        out[f"{spec['name']}/features"] = np.array([pol._extract_features(obs_dict(r)) for r in obs])
        print(spec["name"], "action gap", np.abs(a32 - a64).max(axis=0))
    runs = {}
    for name in CLOSED:
        pol, dbl = pols[name], Double(pols[name])
        for motion in MOTIONS:
            base = 42
            while True:  # seeds whose runs stay off the 0.5 m knife edge and run all 300 steps
                seeds = base + np.arange(EPISODES)
                r32 = [closed_loop(pol, motion, int(s)) for s in seeds]
                ok = all(r[3] < 0 and np.abs(r[2] - 0.5).min() >= 1e-4 for r in r32)
                if ok:
                    break
                base += EPISODES
            r64 = [closed_loop(dbl, motion, int(s)) for s in seeds]
            X32 = np.array([r[0] for r in r32])  # [8, 300, 12]
            X64 = np.array([r[0] for r in r64])
            U32, U64 = np.array([r[1] for r in r32]), np.array([r[1] for r in r64])
            key = f"{name}/{motion}"
            cp = np.array(CHECKPOINTS) - 1
            out[f"{key}/seeds"] = seeds
            out[f"{key}/states"] = X32[:, cp]  # [8, 4, 12]
            out[f"{key}/actions"] = U32[:, cp]  # the command of steps 50 / 100 / 200 / 300
            gx, gu = np.abs(X32 - X64), np.abs(U32 - U64)
            out[f"{key}/state_gap"] = np.array([gx[:, :c].max(axis=(0, 1)) for c in CHECKPOINTS])  # [4, 12]
            out[f"{key}/action_gap"] = np.array([gu[:, :c].max(axis=(0, 1)) for c in CHECKPOINTS])  # [4, 4]
            runs[key] = int(base)
            print(key, "base seed", base, "state gap at 300", gx.max(), "final err", [round(r[2][-1], 3) for r in r32][:4])
            if name == "lqr":
                with tempfile.TemporaryDirectory() as tmp:
                    cfg = EnvConfig.from_dict({"target": {"motion_type": motion}, "logging": {"enabled": False}})
                    mets = {}
                    for tag, ctl in (("metrics", pol), ("metrics64", dbl)):
                        ev = Evaluator(ctl, env_config=cfg, output_dir=tmp)
                        rows = []
                        for s in seeds:
                            data, info = ev.run_episode(seed=int(s), max_steps=STEPS)
                            m = compute_episode_metrics(data, ev.criteria, info)
                            rows.append([float(getattr(m, f)) for f in FIELDS])
                        mets[tag] = np.array(rows)
                    out[f"{key}/metrics"] = mets["metrics"]
                    out[f"{key}/metrics_gap"] = np.abs(mets["metrics"] - mets["metrics64"]).max(axis=0)
                    ev = Evaluator(pol, env_config=cfg, output_dir=tmp)
                    summary = ev.evaluate(num_episodes=EPISODES, base_seed=int(base), max_steps_per_episode=STEPS,
                                          verbose=False)
                    out[f"{key}/summary"] = np.array([float(getattr(summary, k)) for k in SUMMARY])
                print(key, "on-target ratio", out[f"{key}/metrics"][:, 1])
    out["meta_json"] = np.array(json.dumps({"nets": NETS, "closed": CLOSED, "motions": MOTIONS, "episodes": EPISODES,
                                            "steps": STEPS, "checkpoints": CHECKPOINTS, "fields": FIELDS,
                                            "summary": SUMMARY, "base_seeds": runs}))
    path = os.path.join(args.out, "deep_policy.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
