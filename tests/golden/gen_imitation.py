"""Generate tests/golden/imitation.npz: the reference's imitation labels.

Test infrastructure only (build container, reference mounted read-only; the
same stand-ins as gen_golden.py and gen_deep_policy.py, whose helpers this
imports).  Every value comes from the reference's own DeepTrackingPolicy,
QuadcopterEnv and supervisor controllers on the CPU, in the order of the
trainer's imitation epoch (Trainer._train_epoch): supervisor.reset() per
episode, then per step supervisor.compute_action(obs) on the observation the
policy is about to act on, then env.step(policy action).  The supervisor never
influences the flight, so one flight serves every supervisor.

Networks: lqr and n1 of gen_deep_policy.py (make_policy: the same weights).
Supervisors: PIDController(default config), LQRController(default),
RiccatiLQRController({"dt": 0.01}) and the same with use_lqi (the default
q_int of zero: the integral runs, its gains are ~1e-19; the generator asserts
a 4 x 9 gain, that is, no fallback to the heuristic controller).
Targets: stationary and circular; 4 seeds from deep_policy.npz's recorded base
seed of the (network, motion) pair; 300 steps, and the generator asserts that
every stored run lasts 300 steps.

Stored, per flight (network/motion): the seeds, and at the stored steps (0-9
and every 10th) the observation the supervisor saw (quad position, velocity,
target position, velocity) and its time.  Per run (network/supervisor/motion):
the supervisor's FP64 commands at the stored steps, its state BEFORE those
calls (LQI integral; PID integral and last time, NaN = None) so that a
stateful command can be replayed from the fixture alone, the whole-episode
F.mse_loss of the policy's f32 commands against the f32 labels
(torch.tensor(..., dtype=torch.float32), as the trainer builds them), and the
tolerance rule's input: per component and stored step, the largest |command on
the f32 flight - command on the flight of the float64 network|
(gen_deep_policy.Double, which flies its own env) over the seeds and every
step up to it, and the largest loss gap between the two flights.

Usage:  python tests/golden/gen_imitation.py [--out tests/golden]
"""

from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_deep_policy import KEYS, NETS, Double, make_policy  # noqa: E402
from gen_golden import import_reference  # noqa: E402

NET_NAMES = ["lqr", "n1"]
SUPERVISORS = [
    {"name": "pid", "type": "pid", "config": {}},
    {"name": "lqr", "type": "lqr", "config": {}},
    {"name": "riccati", "type": "riccati_lqr", "config": {"dt": 0.01}},
    {"name": "lqi", "type": "riccati_lqr", "config": {"dt": 0.01, "use_lqi": True}},
]
MOTIONS = ["stationary", "circular"]
EPISODES, STEPS = 4, 300
STORED = list(range(10)) + list(range(10, STEPS, 10))


def make_supervisor(spec):
    from quadcopter_tracking.controllers import LQRController, PIDController
    from quadcopter_tracking.controllers.riccati_lqr import RiccatiLQRController

    cls = {"pid": PIDController, "lqr": LQRController, "riccati_lqr": RiccatiLQRController}[spec["type"]]
    return cls(config=dict(spec["config"]))


def state_of(spec, sup):
    """The supervisor's carried state as 4 numbers (unused ones 0)."""
    if spec["type"] == "pid":
        return [*np.asarray(sup.integral_error, float), float("nan") if sup._last_time is None else sup._last_time]
    if spec["config"].get("use_lqi"):
        return [*np.asarray(sup.integral_state, float), 0.0]
    return [0.0] * 4


def flight(ctl, sups, motion, seed):
    """One episode flown by ctl with every supervisor labelling it: observations [300, 12], times [300], the
    policy's commands [300, 4], per supervisor the commands [300, 4] and pre-call states [300, 4]."""
    from quadcopter_tracking.env import QuadcopterEnv

    env = QuadcopterEnv({"target": {"motion_type": motion}, "logging": {"enabled": False}})
    obs = env.reset(seed=seed)
    for s in sups:
        s.reset()
    O, T, U = [], [], []
    S = [[] for _ in sups]
    Z = [[] for _ in sups]
    for k in range(STEPS):
        q, t = obs["quadcopter"], obs["target"]
        O.append(np.concatenate([q["position"], q["velocity"], t["position"], t["velocity"]]).astype(float))
        T.append(float(obs["time"]))
        a = ctl.compute_action(obs)
        for j, s in enumerate(sups):
            Z[j].append(state_of(SUPERVISORS[j], s))
            c = s.compute_action(obs)
            S[j].append([c[k2] for k2 in KEYS])
        obs, _, done, _ = env.step(a)
        U.append([a[k2] for k2 in KEYS])
        assert not done or k == STEPS - 1, f"{motion} seed {seed}: the episode ends at step {k}"
    return np.array(O), np.array(T), np.array(U), np.array(S), np.array(Z)


def mse(u, s, dtype):
    import torch
    import torch.nn.functional as F

    labels = torch.tensor(s, dtype=torch.float32)  # the trainer's label tensor
    return float(F.mse_loss(torch.tensor(u, dtype=dtype), labels.to(dtype)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.dirname(os.path.abspath(__file__)))
    args = ap.parse_args()
    import_reference()
    import torch

    torch.set_num_threads(1)
    base = json.loads(str(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "deep_policy.npz"))
                          ["meta_json"]))["base_seeds"]
    sups = [make_supervisor(s) for s in SUPERVISORS]
    lqi = sups[[s["name"] for s in SUPERVISORS].index("lqi")]
    assert np.asarray(lqi.get_gain_matrix()).shape == (4, 9), "the LQI supervisor fell back to a 6-column gain"
    out = {}
    st = np.array(STORED)
    for name in NET_NAMES:
        pol = make_policy(next(s for s in NETS if s["name"] == name))
        dbl = Double(pol)
        for motion in MOTIONS:
            seeds = base[f"{name}/{motion}"] + np.arange(EPISODES)
            r32 = [flight(pol, sups, motion, int(s)) for s in seeds]
            r64 = [flight(dbl, sups, motion, int(s)) for s in seeds]
            fkey = f"{name}/{motion}"
            out[f"{fkey}/seeds"] = seeds
            out[f"{fkey}/obs"] = np.array([r[0][st] for r in r32])  # [4, 39, 12]
            out[f"{fkey}/time"] = np.array([r[1][st] for r in r32])  # [4, 39]
            for j, spec in enumerate(SUPERVISORS):
                key = f"{name}/{spec['name']}/{motion}"
                S32 = np.array([r[3][j] for r in r32])  # [4, 300, 4]
                S64 = np.array([r[3][j] for r in r64])
                gap = np.maximum.accumulate(np.abs(S32 - S64).max(axis=0), axis=0)  # [300, 4], every step up to it
                out[f"{key}/cmd"] = S32[:, st]
                out[f"{key}/cmd_gap"] = gap[st]
                if spec["type"] == "pid" or spec["config"].get("use_lqi"):
                    out[f"{key}/state"] = np.array([r[4][j][st] for r in r32])  # [4, 39, 4]
                l32 = np.array([mse(r[2], r[3][j], torch.float32) for r in r32])
                l64 = np.array([mse(r[2], r[3][j], torch.float64) for r in r64])
                out[f"{key}/loss"] = l32
                out[f"{key}/loss_gap"] = np.abs(l32 - l64).max()
                print(key, "loss", l32, "loss gap", out[f"{key}/loss_gap"], "cmd gap", gap[-1])
    out["meta_json"] = np.array(json.dumps({"nets": NET_NAMES, "supervisors": SUPERVISORS, "motions": MOTIONS,
                                            "episodes": EPISODES, "steps": STEPS, "stored": STORED}))
    path = os.path.join(args.out, "imitation.npz")
    save_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes")


def save_npz(path, arrays):
    """np.savez_compressed's file with fixed member timestamps: the same arrays give the same bytes."""
    import zipfile

    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(arrays[k]), allow_pickle=False)


if __name__ == "__main__":
    main()
