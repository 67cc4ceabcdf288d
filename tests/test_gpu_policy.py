"""Deep tracking policy on the GPU: the action kernel and the fused policy
rollout against the reference fixture (tests/golden/deep_policy.npz) and
against each other.

Tolerance rule (derived from the reference alone): a device value may differ
from the reference's f32 value by at most 4 x the largest difference between
the reference's own f32 and float64 runs of the same quantity, component and
step horizon (stored in the fixture), with the tolerance of the recorded
rollout parity tests (tests/test_gpu_parity.py: 1e-5 absolute, 1e-8 relative)
as the floor.
"""

import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import oracle as O
import quadtrack
from quadtrack import core
from quadtrack._abi import ACC_STEPS, ACC_TERM
from quadtrack.policy import policy_batch, run_policy_loop

pytestmark = pytest.mark.gpu

FX = np.load(os.path.join(GOLDEN, "deep_policy.npz"))
META = json.loads(str(FX["meta_json"]))
DEV = "cuda:0"
ATOL, RTOL = 1e-5, 1e-8  # the floor: tests/test_gpu_parity.py's recorded-rollout tolerance
CHECKPOINTS = META["checkpoints"]


def tol_of(gap, ref):
    return np.maximum(4.0 * np.asarray(gap), ATOL + RTOL * np.abs(ref))


def state_dict_of(name):
    pre = f"{name}/sd/"
    return {k[len(pre):]: torch.from_numpy(FX[k]) for k in FX.files if k.startswith(pre)}


_POLICIES = {}


def policy_of(name) -> quadtrack.BatchedDeepPolicy:
    if name not in _POLICIES:
        s = next(s for s in META["nets"] if s["name"] == name)
        ob = {k: tuple(v) for k, v in s["output_bounds"].items()} if "output_bounds" in s else None
        _POLICIES[name] = quadtrack.BatchedDeepPolicy.from_state_dict(state_dict_of(name), s["hidden_sizes"],
                                                                      s["activation"], ob, device=DEV)
    return _POLICIES[name]


def obs_tensors(rows):
    """[k, 6, 3] fixture observations -> the observation dict of [k, 3] device tensors."""
    t = torch.as_tensor(np.ascontiguousarray(rows), dtype=torch.float64, device=DEV)
    q = {k: t[:, i] for i, k in enumerate(("position", "velocity", "attitude", "angular_velocity"))}
    return {"quadcopter": q, "target": {"position": t[:, 4], "velocity": t[:, 5]}}


# ------------------------------------------------------------------ 1. action parity

@pytest.mark.parametrize("name", [s["name"] for s in META["nets"]])
def test_action_parity(name):
    a = policy_of(name).compute_action(obs_tensors(FX["obs"])).cpu().numpy()
    ref, ref64 = FX[f"{name}/act32"], FX[f"{name}/act64"]
    gap = np.abs(ref - ref64).max(axis=0)  # per action component, over the 512 observations
    err = np.abs(a - ref)
    print(name, "max |device - ref f32|", err.max(axis=0), "ref f32-f64 gap", gap, "ratio", err.max(axis=0) / np.maximum(gap, 1e-300),
          "worst observation per component", err.argmax(axis=0))
    assert a.shape == (512, 4) and np.isfinite(a).all()
    assert (err <= tol_of(gap[None, :], ref)).all(), (err.max(axis=0), gap)
    # the f32 result widened exactly
    assert np.array_equal(a, a.astype(np.float32).astype(np.float64))


def test_single_observation_drop_in():
    """DeepTrackingPolicy.compute_action (n = 1) gives the batched row, as a dict of floats."""
    s = next(s for s in META["nets"] if s["name"] == "n1")
    pol = quadtrack.DeepTrackingPolicy({"hidden_sizes": s["hidden_sizes"], "activation": s["activation"]}, device=DEV)
    pol.network.load_state_dict(state_dict_of("n1"))
    batch = policy_of("n1").compute_action(obs_tensors(FX["obs"][60:64])).cpu().numpy()
    for j, r in enumerate(FX["obs"][60:64]):
        a = pol.compute_action({"quadcopter": {"position": r[0], "velocity": r[1], "attitude": r[2],
                                               "angular_velocity": r[3]},
                                "target": {"position": r[4], "velocity": r[5]}})
        assert list(a) == ["thrust", "roll_rate", "pitch_rate", "yaw_rate"] and all(type(v) is float for v in a.values())
        assert [a[k] for k in a] == batch[j].tolist()
    pol.reset()
    assert pol.to_batched().device == torch.device(DEV)


# ------------------------------------------------- 2. lane and batch independence

@pytest.mark.parametrize("name", ["n0", "n4", "n5", "n3"])
def test_lane_and_batch_independence(name):
    pol = policy_of(name)
    full = pol.compute_action(obs_tensors(FX["obs"]))
    for k in (1, 63, 64, 65, 130):
        part = pol.compute_action(obs_tensors(FX["obs"][:k]))
        assert torch.equal(part, full[:k]), k
    # an episode's result does not depend on its lane or on its neighbours
    perm = np.random.default_rng(0).permutation(512)
    shuffled = pol.compute_action(obs_tensors(FX["obs"][perm]))
    assert torch.equal(shuffled, full[torch.as_tensor(perm, device=DEV)])
    # strided inputs (the transpose of an SoA block) give the same bits
    soa = torch.as_tensor(FX["obs"][:130], dtype=torch.float64, device=DEV).permute(1, 2, 0).contiguous()  # [6, 3, n]
    q = {k: soa[i].T for i, k in enumerate(("position", "velocity", "attitude", "angular_velocity"))}
    assert torch.equal(pol.compute_action({"quadcopter": q, "target": {"position": soa[4].T, "velocity": soa[5].T}}),
                       full[:130])
    frozen = torch.zeros(130, dtype=torch.int8, device=DEV)
    frozen[[0, 64, 129]] = 1
    fz = pol.compute_action(obs_tensors(FX["obs"][:130]), frozen)
    assert not fz[[0, 64, 129]].any() and torch.equal(fz[1:64], full[1:64]) and torch.equal(fz[65:129], full[65:129])


# ------------------------------------------------------- the shared recorded run

N, STEPS = 130, 40
MOTION = [quadtrack._abi.MOTIONS[i % 5] for i in range(N)]
MASS = np.linspace(0.8, 1.3, N)
ENV_CFG = {"target": {"motion_type": "linear"}}


# every rollout kernel: n4 one 32-row tile (NT = 1), n3 two tiles and three hidden layers (NT = 2), n5 [128, 128] (NT = 4)
ROLLOUT_NETS = ["n4", "n3", "n5"]


@pytest.fixture(scope="module", params=ROLLOUT_NETS)
def recorded(request):
    res = run_policy_loop(policy_of(request.param), ENV_CFG, n=N, seeds=np.arange(N) + 5, motion=MOTION, plant_mass=MASS,
                          max_steps=STEPS, record=True)
    torch.cuda.synchronize()
    res.net = request.param
    return res


def test_rollout_and_action_kernel_agree_bitwise(recorded):
    """The command the rollout recorded at every step is, bit for bit, what the
    action kernel gives on that step's observation (rebuilt from the record
    and qt_target_state by RolloutResult.trajectories, which re-runs the
    policy rollout)."""
    pol = policy_of(recorded.net)
    tr = recorded.trajectories()
    assert int(tr["steps"].min()) == STEPS
    assert torch.equal(tr["next_state"], recorded.record[:, :12])  # the re-run is the policy rollout
    assert torch.equal(tr["action"], recorded.record[:, 12:])
    for s in range(STEPS):
        x, tg = tr["obs_state"][s], tr["obs_target"][s]  # [12, n], [9, n]
        obs = {"quadcopter": {"position": x[0:3].T, "velocity": x[3:6].T, "attitude": x[6:9].T,
                              "angular_velocity": x[9:12].T},
               "target": {"position": tg[0:3].T, "velocity": tg[3:6].T}}
        assert torch.equal(pol.compute_action(obs), recorded.record[s, 12:].T), s
    data = recorded.episode_data([3])
    assert len(data[0]) == STEPS and data[0][7]["action"] == recorded.record[7, 12:, 3].tolist()


def test_recorded_steps_against_oracle_env_step(recorded):
    """Every recorded step from the recorded previous state and command through the CPU oracle's env.step."""
    env = O.env_params(ENV_CFG)
    rec = recorded.record.cpu().numpy()
    pat = recorded.batch.pattern.cpu().numpy().T
    off = recorded.batch.offset.cpu().numpy().T
    worst = 0.0
    for e in range(N):
        m = e % 5
        x, t = O.initial_state(env, m, pat[e], off[e]), 0.0
        for s in range(STEPS):
            xn, t, _, _, _, term = O.env_step(env, m, pat[e], MASS[e], x, t, rec[s, 12:, e])
            assert term == 0
            worst = max(worst, float(np.abs(xn - rec[s, :12, e]).max()))
            np.testing.assert_allclose(rec[s, :12, e], xn, rtol=RTOL, atol=ATOL, err_msg=f"episode {e} step {s}")
            x = rec[s, :12, e]
    print("max |device step - oracle step|", worst)
    # the accumulators agree with the record
    assert (recorded.metric("steps") == STEPS).all()
    u = rec[:, 12:]
    effort = np.sqrt((u * u).sum(axis=1)).sum(axis=0)
    np.testing.assert_allclose(recorded.metric("total_control_effort").cpu().numpy(), effort, rtol=1e-12)


def test_chunked_and_one_launch_agree_bitwise(recorded):
    res = run_policy_loop(policy_of(recorded.net), ENV_CFG, n=N, seeds=np.arange(N) + 5, motion=MOTION,
                          plant_mass=MASS, max_steps=STEPS, chunk=7, record=True)
    assert torch.equal(res.record, recorded.record)
    assert torch.equal(res.metrics, recorded.metrics)
    for k in ("x", "t", "acc", "target"):
        assert torch.equal(getattr(res.state, k), getattr(recorded.state, k)), k
    plain = run_policy_loop(policy_of(recorded.net), ENV_CFG, n=N, seeds=np.arange(N) + 5, motion=MOTION,
                            plant_mass=MASS, max_steps=STEPS)
    assert plain.record is None and torch.equal(plain.metrics, recorded.metrics)
    assert torch.equal(plain.state.x, recorded.state.x)


# ------------------------------------------- 6. closed loop against the reference

@pytest.mark.parametrize("motion", META["motions"])
@pytest.mark.parametrize("name", META["closed"])
def test_closed_loop_against_reference(name, motion):
    key = f"{name}/{motion}"
    seeds = FX[f"{key}/seeds"]
    cfg = {"target": {"motion_type": motion}}
    res = run_policy_loop(policy_of(name), cfg, n=len(seeds), seeds=seeds, max_steps=META["steps"], record=True)
    rec = res.record.cpu().numpy()
    ref, gap = FX[f"{key}/states"], FX[f"{key}/state_gap"]  # [8, 4, 12], [4, 12]
    aref, agap = FX[f"{key}/actions"], FX[f"{key}/action_gap"]
    for j, c in enumerate(CHECKPOINTS):
        got = rec[c - 1, :12].T
        err = np.abs(got - ref[:, j])
        print(key, "step", c, "max state err", err.max(), "ref gap", gap[j].max())
        assert (err <= tol_of(gap[j][None, :], ref[:, j])).all(), (c, err.max(axis=0), gap[j])
        uerr = np.abs(rec[c - 1, 12:].T - aref[:, j])
        assert (uerr <= tol_of(agap[j][None, :], aref[:, j])).all(), (c, uerr.max(axis=0), agap[j])
    assert (res.metric("steps") == META["steps"]).all() and (res.metric("termination_code") == 0).all()
    if name != "lqr":
        return
    # per-episode metrics of the reference Evaluator: counts exact, means under the rule
    F = META["fields"]
    want, mgap = FX[f"{key}/metrics"], FX[f"{key}/metrics_gap"]
    got = np.stack([res.metric(f).cpu().numpy() for f in F], axis=1)
    for f in ("on_target_ratio", "overshoot_count", "success"):
        assert np.array_equal(got[:, F.index(f)], want[:, F.index(f)]), f
    np.testing.assert_allclose(got[:, F.index("episode_duration")], want[:, F.index("episode_duration")], rtol=1e-12)
    for f in ("mean_tracking_error", "max_tracking_error", "rms_tracking_error", "total_control_effort",
              "mean_control_effort", "max_overshoot"):
        i = F.index(f)
        err = np.abs(got[:, i] - want[:, i])
        print(key, f, "max err", err.max(), "ref gap", mgap[i])
        assert (err <= tol_of(mgap[i], want[:, i])).all(), (f, err.max(), mgap[i])
    # evaluate_policy's summary against the Evaluator's
    S = META["summary"]
    sref = dict(zip(S, FX[f"{key}/summary"]))
    summ = quadtrack.evaluate_policy(policy_of(name), cfg, num_episodes=len(seeds), base_seed=int(seeds[0]),
                                     max_steps_per_episode=META["steps"])
    for k in ("total_episodes", "successful_episodes", "success_rate", "best_episode_idx", "worst_episode_idx",
              "meets_criteria"):
        assert float(getattr(summ, k)) == sref[k], k
    for k in ("mean_on_target_ratio", "std_on_target_ratio"):
        assert float(getattr(summ, k)) == pytest.approx(sref[k], rel=1e-12, abs=1e-15), k
    for k, f in (("mean_tracking_error", "mean_tracking_error"), ("std_tracking_error", "mean_tracking_error"),
                 ("mean_control_effort", "mean_control_effort")):
        t = float(tol_of(mgap[F.index(f)], sref[k]))
        assert abs(float(getattr(summ, k)) - sref[k]) <= t, (k, float(getattr(summ, k)), sref[k], t)
    assert len(summ.episode_metrics) == len(seeds)
    assert summ.episode_metrics[0].on_target_ratio == want[0, F.index("on_target_ratio")]


# ------------------------------------------------------------------ 7. early end

@pytest.mark.parametrize("name", ["n0", "n5"])
def test_early_end_freezes_episodes(name):
    cfg = {"target": {"motion_type": "circular"}, "simulation": {"max_episode_time": 0.2}}
    dt, t, want = 0.01, 0.0, 0
    while not t >= 0.2:  # the reference's clock: t += dt, done when t >= max_episode_time
        t += dt
        want += 1
    n = 70
    res = run_policy_loop(policy_of(name), cfg, n=n, seeds=np.arange(n), max_steps=want, chunk=7)
    assert (res.metric("steps") == want).all() and (res.metric("termination_code") == 1).all()
    assert res.episode_metrics()[0].termination_reason == "time_limit"
    longer = run_policy_loop(policy_of(name), cfg, n=n, seeds=np.arange(n), max_steps=want + 15, chunk=7, record=True)
    for k in ("x", "t", "acc", "target"):
        assert torch.equal(getattr(longer.state, k), getattr(res.state, k)), k
    assert torch.equal(longer.metrics, res.metrics)
    assert torch.isnan(longer.record[want:]).all() and not torch.isnan(longer.record[:want]).any()


# ------------------------------------------------------------------ 8. isolation

@pytest.mark.parametrize("name", ["n0", "n5"])
def test_nan_episode_is_isolated(name):
    """One episode whose state is NaN ends as numerical_instability; every
    other episode of its wave and batch is bitwise what it is without it
    (plain NaN arithmetic in that lane's column)."""
    pol = policy_of(name)
    cfg = quadtrack.env.config.as_env_config(ENV_CFG)
    env, crit = cfg.to_params(), core.criteria()
    bad = 70

    def run(poison):
        batch = policy_batch(cfg, N, DEV, seeds=np.arange(N), motion=MOTION, plant_mass=MASS)
        st = core.RolloutState.empty(N, batch.device)
        core.reset(env, batch, st)
        if poison:
            st.x[:, bad] = float("nan")
        for _ in range(3):
            pol.rollout(env, crit, batch, st, 5)
        return st

    a, b = run(False), run(True)
    keep = torch.arange(N, device=DEV) != bad
    for k in ("x", "acc", "target"):
        assert torch.equal(getattr(a, k)[:, keep], getattr(b, k)[:, keep]), k
    assert torch.equal(a.t[keep], b.t[keep])
    assert int(b.acc[ACC_TERM, bad]) == 3 and int(b.acc[ACC_STEPS, bad]) == 1
    assert quadtrack._abi.TERM_REASONS[3] == "numerical_instability"
    assert (a.acc[ACC_TERM] == 0).all() and (a.acc[ACC_STEPS] == 15).all()


# ---------------------------------------------------------------- 9. per-step API

@pytest.mark.parametrize("lean", [False, True])
def test_step_closed_matches_two_calls(lean):
    pol = policy_of("n2")
    n = 130
    mk = lambda: quadtrack.BatchedQuadcopterEnv(n, ENV_CFG, device=DEV, motion=MOTION, mass=MASS, lean=lean)  # noqa: E731
    ea, eb = mk(), mk()
    ea.reset(np.arange(n))
    obs = eb.reset(np.arange(n))
    out = torch.as_tensor([5000.0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], dtype=torch.float64, device=DEV)
    for k in range(20):
        if k == 6:  # two episodes leave the position bounds: done at this step, frozen afterwards
            for e in (ea, eb):
                x = e.get_state_vector()
                x[[3, 64]] = out
                e.set_state_vector(x)
            obs = eb.observation()
        oa, ra, da, ia = ea.step_closed(pol)
        act = pol.compute_action(obs)
        obs, rb, db, ib = eb.step(act)
        done_before = torch.zeros(n, dtype=torch.bool, device=DEV) if k <= 6 else prev_done
        assert torch.equal(ia["action"][~done_before], act[~done_before]), k
        assert not ia["action"][done_before].any(), k  # freeze_done: a done episode's action row is 0
        assert torch.equal(ra, rb) and torch.equal(da, db), k
        assert torch.equal(ea.get_state_vector(), eb.get_state_vector()), k
        assert torch.equal(oa["target"]["position"], obs["target"]["position"]), k
        assert torch.equal(ia["tracking_error"], ib["tracking_error"]), k
        prev_done = da.clone()
    assert prev_done[[3, 64]].all() and int(prev_done.sum()) == 2
    with pytest.raises(ValueError):  # a mixed-device call
        pol.compute_action({"quadcopter": {k: v.cpu() for k, v in obs["quadcopter"].items()},
                            "target": {k: obs["target"][k].cpu() for k in ("position", "velocity")}})
