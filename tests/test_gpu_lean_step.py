"""GPU checks of the lean per-step frames (include/quadtrack.h ABI 10,
BatchedQuadcopterEnv(lean=True)).

The checker everywhere is the default env (full frames) on the same seeds
and controller: the lean path runs the same source expressions and must
give the same bits, so doubles are compared as int64 bit patterns (NaNs and
signed zeros count).  What the lean frame does not store — the target
observation, the time, the tracking error, the on-target ratio — is rebuilt
by qt_lean_expand and must equal the row the default path stored.
"""

import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

F64 = torch.float64
MOTIONS = ["stationary", "linear", "circular", "sinusoidal", "figure8"]


@pytest.fixture(scope="module")
def qt():
    import quadtrack

    quadtrack._abi.require_gpu()
    return quadtrack


def _bits(t):
    return t.view(torch.int64) if t.dtype == F64 else t


def _same(a, b, what=""):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(_bits(a), _bits(b)), what


def _frames_equal(lean_env, env, what=""):
    """The lean env's materialised frame against the default env's frame: every f, c and b row."""
    a, b = lean_env.frame, env.frame
    for name in ("f", "c", "b"):
        _same(getattr(a, name), getattr(b, name), f"{what} rows {name}")


def _ctl_state_equal(ca, cb, what=""):
    if ca.integral_state is None:
        assert cb.integral_state is None
    else:
        _same(ca.integral_state, cb.integral_state, f"{what} controller state")


# ------------------------------------------------------------ 1. closed step

CONTROLLERS = ["lqr_structured", "lqr_dense", "lqi", "pid"]
# every controller on every motion, and feed-forward LQR on the figure-8 (whose acceleration is the
# reference's forward difference); freeze_done and the integrator alternate so that every controller and
# every motion meets both values of both
CASES = [(c, m, (ci + mi) % 2 == 0, "rk4" if (ci + mi // 2) % 2 == 0 else "euler")
         for ci, c in enumerate(CONTROLLERS) for mi, m in enumerate(MOTIONS)]
CASES += [("lqr_ff", "figure8", True, "rk4"), ("lqr_ff", "figure8", False, "euler")]
STEPS = 300
CHECK_FRAMES = (0, 1, 2, 57, STEPS)


def _limits(i, motion, integrator):
    """Randomised limits in the manner of tests/test_gpu_pair.py::_limits, sized for
    300 steps: the position bound sits just above the target's height, inside
    the start offsets' range (z0 = 1 + U(-0.5, 0.5)), so that some episodes
    leave the box at once or while they track and others never do; the targets
    stay inside the box; the time limit lies beyond the loop; the speed clamp
    is low enough to act."""
    r = np.random.default_rng(7000 + i)
    dt = float(r.choice([0.005, 0.01, 0.02]))
    horizon = STEPS * dt
    speed = float(r.uniform(0.2, 0.6)) / horizon if motion == "linear" else float(r.uniform(0.1, 0.4))
    env = {"target": {"motion_type": motion, "speed": speed, "radius": float(r.uniform(0.2, 0.4)),
                      "amplitude": float(r.uniform(0.2, 0.5))},
           "simulation": {"dt": dt, "max_velocity": float(r.uniform(0.3, 2.0)),
                          "max_position": float(r.uniform(1.15, 1.4)),
                          "max_episode_time": float(np.round(horizon + r.uniform(1.0, 3.0), 3)),
                          "integrator": integrator},
           "quadcopter": {"max_angular_rate": 3.0}}
    ctl = {"dt": dt, "max_rate": float(r.uniform(1.0, 3.0)), "q_pos": [float(r.uniform(1e-4, 5.0))] * 2 + [16.0]}
    return env, ctl


def _controller(kind, cfg):
    from quadtrack.controllers import BatchedPID, BatchedRiccatiLQR

    if kind == "pid":
        return BatchedPID({"dt": cfg["dt"], "max_rate": cfg["max_rate"]})
    if kind == "lqi":
        return BatchedRiccatiLQR(dict(cfg, use_lqi=True, q_int=[1e-3, 1e-3, 1e-2]))
    if kind == "lqr_ff":
        return BatchedRiccatiLQR(dict(cfg, feedforward_enabled=True))
    ctl = BatchedRiccatiLQR(cfg)
    if kind == "lqr_dense":
        assert ctl.k_structured
        ctl.k_structured = False  # the same gain through the dense K @ s kernel
    return ctl


def _closed_pair(qt, n, env_cfg, make_ctl, freeze, steps, seeds, check_frames, **per_episode):
    """Drive the default and the lean env side by side; returns the default env's done flags per step."""
    envs = [qt.BatchedQuadcopterEnv(n, env_cfg, freeze_done=freeze, lean=lean, **per_episode)
            for lean in (False, True)]
    ctls = [make_ctl(), make_ctl()]
    for env, ctl in zip(envs, ctls):
        ctl.reset(n)
        env.reset(seeds)
    env, lean = envs
    assert lean.lean and not env.lean
    dones = []
    if 0 in check_frames:
        _frames_equal(lean, env, "reset")
    for k in range(1, steps + 1):
        _, r0, d0, i0 = env.step_closed(ctls[0])
        _, r1, d1, i1 = lean.step_closed(ctls[1])
        _same(r1, r0, f"step {k} reward")
        _same(d1, d0, f"step {k} done")
        _same(i1["action"], i0["action"], f"step {k} action")
        dones.append(d0.clone())
        if k in check_frames:
            _frames_equal(lean, env, f"step {k}")
            _ctl_state_equal(ctls[1], ctls[0], f"step {k}")
    return torch.stack(dones)


@pytest.mark.parametrize("kind,motion,freeze,integrator", CASES,
                         ids=[f"{c}-{m}-{'freeze' if f else 'stepon'}-{g}" for c, m, f, g in CASES])
def test_lean_closed_step_bitwise(qt, kind, motion, freeze, integrator):
    i = CASES.index((kind, motion, freeze, integrator))
    env_cfg, ctl_cfg = _limits(i, motion, integrator)
    ended_early = still_runs = False
    for n in (1, 65, 777):
        dones = _closed_pair(qt, n, env_cfg, lambda: _controller(kind, ctl_cfg), freeze, STEPS,
                             np.arange(n) + 31 * i, CHECK_FRAMES)
        early, runs = bool(dones[:-1].any()), bool((~dones[-1]).any())
        if n > 1:  # one episode cannot do both
            assert early and runs, (n, early, runs)
        ended_early |= early
        still_runs |= runs
    # on the default env's output: the loop saw an episode end before its last step and one still running
    assert ended_early and still_runs


# ------------------------------------------- 2. per-episode motion and mass

def test_lean_per_episode_motion_and_mass_bitwise(qt):
    from quadtrack.controllers import BatchedRiccatiLQR

    n = 700
    motion = np.arange(n) % 5
    mass = 0.8 + 0.4 * ((np.arange(n) * 2654435761) % 1000) / 1000.0
    env_cfg, ctl_cfg = _limits(99, "stationary", "rk4")
    env_cfg["target"].pop("motion_type")
    env_cfg["target"]["speed"] = 0.15
    dones = _closed_pair(qt, n, env_cfg, lambda: BatchedRiccatiLQR(ctl_cfg, mass=mass), True, STEPS,
                         np.arange(n) + 5, CHECK_FRAMES, motion=motion, mass=mass)
    assert bool(dones[:-1].any()) and bool((~dones[-1]).any())


# ---------------------------------------------------------- 3. open loop

def test_lean_open_loop_step_bitwise(qt):
    """The open_loop.npz action cases (NaN, Inf, out of range, position-bound
    exit) through env.step: lean equals default in every row at every step."""
    OL = np.load(os.path.join(GOLDEN, "open_loop.npz"))
    cases = json.loads(str(OL["cases_json"]))
    n = 65
    violations = 0
    for ci, case in enumerate(cases):
        cfg = json.loads(json.dumps(case["env"]))
        cfg.setdefault("target", {})["motion_type"] = case["motion"]
        for freeze in (False, True):
            env = qt.BatchedQuadcopterEnv(n, cfg, freeze_done=freeze)
            lean = qt.BatchedQuadcopterEnv(n, cfg, freeze_done=freeze, lean=True)
            env.reset(np.full(n, case["seed"]))
            lean.reset(np.full(n, case["seed"]))
            for k in range(len(OL["actions"])):
                a = torch.as_tensor(np.broadcast_to(OL["actions"][k], (n, 4)).copy(), device=env.device)
                _, r0, d0, i0 = env.step(a)
                _, r1, d1, i1 = lean.step(a)
                _same(r1, r0, f"case {ci} step {k} reward")
                _same(d1, d0, f"case {ci} step {k} done")
                assert "action" not in i1
                _same(i1["action_violations"], i0["action_violations"], f"case {ci} step {k} violations")
                _same(i1["violation"], i0["violation"], f"case {ci} step {k} violation flag")
                _frames_equal(lean, env, f"case {ci} step {k}")
            violations += int(i0["action_violations"].sum())
    assert violations > 0


# ------------------------------------------- 4. the reference's fixtures

def _scenarios():
    import test_gpu_batched_env as T

    return T


def _scenario_names():
    return [s["name"] for s in json.load(open(os.path.join(GOLDEN, "scenarios.json")))["scenarios"]]


@pytest.mark.parametrize("name", _scenario_names())
def test_lean_loop_matches_reference(qt, name):
    """The closed_loop.npz scenarios of test_gpu_batched_env.py driven with
    lean=True, against the reference's fixture at the same 1e-5 / 1e-8."""
    T = _scenarios()
    s = next(x for x in T.SCENARIOS if x["name"] == name)
    make, env_cfg, motion, mass, n = T._setup(s)
    ctl = make()
    env = qt.BatchedQuadcopterEnv(n, env_cfg, motion=motion, mass=mass, lean=True)
    ctl.reset(n)
    obs = env.reset(s["seeds"])
    dev = env.device
    done_prev = torch.zeros(n, dtype=torch.bool, device=dev)
    sum_pre = torch.zeros(n, dtype=F64, device=dev)
    integ_end = torch.full((3, n), float("nan"), dtype=F64, device=dev)
    for _ in range(4000):
        d = obs["quadcopter"]["position"] - obs["target"]["position"]
        pre = torch.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        obs, reward, done, info = env.step_closed(ctl)
        active = ~done_prev
        sum_pre += torch.where(active, pre, torch.zeros_like(pre))
        if ctl.integral_state is not None:
            integ_end = torch.where((done & active)[None, :], ctl.integral_state[:3], integ_end)
        done_prev = done.clone()
        if bool(done.all()):
            break
    assert bool(done_prev.all()), "episodes did not finish"
    ref = T.CL[name + "_metrics"]
    col = lambda f: ref[:, T.FIELDS.index(f)]  # noqa: E731
    steps = info["step"].cpu().numpy()
    np.testing.assert_array_equal(steps, col("steps"))
    np.testing.assert_array_equal(info["termination_code"].cpu().numpy(), col("termination_code"))
    np.testing.assert_array_equal(info["action_violations"].cpu().numpy(), col("action_violations"))
    np.testing.assert_allclose(info["on_target_ratio"].cpu().numpy(), col("env_on_target_ratio"), rtol=0, atol=1e-12)
    np.testing.assert_allclose(info["time"].cpu().numpy(), col("episode_duration"), rtol=0, atol=1e-12)
    np.testing.assert_allclose(env.time.cpu().numpy(), col("episode_duration"), rtol=0, atol=1e-12)
    np.testing.assert_allclose(sum_pre.cpu().numpy() / steps, col("mean_tracking_error"), rtol=1e-8, atol=T.TOL)
    fin = T.CL[name + "_final"]
    np.testing.assert_allclose(env.get_state_vector().cpu().numpy(), fin[:, :12], rtol=1e-8, atol=T.TOL)
    if ctl.use_lqi or ctl.kind == "pid":
        np.testing.assert_allclose(integ_end.cpu().numpy().T, fin[:, 12:], rtol=1e-8, atol=T.TOL)


# ------------------------------------------------------------ 5. laziness

def test_lean_results_are_lazy(qt):
    from quadtrack.controllers import BatchedRiccatiLQR

    n = 193
    env = qt.BatchedQuadcopterEnv(n, {"target": {"motion_type": "circular"}}, lean=True)
    ctl = BatchedRiccatiLQR({"dt": 0.01})
    ctl.reset(n)
    env.reset(np.arange(n))
    frames = set()
    for _ in range(50):
        obs, rew, done, info = env.step_closed(ctl)
        frames.add(id(env._frame))
        assert list(obs) == ["quadcopter", "target", "time"] and "tracking_error" in info and len(info) == 12
        assert obs["quadcopter"]["position"].shape == (n, 3) and info["action"].shape == (n, 4)
        del obs, rew, done, info
    assert env.expand_launches == 0
    assert len(env._pool.frames) <= 3 and len(frames) <= 3
    obs, rew, done, info = env.step_closed(ctl)
    assert env.expand_launches == 0
    tp = obs["target"]["position"]
    assert env.expand_launches == 1
    assert obs["time"].shape == (n,) and info["tracking_error"].shape == (n,) and obs.frame.n == n
    assert obs["target"]["position"] is tp and info.get("step") is info["step"]
    assert env.frame is obs.frame and env.observation()["target"]["velocity"].shape == (n, 3)
    assert env.expand_launches == 1
    _same(info["tracking_error"], -rew, "err = -reward")
    # a default env never expands
    assert qt.BatchedQuadcopterEnv(4, {}).expand_launches == 0


# --------------------------------------------------------- 6. hold contract

def test_lean_kept_results_never_change(qt):
    from quadtrack.controllers import BatchedRiccatiLQR

    n = 257
    env = qt.BatchedQuadcopterEnv(n, {"target": {"motion_type": "sinusoidal"}}, lean=True)
    ctl = BatchedRiccatiLQR({"dt": 0.01})
    ctl.reset(n)
    env.reset(np.arange(n))
    for _ in range(3):
        obs, rew, done, info = env.step_closed(ctl)
    kept_obs, kept_rew = obs, rew
    tensors = {"position": obs["quadcopter"]["position"], "velocity": obs["quadcopter"]["velocity"],
               "target": obs["target"]["position"], "time": obs["time"], "reward": rew}  # materialises the obs
    copies = {k: v.clone() for k, v in tensors.items()}
    del obs, rew, done, info
    for _ in range(20):
        env.step_closed(ctl)
    for k, v in tensors.items():
        _same(v, copies[k], k)
    _same(kept_obs["target"]["position"], copies["target"])
    _same(kept_rew, copies["reward"])
    assert not torch.equal(env.observation()["quadcopter"]["position"], copies["position"])
    assert len(env._pool.frames) <= env._pool.size


# ----------------------------------------------------------- 7. table growth

def test_lean_time_table_grows(qt):
    """Stepping past the time limit (freeze_done=False) runs off the initial
    table (max_episode_time / dt entries): the env extends it before the
    launch and every row, the time row included, stays the default's."""
    from quadtrack.controllers import BatchedRiccatiLQR

    n, steps = 130, 100
    cfg = {"target": {"motion_type": "circular"}, "simulation": {"dt": 0.02, "max_episode_time": 0.2}}
    probe = qt.BatchedQuadcopterEnv(n, cfg, freeze_done=False, lean=True)
    len0 = probe._table.len
    assert len0 < steps
    envs = [qt.BatchedQuadcopterEnv(n, cfg, freeze_done=False, lean=lean) for lean in (False, True)]
    ctls = [BatchedRiccatiLQR({"dt": 0.02}), BatchedRiccatiLQR({"dt": 0.02})]
    for env, ctl in zip(envs, ctls):
        ctl.reset(n)
        env.reset(np.arange(n))
    env, lean = envs
    for k in range(1, steps + 1):
        _, r0, d0, i0 = env.step_closed(ctls[0])
        _, r1, d1, i1 = lean.step_closed(ctls[1])
        _same(r1, r0, f"step {k} reward")
        _same(d1, d0, f"step {k} done")
        _same(i1["action"], i0["action"], f"step {k} action")
        _same(i1["time"], i0["time"], f"step {k} time")
        _same(lean.time, env.time, f"step {k} env.time")
        _frames_equal(lean, env, f"step {k}")
    assert lean._table.len > steps > len0
    assert bool(d0.all()) and int(i0["step"].min()) == steps  # stepped on after the time limit


# ---------------------------------------------------------------- 8. the rest

def test_lean_set_state_vector(qt):
    from quadtrack.controllers import BatchedRiccatiLQR

    n = 65
    envs = [qt.BatchedQuadcopterEnv(n, {"target": {"motion_type": "linear"}}, lean=lean) for lean in (False, True)]
    ctls = [BatchedRiccatiLQR({"dt": 0.01}), BatchedRiccatiLQR({"dt": 0.01})]
    x = torch.as_tensor(np.random.default_rng(3).uniform(-0.3, 0.3, (n, 12)), device=envs[0].device)
    for env, ctl in zip(envs, ctls):
        env.reset(np.arange(n))
        for _ in range(4):
            env.step_closed(ctl)
        env.set_state_vector(x)
        _same(env.get_state_vector(), x)
        _same(env.observation()["quadcopter"]["velocity"], x[:, 3:6].contiguous())
        for _ in range(4):
            env.step_closed(ctl)
    _frames_equal(envs[1], envs[0], "after set_state_vector")
    _same(envs[1].time, envs[0].time)
    with pytest.raises(ValueError, match="shape"):
        envs[1].set_state_vector(x[:, :11])


def test_lean_in_place_modification_is_refused(qt):
    from quadtrack.controllers import BatchedRiccatiLQR

    n = 257
    env = qt.BatchedQuadcopterEnv(n, {"target": {"motion_type": "circular"}}, lean=True)
    ctl = BatchedRiccatiLQR({"dt": 0.01})
    obs = env.reset(np.arange(n))
    for _ in range(3):  # the two-call loop on lean observations: one expand per step
        obs, _, _, _ = env.step(ctl.compute_action(obs))
    assert env.expand_launches == 3
    obs["quadcopter"]["position"].add_(1.0)
    with pytest.raises(RuntimeError, match="modified in place"):
        env.step(ctl.compute_action(obs))
    with pytest.raises(RuntimeError, match="modified in place"):
        env.step_closed(ctl)


def test_lean_two_call_loop_equals_closed_step(qt):
    """compute_action on a lean observation (materialised through obs.frame),
    then step: bitwise the one-launch lean step_closed."""
    from quadtrack.controllers import BatchedRiccatiLQR

    n = 300
    cfg = {"target": {"motion_type": "sinusoidal"}}
    ctl_cfg = {"dt": 0.01, "use_lqi": True, "q_int": [1e-3, 1e-3, 1e-2]}
    envs = [qt.BatchedQuadcopterEnv(n, cfg, lean=True) for _ in range(2)]
    ctls = [BatchedRiccatiLQR(ctl_cfg), BatchedRiccatiLQR(ctl_cfg)]
    obs = [env.reset(np.arange(n) + 5) for env in envs]
    for ctl in ctls:
        ctl.reset(n)
    for _ in range(60):
        o, r0, _, _ = envs[0].step(ctls[0].compute_action(obs[0]))
        obs[0] = o
        _, r1, _, _ = envs[1].step_closed(ctls[1])
        _same(r0, r1)
    _frames_equal(envs[0], envs[1])
    _ctl_state_equal(ctls[0], ctls[1])
    assert envs[0].expand_launches == 60 + 1 and envs[1].expand_launches == 1


def test_lean_mixed_devices_refused(qt):
    from quadtrack.controllers import BatchedRiccatiLQR

    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    env = qt.BatchedQuadcopterEnv(8, {}, device="cuda:0", lean=True)
    ctl = BatchedRiccatiLQR({"dt": 0.01}, device="cuda:1")
    obs = env.reset(np.arange(8))
    with pytest.raises(ValueError, match="controller"):
        env.step_closed(ctl)
    with pytest.raises(ValueError):
        ctl.compute_action(obs)


def test_lean_empty_and_single_episode_batches(qt):
    """test_gpu_batched_env.py::test_empty_and_single_episode_batches with lean=True."""
    from quadtrack.controllers import BatchedRiccatiLQR

    ctl = BatchedRiccatiLQR({"dt": 0.01})
    env = qt.BatchedQuadcopterEnv(0, {}, lean=True)
    obs = env.reset([])
    a = ctl.compute_action(obs)
    assert tuple(a.shape) == (0, 4)
    obs, r, done, info = env.step(a)
    assert r.numel() == 0 and done.numel() == 0
    env = qt.BatchedQuadcopterEnv(1, {}, lean=True)
    obs = env.reset([0])
    for _ in range(3000):
        obs, r, done, info = env.step_closed(ctl)
    # SURVEY §6 config-1 known answer: seed 0, stationary, final position
    np.testing.assert_allclose(obs["quadcopter"]["position"][0].cpu().numpy(),
                               [0.0673493918, -0.1132311124, 0.9999439135], atol=1e-9)
    assert bool(done[0]) and info["termination_code"][0] == 1
    assert float(info["on_target_ratio"][0]) == pytest.approx(0.992667, abs=1e-6)
    assert env.expand_launches == 1
