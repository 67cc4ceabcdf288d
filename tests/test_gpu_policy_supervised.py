"""The supervised policy rollout on the GPU (qt_policy_supervised_rollout): the
flight is the policy rollout's bit for bit, the teacher's labels and integral
state are the per-step API's bit for bit, the samples are the full record at
their steps, the loss is the FP64 sum of the recorded differences, chunks and
lane placement change nothing, and the labels agree with the reference fixture
(tests/golden/imitation.npz) under tests/test_gpu_policy.py's tolerance rule:
4 x the reference's own f32-vs-float64 gap, floor 1e-5 absolute + 1e-8 relative.

Measured on one MI355X (profiles/r13/gpu_policy_supervised_tests.txt): over the 16 fixture runs the
teacher commands reach at most 0.60 of that bound (n1 / lqr / stationary, 6.1e-6) and the imitation
loss at most 0.56 of its bound (5.9e-6 at a loss of 38); the loss equals the FP64 sum of the record
exactly (relative error 0) in every case.
"""

import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import policy_model as M
import quadtrack
from quadtrack import _abi, core
from quadtrack.controllers import BatchedLQR, BatchedPID, BatchedRiccatiLQR, batched_controller
from quadtrack.policy import SupervisedResult, run_policy_loop, run_policy_supervised, sample_steps
from quadtrack.rollout import _targets_at, build_batch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64 = torch.float64
N, STEPS = 130, 40
SEEDS = np.arange(N) + 5
MOTION = [_abi.MOTIONS[i % 5] for i in range(N)]
MASS = np.linspace(0.8, 1.3, N)
CFG = quadtrack.env.config.as_env_config({"target": {"motion_type": "linear"}})
ENV = CFG.to_params()
NETS = {"n4": 1, "n0": 2, "n5": 4}  # [7] relu (NT 1), [64, 64] relu (NT 2), [128, 128] tanh (NT 4)

_POLICIES = {}


def policy_of(name) -> quadtrack.BatchedDeepPolicy:
    if name not in _POLICIES:
        net = M.fixture_net(name)
        _POLICIES[name] = quadtrack.BatchedDeepPolicy.from_state_dict(net.sd, net.sizes, net.activation, net.bounds,
                                                                      device=DEV)
    return _POLICIES[name]


def _dense(ctl):
    """The controller with every gain entry nonzero: the dense (unstructured) form."""
    g = torch.Generator().manual_seed(7)
    ctl.K = (ctl.K + 1e-3 * (torch.rand(ctl.K.shape, generator=g, dtype=F64) + 0.5).to(ctl.K.device)).contiguous()
    ctl.k_structured = core.gains_structured(ctl.K, ctl.k_cols)
    assert not ctl.k_structured
    return ctl


LQI = {"dt": 0.01, "use_lqi": True, "q_int": [1e-3, 1e-3, 1e-2]}
QPOS = np.stack([np.linspace(1e-4, 4e-4, N), np.linspace(2e-4, 1e-4, N), np.linspace(8.0, 24.0, N)], axis=1)
TEACHERS = {
    # k_cols 6: structured shared, dense shared, structured per episode (own DARE and hover thrust), heuristic
    "riccati": lambda: BatchedRiccatiLQR({"dt": 0.01}, device=DEV),
    "riccati_dense": lambda: _dense(BatchedRiccatiLQR({"dt": 0.01}, device=DEV)),
    "riccati_pe": lambda: BatchedRiccatiLQR({"dt": 0.01}, device=DEV, q_pos=QPOS, mass=MASS),
    "lqr": lambda: BatchedLQR({}, device=DEV),
    # k_cols 9: structured shared, dense per episode, and an integral that saturates at its limit
    "lqi": lambda: BatchedRiccatiLQR(LQI, device=DEV),
    "lqi_dense_pe": lambda: _dense(BatchedRiccatiLQR(LQI, device=DEV, q_pos=QPOS, mass=MASS)),
    "lqi_sat": lambda: BatchedRiccatiLQR(dict(LQI, integral_limit=0.004, integral_zero_threshold=0.0), device=DEV),
    # k_cols 3: the default PID (no integral gain) and one with an integral term; both start without a last time
    "pid": lambda: BatchedPID({}, device=DEV),
    "pid_ki": lambda: BatchedPID({"ki_pos": [0.05, 0.05, 0.5], "integral_limit": 0.05}, device=DEV),
    "pid_pe": lambda: BatchedPID({}, device=DEV, mass=MASS),
}
_TEACHERS = {}


def teacher_of(name):
    if name not in _TEACHERS:
        _TEACHERS[name] = TEACHERS[name]()
    return _TEACHERS[name]


def batch_of(sup, n=N):
    return build_batch(sup, CFG, n, seeds=SEEDS[:n], motion=MOTION[:n], plant_mass=MASS[:n], group_motion=False)


def identity_steps(n, S=STEPS):
    return np.repeat(np.arange(S, dtype=np.int32)[:, None], n, axis=1)


def fly(net, sup, batch, chunks=(STEPS,), steps=None, poke=None) -> SupervisedResult:
    """run_policy_supervised's launches on a given batch, everything recorded."""
    pol, n, total = policy_of(net), batch.n, sum(chunks)
    st = core.RolloutState.empty(n, batch.device)
    core.reset(ENV, batch, st)
    if poke is not None:
        poke(st)
    x0 = st.x.clone()
    steps = identity_steps(n, total) if steps is None else steps
    sd = torch.as_tensor(np.ascontiguousarray(steps), device=batch.device)
    nan = float("nan")
    sample = torch.full((sd.shape[0], _abi.SUP_ROWS, n), nan, dtype=torch.float32, device=batch.device)
    loss = torch.zeros(n, dtype=F64, device=batch.device)
    rec = torch.full((total, 16, n), nan, dtype=F64, device=batch.device)
    trec = torch.full((total, 4, n), nan, dtype=F64, device=batch.device)
    crit, done = core.criteria(), 0
    for k in chunks:
        pol.rollout_supervised(ENV, sup.ctrl, crit, batch, st, k, loss, sd, sample, rec[done:done + k],
                               trec[done:done + k])
        done += k
    res = SupervisedResult(metrics=core.episode_metrics(crit, st), state=st, batch=batch, criteria=crit, record=rec,
                           env=ENV, ctrl=sup.ctrl, policy=pol, loss=loss, sample=sample, steps_sampled=sd,
                           teacher_record=trec, supervisor=sup)
    res.x0 = x0
    torch.cuda.synchronize()
    return res


_RUNS = {}


def run_of(net, teacher) -> SupervisedResult:
    """The shared full run of (net, teacher): one launch, a sample slot at every step."""
    if (net, teacher) not in _RUNS:
        sup = teacher_of(teacher)
        _RUNS[net, teacher] = fly(net, sup, batch_of(sup))
    return _RUNS[net, teacher]


_FLIGHTS = {}


def flight_of(net):
    if net not in _FLIGHTS:
        _FLIGHTS[net] = run_policy_loop(policy_of(net), CFG, n=N, seeds=SEEDS, motion=MOTION, plant_mass=MASS,
                                        max_steps=STEPS, record=True)
        torch.cuda.synchronize()
    return _FLIGHTS[net]


def observations(res, total=STEPS):
    """Per step the observation the step acted on, rebuilt from the record and qt_target_state:
    state [total, 12, n], target [total, 9, n], time [total]."""
    times = np.concatenate([[0.0], np.cumsum(np.full(total, ENV.dt))])  # t_0 .. t_S, sequential t += dt
    tg = _targets_at(ENV, res.batch, torch.as_tensor(times[:-1], dtype=F64, device=res.batch.device))
    return torch.cat([res.x0[None], res.record[:-1, :12]]), tg, times[:-1]


ALL_TEACHERS = list(TEACHERS)
# every teacher on the NT 2 kernel, and the three k_cols on the other two
PAIRS = [("n0", t) for t in ALL_TEACHERS] + [(n, t) for n in ("n4", "n5") for t in ("riccati", "lqi_sat", "pid_ki")]
PAIR_IDS = [f"{n}-{t}" for n, t in PAIRS]


# ------------------------------------------------------------------ 1. the flight is untouched

@pytest.mark.parametrize("net,teacher", PAIRS, ids=PAIR_IDS)
def test_flight_is_the_policy_rollouts(net, teacher):
    res, ref = run_of(net, teacher), flight_of(net)
    assert int(res.state.acc[_abi.ACC_STEPS].min()) == STEPS
    for k in ("x", "target", "t", "acc"):
        np.testing.assert_array_equal(getattr(res.state, k).cpu().numpy(), getattr(ref.state, k).cpu().numpy(), k)
    np.testing.assert_array_equal(res.metrics.cpu().numpy(), ref.metrics.cpu().numpy())
    np.testing.assert_array_equal(res.record.cpu().numpy(), ref.record.cpu().numpy())


def test_public_entry_point_is_the_same_run():
    """run_policy_supervised builds the batch, the sample steps and the buffers of the shared run itself."""
    sup = teacher_of("lqi")
    res = run_policy_supervised(policy_of("n0"), sup, CFG, n=N, seeds=SEEDS, motion=MOTION, plant_mass=MASS,
                                max_steps=STEPS, record=True, samples_per_episode=STEPS, teacher_record=True)
    ref = run_of("n0", "lqi")
    assert np.array_equal(res.steps_sampled.cpu().numpy(), identity_steps(N))  # S = H: one step per stratum
    for a, b in ((res.sample, ref.sample), (res.loss, ref.loss), (res.teacher_record, ref.teacher_record),
                 (res.record, ref.record), (res.state.integ, ref.state.integ), (res.metrics, ref.metrics)):
        np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert res.features.shape == (STEPS, N, 18) and res.targets.shape == res.commands.shape == (STEPS, N, 4)
    assert bool(res.valid.all()) and res.dataset()[0].shape == (STEPS * N, 18)
    named = run_policy_supervised(policy_of("n0"), "riccati_lqr", CFG, n=N, seeds=SEEDS, motion=MOTION,
                                  plant_mass=MASS, max_steps=STEPS, samples_per_episode=0,
                                  supervisor_config={"dt": 0.01})
    np.testing.assert_array_equal(named.loss.cpu().numpy(), run_of("n0", "riccati").loss.cpu().numpy())
    assert named.sample.shape == (0, 26, N) and named.teacher_record is None
    with pytest.raises(ValueError, match="feed-forward"):
        run_policy_supervised(policy_of("n0"), BatchedRiccatiLQR({"dt": 0.01, "feedforward_enabled": True},
                                                                 device=DEV), CFG, n=4, max_steps=4)


# ------------------------------------------------------------------ 2. the labels are the per-step API's

@pytest.mark.parametrize("net,teacher", PAIRS, ids=PAIR_IDS)
def test_teacher_labels_are_the_per_step_apis(net, teacher):
    res, sup = run_of(net, teacher), teacher_of(teacher)
    x, tg, times = observations(res)
    sup.reset(N)  # a fresh controller: integral zero, PID without a last observation time
    if sup.k_cols == 3:
        assert bool(torch.isnan(sup.integral_state[3]).all())
    for s in range(STEPS):
        obs = {"quadcopter": {"position": x[s, 0:3].T, "velocity": x[s, 3:6].T},
               "target": {"position": tg[s, 0:3].T, "velocity": tg[s, 3:6].T},
               "time": torch.full((N,), times[s], dtype=F64, device=DEV)}
        want = sup.compute_action(obs).T.clone()
        np.testing.assert_array_equal(res.teacher_record[s].cpu().numpy(), want.cpu().numpy(), f"step {s}")
    rows = sup._integ_rows()
    if rows:
        np.testing.assert_array_equal(res.state.integ[:rows].cpu().numpy(), sup.integral_state[:rows].cpu().numpy())
    else:
        assert not res.state.integ.any()  # k_cols 6: the reset's zeros, not touched
    if teacher == "lqi_sat":  # the integral reached its limit and stays clamped there
        assert bool((res.state.integ[:3].abs() == 0.004).any())
    if teacher == "pid_ki":
        assert bool((res.state.integ[:3] != 0).any())
    if sup.k_cols == 3:  # the last observation time is the time of the last stepped observation
        assert bool((res.state.integ[3] == times[-1]).all())


# ------------------------------------------------------------------ 3. samples

@pytest.mark.parametrize("net,teacher", PAIRS, ids=PAIR_IDS)
def test_full_samples_are_the_record(net, teacher):
    res = run_of(net, teacher)
    x, tg, _ = observations(res)
    s = res.sample.cpu().numpy()
    np.testing.assert_array_equal(s[:, 18:22], res.teacher_record.cpu().numpy().astype(np.float32))
    np.testing.assert_array_equal(s[:, 22:26].astype(np.float64), res.record[:, 12:16].cpu().numpy())
    feats = torch.cat([tg[:, 0:3] - x[:, 0:3], tg[:, 3:6] - x[:, 3:6], x[:, 6:9], x[:, 9:12], tg[:, 0:3], tg[:, 3:6]],
                      dim=1).to(torch.float32)  # policy_features: FP64 differences, then f32
    np.testing.assert_array_equal(s[:, :18], feats.cpu().numpy())
    # the views of the result
    np.testing.assert_array_equal(res.features.cpu().numpy(), s[:, :18].transpose(0, 2, 1))
    np.testing.assert_array_equal(res.targets.cpu().numpy(), s[:, 18:22].transpose(0, 2, 1))
    np.testing.assert_array_equal(res.commands.cpu().numpy(), s[:, 22:26].transpose(0, 2, 1))


@pytest.mark.parametrize("net", list(NETS))
def test_stratified_samples_and_early_end(net):
    """Stratified slots hold the full record at their steps; an episode that leaves the position bound early
    keeps the NaN pre-fill in the slots beyond its last step, and valid is False there."""
    sup = teacher_of("lqi")
    S = 8
    steps = sample_steps(N, S, STEPS, seed=3)
    gone = [3, 64, 129]

    def poke(st):  # 2 cm inside the bound, 5 m/s outwards: out of bounds within a few steps
        st.x[0, gone] = ENV.max_position - 0.02
        st.x[3, gone] = 5.0

    full = fly(net, sup, batch_of(sup), poke=poke)
    part = fly(net, sup, batch_of(sup), steps=steps, poke=poke)
    flown = full.state.acc[_abi.ACC_STEPS].cpu().numpy().astype(int)
    assert (flown[gone] > 0).all() and (flown[gone] < 10).all() and (np.delete(flown, gone) == STEPS).all()
    assert (full.state.acc[_abi.ACC_TERM, gone] == 2).all()  # position_bounds
    fs, ps = full.sample.cpu().numpy(), part.sample.cpu().numpy()
    valid = part.valid.cpu().numpy()
    np.testing.assert_array_equal(valid, steps < flown[None, :])
    assert not valid[-1, gone].any() and valid[:, 0].all()
    for j in range(S):
        for e in range(N):
            if valid[j, e]:
                np.testing.assert_array_equal(ps[j, :, e], fs[steps[j, e], :, e])
            else:
                assert np.isnan(ps[j, :, e]).all()
    f, y = part.dataset()
    assert f.shape == (int(valid.sum()), 18) and y.shape == (int(valid.sum()), 4) and not torch.isnan(f).any()
    np.testing.assert_array_equal(part.loss.cpu().numpy(), full.loss.cpu().numpy())
    # unflown steps of the full record keep their pre-fill too
    assert np.isnan(fs[flown[3]:, :, 3]).all() and not np.isnan(fs[:flown[3], :, 3]).any()
    assert bool(torch.isnan(full.teacher_record[flown[3]:, :, 3]).all())


# ------------------------------------------------------------------ 4. loss

@pytest.mark.parametrize("net,teacher", PAIRS, ids=PAIR_IDS)
def test_loss_is_the_fp64_sum_of_the_record(net, teacher):
    res = run_of(net, teacher)
    u = res.record[:, 12:16].cpu().numpy()
    s32 = res.teacher_record.cpu().numpy().astype(np.float32).astype(np.float64)
    d = u - s32
    want = (d * d).sum(axis=(0, 1))
    got = res.loss.cpu().numpy()
    # non-negative terms, one rounding per product and per add: (4 steps + 4) half-ulps relative at most
    bound = (4 * STEPS + 4) * 2.0 ** -53
    rel = np.abs(got - want) / want
    print(net, teacher, "max relative loss error", rel.max(), "bound", bound)
    assert (want > 0).all() and (rel <= bound).all()
    np.testing.assert_array_equal(res.imitation_loss().cpu().numpy(), got / (4.0 * STEPS))


# ------------------------------------------------------------------ 5. chunking

@pytest.mark.parametrize("net,teacher", PAIRS, ids=PAIR_IDS)
def test_chunks_equal_one_launch(net, teacher):
    sup = teacher_of(teacher)
    steps = sample_steps(N, 8, STEPS, seed=11)  # strata of 5: the launches at steps 7 and 8 start between slots
    one = fly(net, sup, batch_of(sup), steps=steps)
    parts = fly(net, sup, batch_of(sup), chunks=(7, 1, 32), steps=steps)
    for k in ("x", "integ", "t", "acc", "target"):
        np.testing.assert_array_equal(getattr(parts.state, k).cpu().numpy(), getattr(one.state, k).cpu().numpy(), k)
    for k in ("loss", "sample", "record", "teacher_record"):
        np.testing.assert_array_equal(getattr(parts, k).cpu().numpy(), getattr(one, k).cpu().numpy(), k)
    assert not torch.isnan(one.sample).any()
    full = run_of(net, teacher)  # and the stratified slots are the full run's rows
    np.testing.assert_array_equal(one.loss.cpu().numpy(), full.loss.cpu().numpy())
    fs = full.sample.cpu().numpy()
    np.testing.assert_array_equal(one.sample.cpu().numpy(),
                                  np.stack([fs[steps[j], :, np.arange(N)].T for j in range(8)]))


# ------------------------------------------------------------------ 6. lane independence

@pytest.mark.parametrize("teacher", ["lqi_dense_pe", "riccati_pe", "pid_pe"])
@pytest.mark.parametrize("net", list(NETS))
def test_lane_independence(net, teacher):
    sup = teacher_of(teacher)
    full = run_of(net, teacher)
    perm = np.random.default_rng(0).permutation(N)
    for idx in (np.arange(1), np.arange(63), np.arange(64), np.arange(65), perm):
        sub = full.batch.select(torch.as_tensor(idx, device=DEV))
        got = fly(net, sup, sub)
        for k in ("x", "integ", "acc", "target"):
            np.testing.assert_array_equal(getattr(got.state, k).cpu().numpy(),
                                          getattr(full.state, k).cpu().numpy()[:, idx], k)
        np.testing.assert_array_equal(got.loss.cpu().numpy(), full.loss.cpu().numpy()[idx])
        for k in ("sample", "teacher_record", "record"):
            np.testing.assert_array_equal(getattr(got, k).cpu().numpy(), getattr(full, k).cpu().numpy()[:, :, idx], k)


# ------------------------------------------------------------------ 7. the reference fixture

FX = np.load(os.path.join(GOLDEN, "imitation.npz"))
META = json.loads(str(FX["meta_json"]))
ATOL, RTOL = 1e-5, 1e-8
FX_RUNS = [(n, s["name"], m) for n in META["nets"] for s in META["supervisors"] for m in META["motions"]]


@pytest.mark.parametrize("net,supervisor,motion", FX_RUNS, ids=["-".join(r) for r in FX_RUNS])
def test_reference_fixture(net, supervisor, motion):
    spec = next(s for s in META["supervisors"] if s["name"] == supervisor)
    key, seeds = f"{net}/{supervisor}/{motion}", FX[f"{net}/{motion}/seeds"]
    sup = batched_controller(spec["type"], spec["config"], device=DEV)
    res = run_policy_supervised(policy_of(net), sup, {"target": {"motion_type": motion}}, n=len(seeds), seeds=seeds,
                                max_steps=META["steps"], samples_per_episode=0, teacher_record=True)
    assert (res.metric("steps") == META["steps"]).all()
    got = res.teacher_record.cpu().numpy()[META["stored"]].transpose(2, 0, 1)  # [4, 39, 4]
    ref, gap = FX[f"{key}/cmd"], FX[f"{key}/cmd_gap"]
    tol = M.tol_of(gap[None], ref)
    err = np.abs(got - ref)
    loss, lref = res.imitation_loss().cpu().numpy(), FX[f"{key}/loss"]
    ltol = np.maximum(4.0 * FX[f"{key}/loss_gap"], ATOL + RTOL * np.abs(lref))
    lerr = np.abs(loss - lref)
    print(f"{key}: teacher command max err {err.max():.3e}, fraction of the bound {(err / tol).max():.4f}; "
          f"imitation loss {lref.max():.6g}, max err {lerr.max():.3e}, fraction of the bound {(lerr / ltol).max():.4f}")
    assert (err <= tol).all(), (err.max(axis=(0, 1)), gap.max(axis=0))
    assert (lerr <= ltol).all(), (loss, lref, ltol)


# ------------------------------------------------------------------ 8. the driver

def _trained(seed):
    torch.manual_seed(5)
    pol = quadtrack.DeepTrackingPolicy({"hidden_sizes": [32], "activation": "relu"}, device=DEV)
    out = quadtrack.train_imitation(pol, "riccati_lqr", {"dt": 0.01}, {"target": {"motion_type": "stationary"}},
                                    epochs=3, episodes_per_epoch=64, max_steps=100, seed=seed, keep_datasets=True)
    return pol, out


def test_train_imitation_driver():
    pol, a = _trained(0)
    _, b = _trained(0)
    for x, y in zip(a.datasets[0], b.datasets[0]):  # epoch 0's data set: a function of the seeds
        np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy())
    assert a.datasets[0][0].shape == (64 * 32, 18) and not torch.isnan(a.datasets[0][0]).any()
    np.testing.assert_array_equal(a.dataset_loss_after.numpy(), b.dataset_loss_after.numpy())
    before, after = a.dataset_loss_before.numpy(), a.dataset_loss_after.numpy()
    print("data-set loss before", before, "after", after, "whole-episode imitation loss", a.imitation_loss.numpy())
    assert before.shape == after.shape == (3,) and (after < before).all()
    assert np.isfinite(a.mean_reward.numpy()).all() and (a.mean_reward.numpy() < 0).all()
    assert ((a.mean_on_target_ratio.numpy() >= 0) & (a.mean_on_target_ratio.numpy() <= 1)).all()
    # the returned weights are the policy's, and what the next rollout flies
    for k, v in pol.network.state_dict().items():
        assert v.device.type == "cpu" and torch.equal(v, a.state_dict[k]), k
    cfg = {"target": {"motion_type": "stationary"}}
    flown = run_policy_loop(pol, cfg, n=8, seeds=np.arange(8), max_steps=20, record=True)
    fresh = quadtrack.BatchedDeepPolicy.from_state_dict(a.state_dict, [32], "relu", device=DEV)
    again = run_policy_loop(fresh, cfg, n=8, seeds=np.arange(8), max_steps=20, record=True)
    np.testing.assert_array_equal(flown.record.cpu().numpy(), again.record.cpu().numpy())
    torch.manual_seed(5)
    start = quadtrack.DeepTrackingPolicy({"hidden_sizes": [32], "activation": "relu"}, device=DEV)
    assert not torch.equal(start.network.output_layer.weight, pol.network.output_layer.weight)
