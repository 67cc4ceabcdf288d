"""Deep tracking policy on the GPU, every kernel variant: the twelve
activation x NT code paths of policy_forward (csrc/qt_policy.hpp) through both
entry points, on the architecture matrix of tests/policy_model.py, and the
documented f32 summation order against an exact host model of it.

Rule T1 (all nets): tests/test_gpu_policy.py's rule with its inputs from torch
alone: |device - torch f32| <= max(4 x gap, 1e-5 + 1e-8 |ref|), gap the
per-component maximum over the 512 rows of |torch f32 - torch float64|.

Rule T2 (relu and leaky_relu nets, whose logits the host model gives exactly):
|u_dev - u*| <= 2^-24 (5 |m*| + |u*|) (1 + 2^-10) + 2^-126 scale; derivation at
test_action_against_exact_model.
"""

import numpy as np
import pytest
import torch

import oracle as O
import policy_model as M
import quadtrack
from quadtrack.policy import run_policy_loop

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_POLICIES = {}


def device_policy(net: M.Net) -> quadtrack.BatchedDeepPolicy:
    if net.name not in _POLICIES:
        _POLICIES[net.name] = quadtrack.BatchedDeepPolicy.from_state_dict(net.sd, net.sizes, net.activation, net.bounds,
                                                                          device=DEV)
    return _POLICIES[net.name]


def obs_tensors(rows):
    """[k, 6, 3] fixture observations -> the observation dict of [k, 3] device tensors."""
    t = torch.as_tensor(np.ascontiguousarray(rows), dtype=torch.float64, device=DEV)
    q = {k: t[:, i] for i, k in enumerate(("position", "velocity", "attitude", "angular_velocity"))}
    return {"quadcopter": q, "target": {"position": t[:, 4], "velocity": t[:, 5]}}


def device_actions(net, rows=slice(None)):
    a = device_policy(net).compute_action(obs_tensors(M.FX["obs"][rows])).cpu().numpy()
    assert a.shape == (len(M.FX["obs"][rows]), 4) and np.isfinite(a).all()
    assert np.array_equal(a, a.astype(np.float32).astype(np.float64))  # the f32 result widened exactly
    return a


# ------------------------------------------------------------------ D1. rule T1

@pytest.mark.parametrize("name", M.MATRIX_IDS)
def test_action_against_float64(name):
    net = M.matrix_net(name)
    a = device_actions(net)
    ref, _, gap = M.reference(name)
    err = np.abs(a - ref)
    print(name, "max |device - torch f32|", err.max(axis=0), "torch f32-f64 gap", gap, "ratio",
          err.max(axis=0) / np.maximum(gap, 1e-300), "worst observation per component", err.argmax(axis=0))
    assert (err <= M.tol_of(gap[None, :], ref)).all(), (err.max(axis=0), gap)


# ------------------------------------------------------------------ D2. rule T2

def t2_ratio(net, rows):
    y = M.model_logits(net, M.features(rows))
    u, tol = M.t2_tolerance(net, y)
    ratio = np.abs(device_actions(net, rows) - u) / tol
    return y, ratio


@pytest.mark.parametrize("name", M.FIXTURE_EXACT_IDS + M.MATRIX_EXACT_IDS)
def test_action_against_exact_model(name):
    """The device's command against the host model's exact f32 logit y pushed through the output stage in
    float64: m* = sigmoid(y) scale, u* = m* + lo, scale = float32(hi - lo), lo = float32(lo).

    The device's logits are the model's bit for bit (same fmaf chains in the same order), so only the
    output stage s = 1 / (1 + expf(-y)), m = s scale, u = m + lo errs.  expf is within 1 ulp, 2^-23 relative
    on e, which reaches s with the factor e / (1 + e) <= 1.  The add 1 + e, the division (correctly
    rounded: the unit is built without relaxed math) and the multiplication by scale each add 2^-24
    relative, together 5 x 2^-24 |m*| to first order; the final add contributes 2^-24 |u|; the factor
    1 + 2^-10 covers the second-order terms; 2^-126 scale covers a sigmoid that is flushed or underflows
    for rows that saturate it.  The 1 ulp of expf is the figure of the HIP documentation's table of device
    math functions ("HIP math API", single-precision functions: expf, maximum ulp error 1)."""
    net = M.any_net(name)
    _, ratio = t2_ratio(net, slice(None))
    print(name, "max |u_dev - u*| / tolerance per component", ratio.max(axis=0), "worst observation", ratio.argmax(axis=0))
    assert (ratio <= 1.0).all(), (ratio.max(axis=0), ratio.argmax(axis=0))


@pytest.mark.parametrize("name", M.ORDER_PROBE_IDS)
def test_summation_order_is_the_documented_one(name):
    """The order probe: the same weights with every output bias -12 and bounds (0, 1), on fixture
    observations 60-315.  Every logit then lies in [-16, -8), where one ulp of it is 2^-20 = 9.5e-7
    relative in the command, while rule T2 (scale 1, lo 0) allows about 6 x 2^-24 = 3.6e-7: a device that
    sums in another order, or rounds one step differently, fails on the rows that
    test_policy_model_cpu.py::test_order_probe_has_power counts (at least 10 % of them for plain index
    order).  A failure here after a kernel change means the summation order changed: update
    csrc/qt_policy.hpp's statement and tests/policy_model.py's model together."""
    net = M.order_probe_net(name)
    y, ratio = t2_ratio(net, M.ORDER_ROWS)
    assert ((y >= -16.0) & (y < -8.0)).all(), (y.min(), y.max())
    print(name, "order probe: max |u_dev - u*| / tolerance", ratio.max(), "logits", y.min(), y.max())
    assert (ratio <= 1.0).all(), (ratio.max(), np.unravel_index(ratio.argmax(), ratio.shape))


# ------------------------------------------------------------------ D3. the rollout kernel

N, STEPS = 70, 12
MOTION = [quadtrack._abi.MOTIONS[i % 5] for i in range(N)]
MASS = np.linspace(0.8, 1.3, N)
ENV_CFG = {"target": {"motion_type": "linear"}}
# chosen with the host model and oracle.env_step on the CPU: under the wide-bounds net the env clips commands
# of episodes 33, 43 and 53 (6, 12 and 3 steps) and of no other
SEEDS = np.arange(N) + 100
WIDE = "relu-96x96-wide"


def rollout_net(name):
    return M.wide_bounds_net() if name == WIDE else M.matrix_net(name)


ROLLOUT_IDS = M.MATRIX_IDS + [WIDE]
_RECORDED = {}


def recorded_run(name):
    """The recorded run of one net, launched once and shared (read-only) by the tests below."""
    if name not in _RECORDED:
        pol = device_policy(rollout_net(name))
        res = run_policy_loop(pol, ENV_CFG, n=N, seeds=SEEDS, motion=MOTION, plant_mass=MASS, max_steps=STEPS,
                              record=True)
        torch.cuda.synchronize()
        res.net = name
        _RECORDED[name] = res
    return _RECORDED[name]


@pytest.mark.parametrize("name", ROLLOUT_IDS)
def test_rollout_commands_are_the_action_kernel_bitwise(name):
    """Every recorded command is, bit for bit, compute_action on that step's observation (rebuilt by
    RolloutResult.trajectories, which re-runs the policy rollout)."""
    recorded = recorded_run(name)
    pol = device_policy(rollout_net(recorded.net))
    tr = recorded.trajectories()
    assert int(tr["steps"].min()) == STEPS
    assert torch.equal(tr["next_state"], recorded.record[:, :12])
    assert torch.equal(tr["action"], recorded.record[:, 12:])
    for s in range(STEPS):
        x, tg = tr["obs_state"][s], tr["obs_target"][s]  # [12, n], [9, n]
        obs = {"quadcopter": {"position": x[0:3].T, "velocity": x[3:6].T, "attitude": x[6:9].T,
                              "angular_velocity": x[9:12].T},
               "target": {"position": tg[0:3].T, "velocity": tg[3:6].T}}
        assert torch.equal(pol.compute_action(obs), recorded.record[s, 12:].T), s


@pytest.mark.parametrize("name", ROLLOUT_IDS)
def test_rollout_in_chunks_is_one_launch_bitwise(name):
    recorded = recorded_run(name)
    res = run_policy_loop(device_policy(rollout_net(recorded.net)), ENV_CFG, n=N, seeds=SEEDS, motion=MOTION,
                          plant_mass=MASS, max_steps=STEPS, chunk=5, record=True)
    assert not torch.isnan(recorded.record).any()
    assert torch.equal(res.record, recorded.record)
    assert torch.equal(res.metrics, recorded.metrics)
    for k in ("x", "t", "acc", "target"):
        assert torch.equal(getattr(res.state, k), getattr(recorded.state, k)), k


def test_wide_bounds_rollout_steps_and_violations():
    """Output bounds wider than the env's action limits: the recorded command is the policy's, unclipped; the
    env clips it (every recorded step against oracle.env_step from the recorded previous state and command),
    and action_violations counts exactly the steps whose command it had to clip."""
    recorded = recorded_run(WIDE)
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
            np.testing.assert_allclose(rec[s, :12, e], xn, rtol=M.RTOL, atol=M.ATOL, err_msg=f"episode {e} step {s}")
            x = rec[s, :12, e]
    u = rec[:, 12:]  # [steps, 4, n]
    clipped = (u[:, 0] < env.min_thrust) | (u[:, 0] > env.max_thrust) | (np.abs(u[:, 1:]) > env.max_angular_rate).any(axis=1)
    want = clipped.sum(axis=0)
    got = recorded.metric("action_violations").cpu().numpy()
    print("max |device step - oracle step|", worst, "clipped steps per episode", want.tolist())
    assert np.array_equal(got, want), (got, want)
    assert (want > 0).any() and (want == 0).any()
    assert u[:, 0].max() > env.max_thrust or u[:, 0].min() < env.min_thrust or np.abs(u[:, 1:]).max() > env.max_angular_rate
