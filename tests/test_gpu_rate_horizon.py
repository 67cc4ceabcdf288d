"""The yaw-at-rest loop's no-vote steps without the rate-command clips and
without the post-step on-target test (csrc/qt_kernels.hpp: rate_distance,
run_yaw0's kRate and EQR) against the arithmetic they replace.

QT_RATE_HORIZON=0 makes the rate term of the safe horizon report no distance:
every step is then voted and clipped, today's arithmetic step for step, and
the default run must equal it bit for bit — metrics, final state, target
observation, accumulators.  The one-lane kernels are the ones changed, so the
small batches run with QT_PAIR=0 (a small batch otherwise takes the pair
flavour, which has no rate term and must not change: the 8,192-episode cases
run it).  On-target counts are compared with the oracle's exactly.
Reference loop: env/quadcopter_env.py:152-232, eval.py:119-165."""

import numpy as np
import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu

# tests/test_rate_horizon_cpu.py's set-up whose rate clips act (6 % of the steps there)
SATURATING_ENV = {"target": {"motion_type": "linear"}}
SATURATING_CTL = {"dt": 0.01, "max_rate": 0.07}


@pytest.fixture(scope="module")
def qt():
    import quadtrack

    quadtrack._abi.require_gpu()
    return quadtrack


def _both(monkeypatch, fn):
    out = {}
    for on in ("1", "0"):
        monkeypatch.setenv("QT_RATE_HORIZON", on)
        out[on] = fn()
    monkeypatch.delenv("QT_RATE_HORIZON")
    return out["1"], out["0"]


def _same_state(sa, sb):
    for f in ("x", "t", "acc", "target", "integ"):
        assert torch.equal(getattr(sa, f), getattr(sb, f)), f


def _same(a, b):
    assert torch.equal(a.metrics, b.metrics)
    _same_state(a.state, b.state)


def _controller(gains, n):
    from quadtrack import workloads
    from quadtrack.controllers import BatchedRiccatiLQR

    if gains == "shared":
        return BatchedRiccatiLQR({"dt": 0.01})
    # per-episode structured gains, as config 4's tuner candidates
    dev = torch.device("cuda", torch.cuda.current_device())
    qp, qv, rc = workloads.tuner_candidate_tensors(0, n, dev)
    return BatchedRiccatiLQR({"dt": 0.01}, device=dev, q_pos=qp, q_vel=qv, r_controls=rc)


def _oracle(env_cfg, ctl_cfg, seeds, steps, crit=None, x0=None):
    env = O.env_params(env_cfg)
    pat, off = O.draws(env.motion, seeds)
    if x0 is None:
        x0 = np.array([O.initial_state(env, env.motion, pat[i], off[i]) for i in range(len(seeds))])
    c, K, kc, _, _ = O.controller(dict(ctl_cfg))
    met, xf, _, _ = O.rollout(env, c, crit or O.criteria(), None, pat, None, None, K, kc, False, x0, max_steps=steps)
    return met, xf, x0


def _on_post(met):
    """The env's on-target count of met[episodes, rows]: ratio x steps, an integer."""
    i, j = O.MET_FIELDS.index("env_on_target_ratio"), O.MET_FIELDS.index("steps")
    return np.rint(met[:, i] * met[:, j]).astype(np.int64), met[:, j].astype(np.int64)


BITWISE = [(m, g, n) for m in ("linear", "stationary") for g in ("shared", "per_episode") for n in (64, 130, 8192)]
BITWISE += [("linear", "shared", 40000), ("stationary", "shared", 40000)]


@pytest.mark.parametrize("motion,gains,n", BITWISE)
def test_rate_horizon_bitwise(qt, monkeypatch, motion, gains, n):
    """64 and 130 (a partial wave) through the one-lane kernel, 8,192 through
    the pair flavour, 40,000 (beyond one wave per SIMD in pairs, shared gains)
    through the one-lane kernel as the dispatch picks it."""
    from quadtrack.rollout import run_closed_loop

    if n < 8192:
        monkeypatch.setenv("QT_PAIR", "0")
    ctl = _controller(gains, n)
    cfg = {"target": {"motion_type": motion}}
    a, b = _both(monkeypatch, lambda: run_closed_loop(ctl, cfg, n=n, seeds=np.arange(n) + 3, max_steps=400))
    _same(a, b)


def test_rate_clips_that_act(qt, monkeypatch):
    """A batch whose rate commands do reach their clip: bitwise against the
    knob-off run, and against the oracle at the suite's 1e-5 / 1e-8."""
    from quadtrack.controllers import BatchedRiccatiLQR
    from quadtrack.rollout import run_closed_loop

    monkeypatch.setenv("QT_PAIR", "0")
    n, steps = 128, 600
    ctl = BatchedRiccatiLQR(dict(SATURATING_CTL))
    a, b = _both(monkeypatch, lambda: run_closed_loop(ctl, SATURATING_ENV, n=n, seeds=np.arange(n), max_steps=steps))
    _same(a, b)
    met, xf, _ = _oracle(SATURATING_ENV, SATURATING_CTL, np.arange(n), steps)
    np.testing.assert_allclose(a.metrics.cpu().numpy().T, met, rtol=1e-8, atol=1e-5)
    np.testing.assert_allclose(a.state.x.cpu().numpy().T, xf, rtol=1e-8, atol=1e-5)


@pytest.mark.parametrize("radius", [0.5, 0.3])
def test_on_target_counts_exact(qt, monkeypatch, radius):
    """The env's on-target count against the oracle's, exactly: with the
    criteria's radius equal to the env's 0.5 (the EQR variant rebuilds the count
    from the pre-step flags) and with SuccessCriteria(target_radius=0.3)
    against the env's 0.5 (the per-step test)."""
    from quadtrack.controllers import BatchedRiccatiLQR
    from quadtrack.rollout import run_closed_loop
    from quadtrack.utils.metrics import SuccessCriteria

    monkeypatch.setenv("QT_PAIR", "0")
    n, steps = 128, 600
    cfg = {"target": {"motion_type": "linear"}}
    res = run_closed_loop(BatchedRiccatiLQR({"dt": 0.01}), cfg, n=n, seeds=np.arange(n), max_steps=steps,
                          criteria=SuccessCriteria(target_radius=radius))
    met, _, _ = _oracle(cfg, {"dt": 0.01}, np.arange(n), steps, crit=O.criteria(target_radius=radius))
    got, got_steps = _on_post(res.metrics.cpu().numpy().T)
    ref, ref_steps = _on_post(met)
    assert np.array_equal(got_steps, ref_steps)
    assert np.array_equal(got, ref)
    assert 0 < ref.min() < ref.max() <= steps and len(set(ref.tolist())) > 10  # not vacuous


def test_equal_radii_bitwise_against_the_per_step_test(qt, monkeypatch):
    """The equal-radii run against the same run forced through the per-step
    on-target test: the env's radius one ulp above the criteria's 0.5 (only the
    post-step test reads it, and no error lands on that one number), the
    oracle given the same."""
    from quadtrack.controllers import BatchedRiccatiLQR
    from quadtrack.rollout import run_closed_loop

    monkeypatch.setenv("QT_PAIR", "0")
    n, steps = 130, 600
    up = float(np.nextafter(0.5, 1.0))
    for motion in ("linear", "stationary"):
        cfg = {"target": {"motion_type": motion}}
        cfg_up = {"target": {"motion_type": motion}, "success_criteria": {"target_radius": up}}
        ctl = BatchedRiccatiLQR({"dt": 0.01})
        a = run_closed_loop(ctl, cfg, n=n, seeds=np.arange(n), max_steps=steps)
        b = run_closed_loop(ctl, cfg_up, n=n, seeds=np.arange(n), max_steps=steps)
        assert b.env.target_radius == up and a.env.target_radius == 0.5
        _same(a, b)
        met, _, _ = _oracle(cfg_up, {"dt": 0.01}, np.arange(n), steps)
        assert np.array_equal(_on_post(b.metrics.cpu().numpy().T)[0], _on_post(met)[0])


def _chunked(qt, env_cfg, n, chunks):
    from quadtrack import core
    from quadtrack.controllers import BatchedRiccatiLQR
    from quadtrack.env.config import EnvConfig
    from quadtrack.rollout import build_batch

    ctl = BatchedRiccatiLQR({"dt": 0.01})
    env = EnvConfig.from_dict(env_cfg).to_params()
    crit = core.criteria()
    batch = build_batch(ctl, env_cfg, n, seeds=np.arange(n))
    st = core.RolloutState.empty(n, batch.device)
    core.reset(env, batch, st)
    for k in chunks:
        core.rollout(env, ctl.ctrl, crit, batch, st, k, None)
    return core.episode_metrics(crit, st), st


# acc rows that hold counts and codes (include/quadtrack.h QT_ACC_*): on_pre,
# on_post, os_count, os_streak, prev_on, steps, violations, term
COUNT_ROWS = [3, 4, 6, 9, 10, 11, 12, 13]


def test_chunked_launches(qt, monkeypatch):
    """Launches of 137 steps up to 600 (and one of no steps): the on-target
    count rebuilt per run carries across launch boundaries.  Bitwise, launch
    for launch, equal to the knob-off run and to the run forced through the
    per-step on-target test; on-target counts exactly the oracle's.

    Against ONE launch of 600 steps every count is exact, but the floating
    rows are not bitwise, in this loop as in the one before it: a launch
    starts from the directly evaluated sin / cos of roll and pitch where a
    running loop carries them (attitude_trig_resid: a few ulp of drift per
    step; tests/test_gpu_pair.py says the same of its chunked case).  Measured
    here, and the same figures with the parent commit's library: metrics
    differ by at most 4.9e-11 absolute, the state by 4.7e-14.  The carried
    trig is within a few ulp x 137 steps ~ 1e-13 of the evaluated one and the
    sums run over 600 steps, so the rows are held to the 1e-9 this suite uses
    where a restart is compared with a carried run
    (test_gpu_pair.py::test_pair_flavour_deferred_waves)."""
    monkeypatch.setenv("QT_PAIR", "0")
    n = 130
    cfg = {"target": {"motion_type": "linear"}}
    cfg_up = {"target": {"motion_type": "linear"}, "success_criteria": {"target_radius": float(np.nextafter(0.5, 1.0))}}
    chunks = [137, 137, 0, 137, 137, 52]
    assert sum(chunks) == 600
    (ma, sa), (mb, sb) = _both(monkeypatch, lambda: _chunked(qt, cfg, n, chunks))
    assert torch.equal(ma, mb)
    _same_state(sa, sb)
    mu, su = _chunked(qt, cfg_up, n, chunks)  # the per-step on-target test
    assert torch.equal(ma, mu)
    _same_state(sa, su)
    met, _, _ = _oracle(cfg, {"dt": 0.01}, np.arange(n), 600)
    assert np.array_equal(_on_post(ma.cpu().numpy().T)[0], _on_post(met)[0])
    m1, s1 = _chunked(qt, cfg, n, [600])
    print("chunked against one launch: max |d metrics| %.3e, max |d x| %.3e, bitwise %s" % (
        float((ma - m1).abs().max()), float((sa.x - s1.x).abs().max()), torch.equal(ma, m1) and torch.equal(sa.x, s1.x)))
    assert torch.equal(sa.acc[COUNT_ROWS], s1.acc[COUNT_ROWS])
    assert torch.equal(sa.t, s1.t)
    np.testing.assert_allclose(ma.cpu().numpy(), m1.cpu().numpy(), rtol=1e-9, atol=1e-9)
    for f in ("x", "acc", "target"):
        np.testing.assert_allclose(getattr(sa, f).cpu().numpy(), getattr(s1, f).cpu().numpy(), rtol=1e-9, atol=1e-9)


def test_early_termination(qt, monkeypatch):
    """A wave where 16 of 64 lanes leave max_position within 100 steps (started
    near 1000 m, flying outward) and the loop restarts for the others: step
    counts, termination codes and on-target counts exactly the oracle's,
    every row bitwise the knob-off run's."""
    from quadtrack import core
    from quadtrack.controllers import BatchedRiccatiLQR
    from quadtrack.env.config import EnvConfig
    from quadtrack.rollout import build_batch

    monkeypatch.setenv("QT_PAIR", "0")
    n, steps = 64, 600
    cfg = {"target": {"motion_type": "linear"}}
    ctl = BatchedRiccatiLQR({"dt": 0.01})
    env = EnvConfig.from_dict(cfg).to_params()
    crit = core.criteria()
    far = np.arange(0, n, 4)

    def run():
        batch = build_batch(ctl, cfg, n, seeds=np.arange(n))
        st = core.RolloutState.empty(n, batch.device)
        core.reset(env, batch, st)
        for i, slot in enumerate(far):
            st.x[0, slot] = 999.9 - 0.25 * i
            st.x[3, slot] = 20.0
        core.rollout(env, ctl.ctrl, crit, batch, st, steps, None)
        return core.episode_metrics(crit, st), st

    (ma, sa), (mb, sb) = _both(monkeypatch, run)
    assert torch.equal(ma, mb)
    _same_state(sa, sb)
    _, _, x0 = _oracle(cfg, {"dt": 0.01}, np.arange(n), 0)
    for i, slot in enumerate(far):
        x0[slot, 0] = 999.9 - 0.25 * i
        x0[slot, 3] = 20.0
    met, xf, _ = _oracle(cfg, {"dt": 0.01}, np.arange(n), steps, x0=x0)
    got = ma.cpu().numpy().T
    code = O.MET_FIELDS.index("termination_code")
    ref_post, ref_steps = _on_post(met)
    assert np.all(ref_steps[far] < 100) and np.all(np.delete(ref_steps, far) == steps)
    assert len(set(ref_steps[far].tolist())) > 4  # the lanes leave at different steps
    got_post, got_steps = _on_post(got)
    assert np.array_equal(got_steps, ref_steps)
    assert np.array_equal(got[:, code], met[:, code])
    assert np.array_equal(got_post, ref_post)
    np.testing.assert_allclose(sa.x.cpu().numpy().T, xf, rtol=1e-8, atol=1e-5)


@pytest.mark.parametrize("counts", [(64, 64, 64, 64, 64), (90, 50, 64, 70, 33)],
                         ids=["64_each", "ragged_with_riders"])
def test_grouped_batch_bitwise(qt, monkeypatch, counts):
    """All five motions in one grouped launch (the ragged counts leave free
    lanes that stationary riders fill): bitwise equal knob on / off."""
    from quadtrack.controllers import BatchedRiccatiLQR
    from quadtrack.rollout import run_closed_loop

    motion = np.concatenate([np.full(c, m, dtype=np.int8) for m, c in enumerate(counts)])
    motion = motion[np.random.default_rng(5).permutation(len(motion))]
    n = len(motion)
    ctl = BatchedRiccatiLQR({"dt": 0.01})
    a, b = _both(monkeypatch, lambda: run_closed_loop(ctl, {}, n=n, seeds=np.arange(n), motion=motion, max_steps=400))
    _same(a, b)


def test_knob_bad_value_is_ignored_and_reported_once(qt, monkeypatch, capfd):
    """QT_RATE_HORIZON takes 0 or 1; anything else leaves the term on and is
    reported once on stderr."""
    from quadtrack.controllers import BatchedRiccatiLQR
    from quadtrack.rollout import run_closed_loop

    monkeypatch.setenv("QT_PAIR", "0")
    ctl = BatchedRiccatiLQR({"dt": 0.01})
    cfg = {"target": {"motion_type": "linear"}}
    monkeypatch.delenv("QT_RATE_HORIZON", raising=False)
    a = run_closed_loop(ctl, cfg, n=64, seeds=np.arange(64), max_steps=300)
    capfd.readouterr()
    monkeypatch.setenv("QT_RATE_HORIZON", "off")
    b = run_closed_loop(ctl, cfg, n=64, seeds=np.arange(64), max_steps=300)
    c = run_closed_loop(ctl, cfg, n=64, seeds=np.arange(64), max_steps=300)
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    _same(a, b)
    _same(a, c)
    assert err.count("ignoring QT_RATE_HORIZON=off") == 1
