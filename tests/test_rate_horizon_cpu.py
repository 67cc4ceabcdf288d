"""The rate-command term of the yaw-at-rest loop's safe horizon
(csrc/qt_kernels.hpp rate_distance, csrc/qt_device.hpp make_horizon) checked
against the steps the oracle actually takes.  CPU only.

Inside a safe horizon the loops with 6-column gains and no feed-forward run
their steps without the two rate-command clips.  That is sound when the raw
roll / pitch rate commands raw_r = sum_j K_rj s_j (s: the six controller
errors p_T - p, v_T - v) stay strictly inside +-max_rate for the horizon's
steps.  The bound: per step and component a position error moves by at most
dp + (the target's reach), a velocity error by at most
(1 - cv) vmax + tmax / m sum|wv| + |gv| + (the target's velocity reach), so

    h_r = (max_rate (1 - 1e-9) - sum_j |K_rj| |s_j|) / sum_j |K_rj| delta_j

steps ahead of an observation the command cannot have reached the clip.  The
constants are restated here from the RK4 recurrences (as test_horizon_cpu.py
restates its neighbours), and over recorded oracle episodes every step k and
every j < min(h_r(k), 62) must find the raw command of step k + j inside the
clip.

Target reach per step (tstep bounds t' - t): stationary 0 / 0; linear
|v_T,j| tstep / 0 (the velocity is constant).  The kernels take the term for
these two only; the periodic targets keep their clips.  For the circular and
sinusoidal cases the bound is checked here with the reach their patterns
allow, amplitude omega tstep for a position and amplitude omega^2 tstep for
a velocity, per component (the mean value theorem on a sin(omega t + phi)).
"""

import numpy as np
import pytest

import oracle as O

K_MAX_HORIZON = 62
MARGIN = 1e-9
SLACK = 1.0 + 1e-9


def rk4_linear(lam, h, y, f):
    """Stage values of y' = f_i - lam y over one RK4 step (qt_device.hpp rk4_linear)."""
    k1 = f[0] - lam * y
    y2 = y + 0.5 * h * k1
    k2 = f[1] - lam * y2
    y3 = y + 0.5 * h * k2
    k3 = f[2] - lam * y3
    y4 = y + h * k3
    k4 = f[3] - lam * y4
    return (y2, y3, y4, y + h / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4), h / 6.0 * (y + 2.0 * y2 + 2.0 * y3 + y4))


def step_bounds(e, c, mass):
    """Per step and component: the position bound dp (yaw0_horizon's), the
    velocity bound dvc (rate_distance's) and the time bound tstep."""
    h, inv_m = e.dt, 1.0 / mass
    delta = e.drag_linear * inv_m
    o = rk4_linear(delta, h, 1.0, [0.0] * 4)
    cv, pv = o[3], o[4]
    wv, pa = [], []
    for i in range(4):
        f = [0.0] * 4
        f[i] = 1.0
        oi = rk4_linear(delta, h, 0.0, f)
        wv.append(oi[3])
        if i < 3:
            pa.append(oi[4])
    g = -mass * e.gravity * inv_m
    gv, gp = g * sum(wv), g * sum(pa)
    tmi = max(abs(c.min_thrust), abs(c.max_thrust)) * inv_m
    vmax = e.max_velocity * (1.0 - 1e-12)
    pabs = e.max_position * 1e-15
    dp = (abs(pv) * vmax + tmi * sum(abs(p) for p in pa) + abs(gp)) * SLACK + pabs
    dvc = ((1.0 - cv) * vmax + tmi * sum(abs(w) for w in wv) + abs(gv)) * SLACK + e.max_velocity * 1e-14
    tstep = (e.dt + (abs(e.max_episode_time) + e.dt) * 4.5e-16) * SLACK
    assert 0.0 <= cv <= 1.0
    return dp, dvc, tstep, pabs


def target_reach(e, motion, tv, tstep):
    """Per-component reach of the target's position and velocity in one step
    (tv: the observation's target velocity [steps, 3])."""
    z = np.zeros_like(tv)
    if motion == "stationary":
        return z, z
    if motion == "linear":
        return np.abs(tv) * tstep, z
    if motion == "circular":
        om = e.speed / e.radius
        amp, oms = np.array([e.radius, e.radius, 0.0]), np.array([om, om, 0.0])
    elif motion == "sinusoidal":
        amp = e.amplitude * np.array([1.0, 0.5, 0.25])
        oms = 2.0 * np.pi * e.frequency * np.array([1.0, 1.3, 0.7])
    else:
        raise ValueError(motion)
    return z + amp * oms * tstep * SLACK, z + amp * oms * oms * tstep * SLACK


def rate_distance(e, c, K, mass, motion, xs, tg):
    """h_r per step (the smaller of rows 1 and 2) and the raw commands.
    xs[steps, 12]: states at the step starts; tg[steps, 9]: their targets."""
    dp, dvc, tstep, pabs = step_bounds(e, c, mass)
    s = np.hstack([tg[:, :3] - xs[:, :3], tg[:, 3:6] - xs[:, 3:6]])
    rp, rv = target_reach(e, motion, tg[:, 3:6], tstep)
    d = np.hstack([dp + pabs + rp, dvc + rv])
    Ka = np.abs(np.asarray(K)[1:3, :6])
    lim = c.max_rate * (1.0 - MARGIN)
    num = lim - np.abs(s) @ Ka.T
    den = d @ Ka.T + 1e-300
    raw = s @ np.asarray(K)[1:3, :6].T
    return np.min(num / den, axis=1), raw


def recorded(e, c, cr, K, kc, mass, pat, x0, max_steps=-1):
    """One oracle episode: states and targets at every step start."""
    _, _, _, rec = O.episode(e, c, cr, e.motion, pat, mass, c.hover_thrust, K, kc, x0, max_steps=max_steps,
                             record=True)
    n = int(np.count_nonzero(np.any(rec != 0.0, axis=1)))
    xs = np.vstack([x0[None, :], rec[:n - 1, :12]])
    t, tg = 0.0, np.zeros((n, 9))
    for k in range(n):
        tg[k] = O.target_state(e, e.motion, pat, t)
        t = t + e.dt
    return xs, tg, rec[:n, 12:16]


def check_episode(e, c, K, mass, motion, xs, tg, u):
    """The bound's claim on one episode; returns (h_r, saturated flags)."""
    h, raw = rate_distance(e, c, K, mass, motion, xs, tg)
    n = len(h)
    sat = np.any(np.abs(raw) >= c.max_rate, axis=1)
    # the recomputed raw commands are the oracle's: clipped, they are its actions
    np.testing.assert_allclose(np.clip(raw, -c.max_rate, c.max_rate), u[:, 1:3], rtol=1e-12, atol=1e-12)
    # steps to the next saturated step (n: none before the episode ends)
    nxt = np.full(n + 1, 2 * n, dtype=np.int64)
    for k in range(n - 1, -1, -1):
        nxt[k] = 0 if sat[k] else nxt[k + 1] + 1
    H = np.clip(np.floor(np.minimum(h, K_MAX_HORIZON)), 0, K_MAX_HORIZON).astype(np.int64)
    bad = np.nonzero(H > nxt[:n])[0]
    assert bad.size == 0, (int(bad[0]), float(h[bad[0]]), int(nxt[bad[0]]))
    return h, sat


def start(e, ep, rng, scale):
    pat, off = O.draws(e.motion, [ep])
    if scale is None:  # the env's own reset
        return pat[0], O.initial_state(e, e.motion, pat[0], off[0])
    x0 = O.initial_state(e, e.motion, pat[0], rng.uniform(-scale, scale, 3))
    x0[3:6] = rng.uniform(-3.0, 3.0, 3)
    x0[6:8] = rng.uniform(-0.8, 0.8, 2)
    return pat[0], x0


# the set-ups of test_horizon_cpu.py with 6-column gains: (name, env, controller, offset scale)
CASES = [
    ("lqr_far", {"target": {"motion_type": "linear"}}, {}, 40.0),
    ("lqr_heavy_far", {"target": {"motion_type": "circular"}, "quadcopter": {"mass": 1.8}}, {"mass": 1.8}, 30.0),
    ("lqr_light_aggressive", {"target": {"motion_type": "sinusoidal"}, "quadcopter": {"mass": 0.4}},
     {"mass": 0.4, "q_pos": [10.0, 10.0, 40.0], "q_vel": [1.0, 1.0, 4.0]}, 20.0),
    ("no_drag_fast", {"target": {"motion_type": "linear", "speed": 8.0},
                      "quadcopter": {"drag_coeff_linear": 0.0, "drag_coeff_angular": 0.0}}, {}, 60.0),
]

# Rate clips that act: the default gains against a 0.07 rad/s clip, which the
# first seconds' velocity error (the target's 1 m/s) exceeds, from the env's
# own reset (tests/test_gpu_rate_horizon.py runs the same set-up)
SATURATING_ENV = {"target": {"motion_type": "linear"}}
SATURATING_CTL = {"dt": 0.01, "max_rate": 0.07}
SATURATING_STEPS = 600


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_rate_bound_holds(case):
    name, env_cfg, ctl_cfg, scale = case
    e = O.env_params(env_cfg)
    c, K, kc, _, _ = O.controller(dict(ctl_cfg))
    assert kc == 6
    mass = env_cfg.get("quadcopter", {}).get("mass", 1.0)
    motion = env_cfg["target"]["motion_type"]
    rng = np.random.default_rng(len(name))
    for ep in range(6):
        pat, x0 = start(e, ep, rng, scale)
        xs, tg, u = recorded(e, c, O.criteria(), K, kc, mass, pat, x0)
        assert len(xs) > 100
        check_episode(e, c, K, mass, motion, xs, tg, u)


def test_rate_bound_bench_configuration():
    """The bench workload (linear target, default Riccati-LQR, the env's reset,
    seeds = episode index): the bound holds and never shortens the 62-step
    horizon, at any step of 64 episodes."""
    e = O.env_params({"target": {"motion_type": "linear"}})
    c, K, kc, _, _ = O.controller({"dt": 0.01})
    lo = np.inf
    for ep in range(64):
        pat, x0 = start(e, ep, None, None)
        xs, tg, u = recorded(e, c, O.criteria(), K, kc, 1.0, pat, x0)
        assert len(xs) == 3000
        h, sat = check_episode(e, c, K, 1.0, "linear", xs, tg, u)
        assert not sat.any()
        lo = min(lo, float(np.floor(h).min()))
    print(f"bench configuration: min floor(h_r) = {lo}")
    assert lo >= K_MAX_HORIZON


def test_rate_bound_where_the_clips_act():
    e = O.env_params(SATURATING_ENV)
    c, K, kc, _, _ = O.controller(dict(SATURATING_CTL))
    assert kc == 6
    nsat = nsteps = 0
    for ep in range(16):
        pat, x0 = start(e, ep, None, None)
        xs, tg, u = recorded(e, c, O.criteria(), K, kc, 1.0, pat, x0, max_steps=SATURATING_STEPS)
        h, sat = check_episode(e, c, K, 1.0, "linear", xs, tg, u)
        # less than 2 steps of distance before every saturated step (and none at it)
        ks = np.nonzero(sat)[0]
        assert np.all(h[ks] <= 0.0)
        assert np.all(h[ks[ks > 0] - 1] < 2.0)
        nsat += int(sat.sum())
        nsteps += len(sat)
    print(f"saturating set-up: {nsat} of {nsteps} steps at the rate clip")
    assert nsat > 0.01 * nsteps
