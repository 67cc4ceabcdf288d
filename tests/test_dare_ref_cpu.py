"""CPU checks of tests/dare_ref.py, the high-precision DARE reference and
input sets that tests/test_gpu_dare_edges.py holds the kernels against: the
mpmath truth reproduces the scipy fixtures and meets its own residual bound
on every problem, the float64 comparators converge where they must and fail
where they must, and the validation matrices keep their stated distance from
the thresholds.  No GPU."""

import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

import dare_ref as DR
import oracle as O


@pytest.fixture(scope="module")
def truths():
    """Every problem of W and G solved once."""
    W = {n: [DR.mp_dare(q.A, q.B, q.Q, q.R) for q in DR.set_W(n)] for n in DR.W_SIZES}
    G = {s: [DR.mp_dare(q.A, q.B, q.Q, q.R) for q in DR.set_G(*s)] for s in DR.G_SIZES}
    return W, G


def test_mp_dare_reproduces_scipy_fixtures():
    D = np.load(os.path.join(GOLDEN, "dare_cases.npz"))
    cfgs = json.loads(str(D["configs_json"]))
    dense = [i for i, c in enumerate(cfgs) if "Q" in c]
    sel = list(range(10)) + dense[:6]
    assert len(sel) == 16 and not any(D["fallback"][i] for i in sel)
    assert {int(D["n"][i]) for i in sel} == {6, 9}
    for i in sel:
        n = int(D["n"][i])
        A, B = DR.hover_system(n, float(D["dt"][i]), float(D["mass"][i]), float(D["gravity"][i]))
        t = DR.mp_dare(A, B, D["Q"][i][:n, :n], D["R"][i])
        np.testing.assert_allclose(t.K, D["K"][i][:, :n], rtol=1e-8, atol=1e-10, err_msg=str(i))
        np.testing.assert_allclose(t.P, D["P"][i][:n, :n], rtol=1e-8, atol=1e-10, err_msg=str(i))


def test_truth_residual_and_doublings(truths):
    """mp_dare asserts its residual itself; here the recorded figure, and the
    double-double split."""
    W, G = truths
    for t in [t for ts in list(W.values()) + list(G.values()) for t in ts]:
        assert t.residual <= 1e-30
        assert 1 <= t.iters <= 64
        assert np.all(np.abs(t.K_lo) <= np.abs(t.K) * DR.EPS) and np.all(np.abs(t.P_lo) <= np.abs(t.P) * DR.EPS)


def test_oracle_converges_on_W(truths):
    W, _ = truths
    for n in DR.W_SIZES:
        for q, t in zip(DR.set_W(n), W[n]):
            oA, oB = O.system(n, q.dt, q.mass)
            assert np.array_equal(oA, q.A) and np.array_equal(oB, q.B)  # one float64 model everywhere
            P, K = O.dare(n, q.A, q.B, q.Q, q.R)
            assert DR.gain_error(K, t) < 1e-9 and DR.p_error(P, t) < 1e-9
            assert np.all(K[3] == 0.0) and np.all(t.K[3] == 0.0)


def test_np_sda_converges_on_G(truths):
    _, G = truths
    for s in DR.G_SIZES:
        for q, t in zip(DR.set_G(*s), G[s]):
            out = DR.np_sda(q.A, q.B, q.Q, q.R)
            assert out is not None, s
            P, K, it = out
            assert 1 <= it <= 64
            assert DR.gain_error(K, t) < 1e-8 and DR.p_error(P, t) < 1e-8


def test_set_shapes():
    for n in DR.W_SIZES:
        W = DR.set_W(n)
        assert len(W) == 16 and {q.dt for q in W} == set(DR.W_DTS)
        zero_int = [bool(np.all(np.diag(q.Q)[6:] == 0.0)) for q in W]
        assert zero_int == ([False, True] * 8 if n == 9 else [True] * 16)
    for n, p in DR.G_SIZES:
        G = DR.set_G(n, p)
        assert len(G) == 6
        for i, q in enumerate(G):
            assert np.max(np.abs(np.linalg.eigvals(q.A))) == pytest.approx(DR.G_RADII[i % 3], rel=1e-12)
            assert np.linalg.matrix_rank(q.Q) == (n + 1) // 2
            np.testing.assert_allclose(np.linalg.eigvalsh(q.R), 10.0 ** np.linspace(-3, 1, p), rtol=1e-9)


def test_unstabilisable_problems_have_no_sda_solution():
    for a00 in (1.0, 2.0):
        q = DR.unstabilisable(a00)
        assert DR.np_sda(q.A, q.B, q.Q, q.R) is None
    q = DR.linear_rate_problem()
    assert DR.np_sda(q.A, q.B, q.Q, q.R) is not None


def test_gain_error_measure():
    t = DR.Truth(np.eye(2), np.zeros((2, 2)), np.array([[2.0, 1.0], [0.0, 0.0]]), np.zeros((2, 2)), 1, 0.0)
    assert DR.gain_error(np.array([[2.0, 1.5], [0.0, 0.0]]), t) == 0.25  # relative to the row's largest entry
    assert DR.gain_error(np.array([[2.0, 1.0], [0.0, 1e-300]]), t) == np.inf  # a zero row must be exactly zero
    assert DR.gain_error(np.array([[np.nan, 1.0], [0.0, 0.0]]), t) == np.inf
    assert DR.bound(1e-13, None) == 8e-13 and DR.bound(1e-16, 1e-9) == 1e-9 and DR.bound(0.0, None) == DR.FLOOR


def test_set_V_conditions():
    """Every generated matrix keeps its distance from the threshold it is
    near, numpy's Cholesky decides as the eigenvalue predicate does, and each
    threshold is approached from both sides."""
    V = DR.set_V()
    seen = set()
    for c in V:
        k = c.n if c.which == "Q" else c.p
        assert c.M.shape == (k, k)
        want = DR.predicate(c.which, c.M)
        assert DR.cholesky_decision(c.which, c.M) == want, c.label
        seen.add((c.which, c.kind, want))
        if c.kind == "eig":
            thr = DR.Q_THRESHOLD if c.which == "Q" else DR.R_THRESHOLD
            assert np.array_equal(c.M, c.M.T)
            ev = np.linalg.eigvalsh(c.M)
            assert abs(ev[0] - c.lam_min) <= DR.v_margin(c.M) / 64, c.label  # the built matrix has the lambda_min asked for
            assert abs(ev[0] - thr) >= DR.v_margin(c.M), c.label
            assert abs(c.lam_min - thr) >= DR.v_margin(c.M), c.label
            assert want == (c.lam_min >= thr if c.which == "Q" else c.lam_min > thr), c.label
        elif c.kind == "asym":
            d = np.abs(c.M - c.M.T)
            lim = DR.ATOL + DR.RTOL * np.abs(c.M.T)
            assert np.max(np.abs(c.M)) <= 1e-4 and DR.RTOL * np.max(np.abs(c.M)) < 1e-9
            off = d > 0
            assert off.sum() == 2
            assert np.all((d[off] >= 1.5 * lim[off]) | (1.5 * d[off] <= lim[off])), c.label
            assert want == bool(np.all(d <= lim)), c.label
            assert np.linalg.eigvalsh(0.5 * (c.M + c.M.T))[0] >= 1e-6 - 2e-8  # either triangle is far from the eigenvalue tests
        else:
            assert want and np.linalg.matrix_rank(c.M) == 1
    for which in "QR":
        assert {(which, "eig", True), (which, "eig", False), (which, "asym", True), (which, "asym", False)} <= seen


def test_accepted_V_cases_are_solvable():
    """What the status of an accepted V case must be.  With A = 0.5 I every
    accepted case has a solution (np_sda converges), so the dense kernel owes
    status 0.  On the hover model, whose modes are marginal, every accepted
    diagonal case with lambda_min >= 0 is solved by the oracle too; a weight
    that the predicate accepts although it is negative (f = -0.9, -0.5) can
    leave the equation without a solution, which is not the validation's
    doing: there the oracle's outcome is the expectation."""
    unsolved = []
    for c in DR.set_V():
        if not DR.predicate(c.which, c.M):
            continue
        A = 0.5 * np.eye(c.n)
        B = np.eye(c.n)[:, :c.p]
        Q, R = (c.M, np.eye(c.p)) if c.which == "Q" else (np.eye(c.n), c.M)
        assert DR.np_sda(A, B, Q, R) is not None, c.label
        if c.diagonal and c.n in (6, 9):
            A, B = DR.hover_system(c.n, 0.01, 1.0)
            try:
                O.dare(c.n, A, B, Q, R)
            except RuntimeError:
                assert c.lam_min < 0.0, c.label
                unsolved.append(c.label)
    assert unsolved  # the case exists: the GPU test must not expect 0 there
