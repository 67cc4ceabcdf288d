"""High-precision reference and seeded input sets for the DARE kernels
(csrc/qt_dare.hip): tests/test_dare_ref_cpu.py checks this file on the CPU,
tests/test_gpu_dare_edges.py uses it against the kernels.

Plain Python on mpmath, numpy and scipy; nothing here imports the package
under test.

* mp_dare   the doubling iteration in 60-digit mpmath: the truth.
* np_sda    the same iteration in float64 numpy, for sizes the C oracle does
            not cover (p != 4).
* scipy_dare  what the reference ships: solve_discrete_are and
            K = solve(R + B'PB, B'PA) (riccati_lqr.py:176-182).
* set_W / set_G / set_V  the input sets (fixed seeds).
* gain_error / p_error  the error measures.

The equation: A'XA - X - A'XB (R + B'XB)^-1 B'XA + Q = 0.
"""

from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import mpmath
import numpy as np
import scipy.linalg

MP_DPS = 60          # working precision of the truth, decimal digits
MP_STOP = "1e-36"    # relative change of H at which the mpmath iteration stops (<= 1e-30)
MP_RESIDUAL = "1e-30"  # asserted bound of the truth's own DARE residual, relative to |P|
EPS = 2.0 ** -52
FLOOR = 64 * EPS     # the accuracy bound's third term

Q_THRESHOLD = -1e-10  # min eig(Q) < -1e-10 fails (riccati_lqr.py:57-84)
R_THRESHOLD = 1e-10   # min eig(R) <= 1e-10 fails (riccati_lqr.py:87-116)
ATOL, RTOL = 1e-8, 1e-5  # np.allclose(M, M.T, atol=1e-8)


# ------------------------------------------------------------------ models


def hover_system(n: int, dt: float, mass: float, gravity: float = 9.81):
    """The discrete hover model (riccati_lqr.py:187-316): A = I + A_c dt,
    B = B_c dt, integral rows for n = 9.  The entries are formed as the
    kernels form them, so the truth is the truth of the same float64 model."""
    A = np.eye(n)
    for i in range(3):
        A[i, 3 + i] = dt
    if n == 9:
        for i in range(3):
            A[6 + i, i] = dt
    B = np.zeros((n, 4))
    B[5, 0] = 1.0 / mass * dt
    B[4, 1] = -gravity * dt
    B[3, 2] = gravity * dt
    return A, B


# ------------------------------------------------------------------- truth


@dataclass(frozen=True)
class Truth:
    """A 60-digit solution as double-double: X = X_hi + X_lo, both float64."""
    P: np.ndarray
    P_lo: np.ndarray
    K: np.ndarray
    K_lo: np.ndarray
    iters: int
    residual: float  # max |DARE residual| / max |P|, evaluated in mpmath


def _to_mp(M):
    return mpmath.matrix(np.asarray(M, dtype=np.float64).tolist())


def _hi_lo(M):
    hi = np.array([[float(M[i, j]) for j in range(M.cols)] for i in range(M.rows)])
    lo = np.array([[float(M[i, j] - mpmath.mpf(hi[i, j])) for j in range(M.cols)] for i in range(M.rows)])
    return hi, lo


def _mp_maxabs(M):
    return max(abs(M[i, j]) for i in range(M.rows) for j in range(M.cols))


def _mp_fro(M):
    return mpmath.sqrt(sum(M[i, j] ** 2 for i in range(M.rows) for j in range(M.cols)))


def mp_dare(A, B, Q, R, max_iter: int = 400) -> Truth:
    """Structure-preserving doubling in mpmath (MP_DPS digits), stopped at a
    relative change of H <= MP_STOP; K = (R + B'PB)^-1 B'PA in mpmath too.
    Asserts its own DARE residual <= MP_RESIDUAL |P|."""
    with mpmath.workdps(MP_DPS):
        A0, B0, Q0, R0 = _to_mp(A), _to_mp(B), _to_mp(Q), _to_mp(R)
        n = A0.rows
        eye = mpmath.eye(n)
        G = B0 * mpmath.inverse(R0) * B0.T
        H, Ak = Q0.copy(), A0.copy()
        stop = mpmath.mpf(MP_STOP)
        it, done = 0, False
        while it < max_iter and not done:
            it += 1
            Wi = mpmath.inverse(eye + G * H)
            Y1, Y2 = Wi * Ak, Wi * G
            M = Ak.T * H * Y1
            Hn = H + (M + M.T) / 2
            M = Ak * Y2 * Ak.T
            G = G + (M + M.T) / 2
            Ak = Ak * Y1
            done = _mp_fro(Hn - H) <= stop * _mp_fro(Hn)
            H = Hn
        assert done, f"mpmath doubling iteration did not settle in {max_iter} doublings"
        BtP = B0.T * H
        S = R0 + BtP * B0
        K = mpmath.inverse(S) * (BtP * A0)
        res = A0.T * H * A0 - H - (A0.T * H * B0) * K + Q0
        pmax = _mp_maxabs(H)
        rel = _mp_maxabs(res) / pmax if pmax != 0 else _mp_maxabs(res)
        assert rel <= mpmath.mpf(MP_RESIDUAL), f"truth residual {mpmath.nstr(rel, 5)} |P|"
        P_hi, P_lo = _hi_lo(H)
        K_hi, K_lo = _hi_lo(K)
        return Truth(P_hi, P_lo, K_hi, K_lo, it, float(rel))


# ------------------------------------------------- the float64 comparators


def np_sda(A, B, Q, R, max_iter: int = 64, tol: float = 1e-14):
    """The doubling iteration in float64 numpy (np.linalg.solve), the
    oracle's algorithm at any (n, p).  Returns (P, K, iters), or None when H
    stops being finite or does not settle within max_iter doublings.
    isfinite is tested on H before any norm is formed, and on the norms
    before they are compared: inf <= tol * inf is true."""
    A, B, Q, R = (np.asarray(x, dtype=np.float64) for x in (A, B, Q, R))
    n = A.shape[0]
    with np.errstate(all="ignore"):
        try:
            G = B @ np.linalg.solve(R, B.T)
        except np.linalg.LinAlgError:
            return None
        H, Ak = Q.copy(), A.copy()
        for it in range(1, max_iter + 1):
            try:
                Y = np.linalg.solve(np.eye(n) + G @ H, np.hstack([Ak, G]))
            except np.linalg.LinAlgError:
                return None
            Y1, Y2 = Y[:, :n], Y[:, n:]
            M = Ak.T @ (H @ Y1)
            Hn = H + 0.5 * (M + M.T)
            M = Ak @ (Y2 @ Ak.T)
            G = G + 0.5 * (M + M.T)
            Ak = Ak @ Y1
            if not np.all(np.isfinite(Hn)):
                return None
            dn, hn = np.linalg.norm(Hn - H), np.linalg.norm(Hn)
            if not (np.isfinite(dn) and np.isfinite(hn)):  # a finite H near 1e308 whose squares overflow
                return None
            H = Hn
            if dn <= tol * hn:
                BtP = B.T @ H
                return H, np.linalg.solve(R + BtP @ B, BtP @ A), it
    return None


def scipy_dare(A, B, Q, R):
    """(P, K) as the reference computes them, or None where scipy raises."""
    try:
        with np.errstate(all="ignore"):
            P = scipy.linalg.solve_discrete_are(A, B, Q, R)
            BtP = B.T @ P
            K = np.linalg.solve(R + BtP @ B, BtP @ A)
    except Exception:
        return None
    if not (np.all(np.isfinite(P)) and np.all(np.isfinite(K))):
        return None
    return P, K


# ---------------------------------------------------------- error measures


def gain_error(K, truth: Truth) -> float:
    """max over entries of |K - K_true| / (largest |entry| of that row of
    K_true).  A row of K_true that is identically zero (yaw) must be exactly
    zero in K: any other value is an infinite error."""
    K = np.asarray(K, dtype=np.float64)
    worst = 0.0
    for i in range(K.shape[0]):
        scale = float(np.max(np.abs(truth.K[i])))
        if scale == 0.0:
            if np.any(K[i] != 0.0):
                return math.inf
            continue
        d = np.abs((K[i] - truth.K[i]) - truth.K_lo[i])
        if not np.all(np.isfinite(d)):
            return math.inf
        worst = max(worst, float(np.max(d)) / scale)
    return worst


def p_error(P, truth: Truth) -> float:
    """max |P - P_true| / max |P_true|."""
    d = np.abs((np.asarray(P, dtype=np.float64) - truth.P) - truth.P_lo)
    if not np.all(np.isfinite(d)):
        return math.inf
    return float(np.max(d)) / float(np.max(np.abs(truth.P)))


def bound(e_cpu: float, e_scipy: float | None) -> float:
    """max(e_scipy, 8 e_cpu, 64 * 2^-52): never worse than what the reference
    ships, or within a margin of a CPU run of the same algorithm."""
    return max(8.0 * e_cpu, FLOOR, e_scipy if e_scipy is not None else 0.0)


# ------------------------------------------------------------- input sets


@dataclass(frozen=True)
class Problem:
    A: np.ndarray
    B: np.ndarray
    Q: np.ndarray
    R: np.ndarray
    dt: float = 0.0     # hover problems only
    mass: float = 1.0   # hover problems only

    @property
    def n(self):
        return self.A.shape[0]

    @property
    def p(self):
        return self.B.shape[1]


W_DTS = (0.001, 0.005, 0.01, 0.02, 0.05)
W_SIZES = (6, 9)
G_SIZES = ((2, 1), (6, 4), (9, 4), (16, 8))
G_RADII = (0.5, 1.0, 1.2)


@functools.cache
def set_W(n: int) -> tuple[Problem, ...]:
    """Wide hover problems: 16 for n = 6 or 9, diagonal weights over many
    decades, q_int exactly 0 on every other n = 9 problem."""
    rng = np.random.default_rng(16000 + n)
    out = []
    for i in range(16):
        dt = W_DTS[i % len(W_DTS)]
        mass = float(rng.uniform(0.2, 5.0))
        q = np.concatenate([10.0 ** rng.uniform(-8, 4, 3), 10.0 ** rng.uniform(-8, 4, 3),
                            10.0 ** rng.uniform(-8, 2, 3)])
        r = 10.0 ** rng.uniform(-4, 3, 4)
        if n == 9 and i % 2 == 1:
            q[6:] = 0.0
        A, B = hover_system(n, dt, mass)
        out.append(Problem(A, B, np.diag(q[:n]), np.diag(r), dt, mass))
    return tuple(out)


def _orthogonal(rng, k):
    return np.linalg.qr(rng.normal(size=(k, k)))[0]


@functools.cache
def set_G(n: int, p: int) -> tuple[Problem, ...]:
    """General dense problems: 6 per size; A random with spectral radius
    0.5 / 1.0 / 1.2 in turn, B dense, Q = C'C of rank ceil(n/2), R with
    eigenvalues 10^linspace(-3, 1, p)."""
    rng = np.random.default_rng(17000 + 100 * n + p)
    out = []
    for i in range(6):
        A = rng.normal(size=(n, n))
        A *= G_RADII[i % 3] / np.max(np.abs(np.linalg.eigvals(A)))
        B = rng.normal(size=(n, p))
        C = rng.normal(size=((n + 1) // 2, n))
        Q = C.T @ C
        Q = 0.5 * (Q + Q.T)
        U = _orthogonal(rng, p)
        R = U @ np.diag(10.0 ** np.linspace(-3, 1, p)) @ U.T
        R = 0.5 * (R + R.T)
        out.append(Problem(A, B, Q, R))
    return tuple(out)


# the two valid problems no solver can answer: an uncontrollable mode on, and
# outside, the unit circle (Q = R = I)
def unstabilisable(a00: float, n: int = 2):
    A = np.diag([a00] + [0.5] * (n - 1))
    B = np.zeros((n, 1))
    B[1, 0] = 1.0
    return Problem(A, B, np.eye(n), np.eye(1))


# A = diag(1e-5, 1), Q = diag(1, 1e-9): the marginal mode's P grows at a linear
# rate after a first doubling that changes H by 1e-9 |H| only
def linear_rate_problem():
    return Problem(np.diag([1e-5, 1.0]), np.array([[0.0], [1.0]]), np.diag([1.0, 1e-9]), np.eye(1))


# ---- set V: validation matrices near the thresholds

V_SIZES = ((2, 1), (6, 4), (9, 4), (16, 8))  # (n, p): Q-matrices are n x n, R-matrices p x p
V_FACTORS_Q = (-4.0, -2.0, -1.1, -0.9, -0.5, 0.0, 0.5)  # lambda_min = f * 1e-10, threshold factor -1
V_FACTORS_R = (0.5, 0.9, 1.1, 2.0, 4.0)                  # threshold factor +1
V_SCALES = (1e-3, 1.0)
# At scale 1e3 the margin 64 n 2^-52 |M|_2 reaches 2.3e-10 for n = 16, more
# than |f - threshold factor| = 0.5 leaves (0.5e-10), so the scale-1e3 cases
# use factors 3 away from the threshold, one failing and one passing per weight.
V_SCALE_BIG = 1e3
V_FACTORS_Q_BIG = (-4.0, 2.0)
V_FACTORS_R_BIG = (-2.0, 4.0)
V_DELTAS = (0.5e-8, 2e-8)


@dataclass(frozen=True)
class VCase:
    which: str       # "Q" or "R": the weight under test (its partner is I)
    n: int
    p: int
    M: np.ndarray
    kind: str        # "eig", "asym", "rank1"
    diagonal: bool   # M = np.diag(lambda): also runs through the hover kernels
    lam_min: float = 0.0
    label: str = ""


def v_margin(M) -> float:
    """Distance the smallest eigenvalue must keep from its threshold for the
    decision not to hang on rounding: 64 n 2^-52 |M|_2."""
    return 64 * M.shape[0] * EPS * float(np.linalg.norm(M, 2))


def predicate(which: str, M) -> bool:
    """The reference's decision (riccati_lqr.py:57-116), as oracle._psd / _pd."""
    if not np.allclose(M, M.T, atol=ATOL):
        return False
    ev = np.linalg.eigvalsh(M)
    return not np.any(ev < Q_THRESHOLD) if which == "Q" else not np.any(ev <= R_THRESHOLD)


def cholesky_decision(which: str, M) -> bool:
    """The kernels' restatement: symmetric within allclose, then Q + 1e-10 I
    (R - 1e-10 I) positive definite by Cholesky."""
    if not np.allclose(M, M.T, atol=ATOL):
        return False
    shift = -Q_THRESHOLD if which == "Q" else -R_THRESHOLD
    try:
        np.linalg.cholesky(M + shift * np.eye(M.shape[0]))
        return True
    except np.linalg.LinAlgError:
        return False


@functools.cache
def set_V() -> tuple[VCase, ...]:
    rng = np.random.default_rng(18000)
    out = []
    for n, p in V_SIZES:
        for which, k in (("Q", n), ("R", p)):
            small = V_FACTORS_Q if which == "Q" else V_FACTORS_R
            big = V_FACTORS_Q_BIG if which == "Q" else V_FACTORS_R_BIG
            for scale, f in [(s, f) for s in V_SCALES for f in small] + [(V_SCALE_BIG, f) for f in big]:
                for diagonal in (False, True):
                    lam = scale * 10.0 ** rng.uniform(-2, 0, k)
                    lam[int(rng.integers(k))] = f * 1e-10
                    if diagonal:
                        M = np.diag(lam)
                    else:
                        U = _orthogonal(rng, k)
                        M = U @ np.diag(lam) @ U.T
                        M = 0.5 * (M + M.T)
                    out.append(VCase(which, n, p, M, "eig", diagonal, f * 1e-10,
                                     f"{which}{k} f={f:g} scale={scale:g}{' diag' if diagonal else ''}"))
            if k >= 2:
                # asymmetric: a PD matrix with entries <= 1e-4 (eigenvalues in [1e-6, 1e-5], far above
                # both thresholds and above delta) plus delta at one off-diagonal entry, not its mirror
                for delta in V_DELTAS:
                    U = _orthogonal(rng, k)
                    M = U @ np.diag(10.0 ** rng.uniform(-6, -5, k)) @ U.T
                    M = 0.5 * (M + M.T)
                    i, j = (int(x) for x in rng.choice(k, 2, replace=False))
                    M[i, j] += delta
                    out.append(VCase(which, n, p, M, "asym", False, label=f"{which}{k} asym delta={delta:g}"))
        c = rng.normal(size=n)
        out.append(VCase("Q", n, p, np.outer(c, c), "rank1", False, label=f"Q{n} rank one"))
    return tuple(out)
