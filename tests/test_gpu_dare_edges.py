"""The DARE kernels (csrc/qt_dare.hip: dare_axis_kernel, dare_row_kernel) at
the places the closed-loop suite does not reach:

* accuracy against a 60-digit mpmath solution (tests/dare_ref.py) on hover
  problems far outside the default tuner ranges (set W) and on general dense
  problems (set G), bounded by the reference's own float64 answers:
      error(gpu) <= max(error(scipy), 8 error(cpu run of the doubling), 64 * 2^-52);
* the validation decisions next to their thresholds (set V), NaN weights;
* the failure statuses on valid inputs, and what a failed problem does to
  the problems that share its wavefront;
* the device fallback gains against the oracle's restatement, bit for bit;
* P == NULL / iters == NULL, shared A / B, batch sizes around a wave and a block.

The structured (axis) and the dense (row) kernel run every hover launch of
this file and must report the same status on every problem.
Reference: riccati_lqr.py:57-184, 737-777; controllers/__init__.py:522-574."""

import functools
import time

import numpy as np
import pytest
import torch

import dare_ref as DR
import oracle as O

pytestmark = pytest.mark.gpu

OK, Q_NOT_PSD, R_NOT_PD, NO_CONVERGE, SINGULAR = 0, 1, 2, 3, 4
MAX_ITER = 64


@pytest.fixture(scope="module")
def qt():
    import quadtrack

    quadtrack._abi.require_gpu()
    return quadtrack


def _dev():
    return torch.device("cuda:0")


def _soa(x):
    """[m, r, c] -> [r*c, m] float64 on the device."""
    x = np.asarray(x, dtype=np.float64)
    return torch.as_tensor(np.ascontiguousarray(x.reshape(x.shape[0], -1).T), device=_dev())


class Out:
    """One launch's outputs on the host: K [m, p, n], P [m, n, n], st [m], it [m]."""

    def __init__(self, K, P, st, it, n, p):
        torch.cuda.synchronize()
        self.K = np.ascontiguousarray(K.cpu().numpy().T).reshape(-1, p, n)
        self.P = None if P is None else np.ascontiguousarray(P.cpu().numpy().T).reshape(-1, n, n)
        self.st = st.cpu().numpy().astype(int)
        self.it = None if it is None else it.cpu().numpy().astype(int)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def assert_same_bits(a: Out, b: Out, ia, ib=None):
    """K, P, status and iters of problems ia of a and ib of b, bit for bit."""
    ib = ia if ib is None else ib
    for f in ("K", "P", "st", "it"):
        assert _bits(getattr(a, f)[ia]) == _bits(getattr(b, f)[ib]), f


def run_dense(core, A, B, Q, R, ab_per_problem=True):
    n, p = Q.shape[1], R.shape[1]
    return Out(*core.dare_dense(_soa(A), _soa(B), _soa(Q), _soa(R), ab_per_problem), n, p)


def run_hover(core, n, dt, gravity, mass, Q, R):
    """Both hover kernels on one batch: {structured: Out}; their statuses must agree."""
    mass = None if mass is None else torch.as_tensor(np.asarray(mass, dtype=np.float64), device=_dev())
    out = {s: Out(*core.dare_batched(n, dt, gravity, mass, _soa(Q), _soa(R), s), n, 4) for s in (True, False)}
    assert np.array_equal(out[True].st, out[False].st), (out[True].st, out[False].st)
    return out


KERNEL = {True: "axis", False: "row"}


# ------------------------------------------------ references, once per module


@functools.cache
def w_refs(n):
    """Per W problem: (truth, oracle (P, K), scipy (P, K) or None)."""
    out = []
    for q in DR.set_W(n):
        P, K = O.dare(n, q.A, q.B, q.Q, q.R)
        out.append((DR.mp_dare(q.A, q.B, q.Q, q.R), (P, K), DR.scipy_dare(q.A, q.B, q.Q, q.R)))
    return out


def dense_ref(q):
    P, K, _ = DR.np_sda(q.A, q.B, q.Q, q.R)
    return DR.mp_dare(q.A, q.B, q.Q, q.R), (P, K), DR.scipy_dare(q.A, q.B, q.Q, q.R)


@functools.cache
def g_refs(n, p):
    return [dense_ref(q) for q in DR.set_G(n, p)]


def bounds(ref):
    """(K bound, P bound, cpu errors, scipy errors) of one problem."""
    truth, cpu, sc = ref
    ek, ep = DR.gain_error(cpu[1], truth), DR.p_error(cpu[0], truth)
    sk, sp = (DR.gain_error(sc[1], truth), DR.p_error(sc[0], truth)) if sc is not None else (None, None)
    return DR.bound(ek, sk), DR.bound(ep, sp), (ek, ep), (sk, sp)


class Ratios:
    """gpu / cpu and gpu / scipy gain-error ratios of one kernel on one set."""

    def __init__(self, name):
        self.name, self.cpu, self.sc, self.worst = name, [], [], 0.0

    def add(self, e, ecpu, esc):
        self.cpu.append(e / max(ecpu, DR.EPS / 2))
        if esc is not None:
            self.sc.append(e / max(esc, DR.EPS / 2))
        self.worst = max(self.worst, e)

    def report(self):
        sc = f"max {max(self.sc):.3g} median {np.median(self.sc):.3g} (of {len(self.sc)})" if self.sc else "none"
        print(f"dare_edges: {self.name}: gain error max {self.worst:.3g}; gpu/cpu max {max(self.cpu):.3g} "
              f"median {np.median(self.cpu):.3g}; gpu/scipy {sc}")


def check_accuracy(out: Out, i, ref, ratios=None, tag=""):
    """Problem i of a launch against its truth, within the bound."""
    truth = ref[0]
    bk, bp, (ek, ep), (sk, sp) = bounds(ref)
    gk, gp = DR.gain_error(out.K[i], truth), DR.p_error(out.P[i], truth)
    if ratios is not None:
        ratios.add(gk, ek, sk)
    assert out.st[i] == OK and 1 <= out.it[i] <= MAX_ITER, (tag, i, out.st[i], out.it[i])
    assert gk <= bk, (tag, i, "K", gk, bk, ek, sk)
    assert gp <= bp, (tag, i, "P", gp, bp, ep, sp)
    return bk, bp


# ------------------------------------------------------------------ accuracy


@pytest.mark.parametrize("n", DR.W_SIZES)
def test_wide_hover_problems_against_truth(qt, n):
    """Set W through both hover kernels.  A launch has one dt: each of the
    five launches holds all 16 problems' weights and masses, and the problems
    whose own dt it is are compared with their truth."""
    t0 = time.perf_counter()
    W, refs = DR.set_W(n), w_refs(n)
    Q, R = np.stack([q.Q for q in W]), np.stack([q.R for q in W])
    mass = np.array([q.mass for q in W])
    ratios = {s: Ratios(f"{KERNEL[s]} kernel, set W n={n}") for s in (True, False)}
    seen = 0
    for dt in DR.W_DTS:
        out = run_hover(qt.core, n, dt, 9.81, mass, Q, R)
        for i in [i for i, q in enumerate(W) if q.dt == dt]:
            seen += 1
            for s in (True, False):
                bk, bp = check_accuracy(out[s], i, refs[i], ratios[s], f"W{n} {KERNEL[s]}")
                assert np.all(out[s].K[i][3] == 0.0)  # the yaw row
            # the two kernels agree within the sum of their bounds
            truth = refs[i][0]
            scale = np.max(np.abs(truth.K[:3]), axis=1, keepdims=True)
            assert np.max(np.abs(out[True].K[i][:3] - out[False].K[i][:3]) / scale) <= 2 * bk
            assert np.max(np.abs(out[True].P[i] - out[False].P[i])) <= 2 * bp * np.max(np.abs(truth.P))
    assert seen == len(W)
    for r in ratios.values():
        r.report()
    print(f"dare_edges: W n={n} took {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("n,p", DR.G_SIZES)
def test_general_dense_problems_against_truth(qt, n, p):
    """Set G through the row kernel, the 6 problems of a size in one launch."""
    G, refs = DR.set_G(n, p), g_refs(n, p)
    out = run_dense(qt.core, *(np.stack([getattr(q, f) for q in G]) for f in "ABQR"))
    ratios = Ratios(f"row kernel, set G n={n} p={p}")
    for i in range(len(G)):
        check_accuracy(out, i, refs[i], ratios, f"G{n}x{p}")
    ratios.report()


def test_linear_rate_problem_against_truth(qt):
    """A marginal mode whose P grows at a linear rate (tests/test_gpu_parity.py
    holds it to scipy at 1e-9): the same bound as W and G, beside set G's
    n = 2 problems."""
    q = DR.linear_rate_problem()
    G = (q,) + DR.set_G(2, 1)[:3]
    out = run_dense(qt.core, *(np.stack([getattr(x, f) for x in G]) for f in "ABQR"))
    check_accuracy(out, 0, dense_ref(q), None, "linear rate")
    assert out.it[0] > 1


# ------------------------------------------------------ validation decisions


def v_status(c):
    if DR.predicate(c.which, c.M):
        return OK
    return Q_NOT_PSD if c.which == "Q" else R_NOT_PD


@pytest.mark.parametrize("n,p", DR.V_SIZES)
@pytest.mark.parametrize("which", ["Q", "R"])
def test_validation_near_thresholds_dense(qt, which, n, p):
    """Set V through the row kernel with A = 0.5 I, B = the first p columns
    of I (shared by the launch) and the partner weight I: exactly the
    predicate's decision, and status 0 where it accepts (every accepted case
    has a solution, tests/test_dare_ref_cpu.py)."""
    cases = [c for c in DR.set_V() if (c.which, c.n, c.p) == (which, n, p)]
    assert len(cases) >= 20
    m = len(cases)
    Q = np.stack([c.M if which == "Q" else np.eye(n) for c in cases])
    R = np.stack([c.M if which == "R" else np.eye(p) for c in cases])
    out = run_dense(qt.core, 0.5 * np.eye(n)[None], np.eye(n)[None, :, :p], Q, R, ab_per_problem=False)
    want = [v_status(c) for c in cases]
    got = out.st.tolist()
    assert got == want, [(c.label, g, w) for c, g, w in zip(cases, got, want) if g != w]
    assert {OK, Q_NOT_PSD if which == "Q" else R_NOT_PD} == set(want) and m == len(got)
    # Q is judged before R: every rejected case again, with the partner weight bad as well
    bad = [c for c, w in zip(cases, want) if w != OK]
    Qb = np.stack([c.M if which == "Q" else -np.eye(n) for c in bad])
    Rb = np.stack([c.M if which == "R" else np.zeros((p, p)) for c in bad])
    outb = run_dense(qt.core, 0.5 * np.eye(n)[None], np.eye(n)[None, :, :p], Qb, Rb, ab_per_problem=False)
    assert outb.st.tolist() == [Q_NOT_PSD] * len(bad)


@pytest.mark.parametrize("n", [6, 9])
@pytest.mark.parametrize("which", ["Q", "R"])
def test_validation_near_thresholds_hover(qt, which, n):
    """Set V's diagonal cases through both hover kernels.  The validation
    decision is the predicate's.  Where it accepts, the status is the
    oracle's outcome on the same problem: 0, except that a weight accepted
    although negative (-0.9e-10, -0.5e-10) can leave the hover model, whose
    open-loop modes are marginal, without a solution (status 3 from the
    oracle, an exception from the reference): that is the solver's answer,
    not the validation's."""
    cases = [c for c in DR.set_V() if c.diagonal and c.which == which and c.n == n]
    assert len(cases) >= 10
    A, B = DR.hover_system(n, 0.01, 1.0)
    Q = np.stack([c.M if which == "Q" else np.eye(n) for c in cases])
    R = np.stack([c.M if which == "R" else np.eye(4) for c in cases])
    want = []
    for c, q, r in zip(cases, Q, R):
        w = v_status(c)
        if w == OK:
            try:
                O.dare(n, A, B, q, r)
            except RuntimeError:
                assert c.lam_min < 0.0
                w = NO_CONVERGE
        want.append(w)
    out = run_hover(qt.core, n, 0.01, 9.81, None, Q, R)
    for s in (True, False):
        got = out[s].st.tolist()
        assert got == want, (KERNEL[s], [(c.label, g, w) for c, g, w in zip(cases, got, want) if g != w])
    assert {OK, Q_NOT_PSD if which == "Q" else R_NOT_PD} <= set(want)


@pytest.mark.parametrize("n", [6, 9])
def test_nan_weight_fails_its_own_test(qt, n):
    """A NaN on the diagonal of Q is QT_DARE_Q_NOT_PSD and one on R's
    QT_DARE_R_NOT_PD, from both kernels, as np.allclose(M, M.T) is false on a
    NaN in the reference (riccati_lqr.py:74, 104).  The axis kernel used to
    pass a NaN through both of its tests and end in QT_DARE_NO_CONVERGE."""
    W = DR.set_W(n)
    spots = [("Q", i) for i in range(n)] + [("R", i) for i in range(4)] + [("QR", 0), (None, 0)]
    Q = np.stack([W[k % 16].Q.copy() for k in range(len(spots))])
    R = np.stack([W[k % 16].R.copy() for k in range(len(spots))])
    want = []
    for k, (which, i) in enumerate(spots):
        if which and "Q" in which:
            Q[k, i, i] = np.nan
        if which and "R" in which:
            R[k, i, i] = np.nan
        want.append(OK if which is None else (Q_NOT_PSD if "Q" in which else R_NOT_PD))
    out = run_hover(qt.core, n, 0.01, 9.81, None, Q, R)
    for s in (True, False):
        assert out[s].st.tolist() == want, KERNEL[s]
    # the general entry, off-diagonal NaNs included
    A = 0.5 * np.eye(n)[None]
    Q[0, 0, 1] = Q[0, 1, 0] = np.nan
    Q[0, 0, 0] = 1.0
    outd = run_dense(qt.core, A, np.eye(n)[None, :, :4], Q, R, ab_per_problem=False)
    assert outd.st.tolist() == want


# ----------------------------------------------- failure statuses, valid inputs


def test_unstabilisable_problems(qt):
    """An uncontrollable mode on the unit circle: H doubles with every
    doubling and never settles (status 3 after all 64 doublings); outside
    it: H overflows and the isfinite exit fires (status 3 sooner).  A NaN in
    A ends the same way."""
    marginal, unstable = DR.unstabilisable(1.0), DR.unstabilisable(2.0)
    with pytest.raises(RuntimeError, match="DARE solver failed"):
        qt.solve_dare(marginal.A, marginal.B, marginal.Q, marginal.R)
    with pytest.raises(RuntimeError, match="DARE solver failed"):
        qt.solve_dare(unstable.A, unstable.B, unstable.Q, unstable.R)
    nan_a = DR.Problem(np.array([[0.5, np.nan], [0.0, 0.5]]), marginal.B, marginal.Q, marginal.R)
    good = DR.set_G(2, 1)[0]
    G = (marginal, unstable, nan_a, good)
    out = run_dense(qt.core, *(np.stack([getattr(x, f) for x in G]) for f in "ABQR"))
    assert out.st.tolist() == [NO_CONVERGE, NO_CONVERGE, NO_CONVERGE, OK]
    assert out.it[0] == MAX_ITER and 1 <= out.it[1] < MAX_ITER and 1 <= out.it[2] < MAX_ITER
    assert not out.K[:3].any() and not out.P[:3].any()  # no hover model: a failed problem's K is zero


def heuristic_K(n, Q, R):
    """The fallback gains the device owes a failed hover problem
    (controllers/__init__.py:537-572 through the oracle's restatement)."""
    q, r = np.diag(Q), np.diag(R)
    K = np.zeros((4, n))
    K[:, :6] = O.heuristic_gains(q[0:3], q[3:6], r[0], np.mean(r[1:4]))
    return K


def assert_fallback(out: Out, i, n, Q, R, tag):
    want = heuristic_K(n, Q, R)
    np.testing.assert_array_equal(out.K[i], want, err_msg=str((tag, i)))  # bit for bit, NaNs in the same places
    assert not np.signbit(out.K[i][want == 0.0]).any()
    assert not out.K[i][3].any() and not out.K[i][:, 6:].any() and not out.P[i].any()


@pytest.mark.parametrize("n", [6, 9])
def test_hover_without_gravity_falls_back(qt, n):
    """gravity = 0: x and y are uncontrollable double integrators.  Status 3
    on every problem from both kernels, P = 0 and K the fallback gains."""
    W = DR.set_W(n)
    Q, R = np.stack([q.Q for q in W]), np.stack([q.R for q in W])
    out = run_hover(qt.core, n, 0.01, 0.0, np.array([q.mass for q in W]), Q, R)
    for s in (True, False):
        assert out[s].st.tolist() == [NO_CONVERGE] * len(W), KERNEL[s]
        assert np.all(out[s].it == MAX_ITER)
        for i in range(len(W)):
            assert_fallback(out[s], i, n, Q[i], R[i], KERNEL[s])


# --------------------------------------- neighbours of a failed problem, fallback


def failed_slot(i):
    """Which problems of a launch fail: a different set of slots in every
    16-problem wave of the axis kernel and every 4-problem wave of the row
    kernel, each wave keeping good problems."""
    return (i + i // 16) % 3 == 0


def check_wave_mix(m, width):
    slots = set()
    for w in range(0, m, width):
        f = [failed_slot(i) for i in range(w, min(w + width, m))]
        assert any(f) and not all(f)
        slots.add(tuple(f))
    assert len(slots) > 1


@pytest.mark.parametrize("n", [6, 9])
def test_hover_neighbours_of_failed_problems(qt, n):
    """40 hover problems (two and a half axis-kernel waves, ten row-kernel
    waves), a third of them failing: a negative q, a zero r, a NaN q, a NaN r,
    and an infinite mass (the z axis uncontrollable: no convergence).  The
    good problems come out bit for bit as in a launch where every failed
    problem is replaced by a good one, and within the accuracy bound; the
    failed ones have their status, P = 0 and the fallback gains."""
    dt, m = 0.01, 40
    pool = [i for i, q in enumerate(DR.set_W(n)) if q.dt == dt]
    assert len(pool) == 3
    W, refs = DR.set_W(n), w_refs(n)
    pick = [pool[i % 3] for i in range(m)]
    Q = np.stack([W[k].Q.copy() for k in pick])
    R = np.stack([W[k].R.copy() for k in pick])
    mass = np.array([W[k].mass for k in pick])
    Qf, Rf, massf = Q.copy(), R.copy(), mass.copy()
    want = np.zeros(m, dtype=int)
    kinds = 0
    for i in range(m):
        if not failed_slot(i):
            continue
        kind = kinds % 5
        kinds += 1
        if kind == 0:
            Qf[i, i % 6, i % 6] = -1.0
        elif kind == 1:
            Rf[i, i % 4, i % 4] = 0.0
        elif kind == 2:
            Qf[i, i % n, i % n] = np.nan
        elif kind == 3:
            Rf[i, i % 4, i % 4] = np.nan
        else:
            massf[i] = np.inf
        want[i] = (Q_NOT_PSD, R_NOT_PD, Q_NOT_PSD, R_NOT_PD, NO_CONVERGE)[kind]
    assert kinds >= 10
    check_wave_mix(m, 16)
    check_wave_mix(m, 4)
    mixed = run_hover(qt.core, n, dt, 9.81, massf, Qf, Rf)
    clean = run_hover(qt.core, n, dt, 9.81, mass, Q, R)
    good = np.flatnonzero(want == OK)
    for s in (True, False):
        assert mixed[s].st.tolist() == want.tolist(), KERNEL[s]
        assert clean[s].st.tolist() == [OK] * m
        assert_same_bits(mixed[s], clean[s], good)
        for i in good[:6]:
            check_accuracy(mixed[s], i, refs[pick[i]], None, f"neighbours {KERNEL[s]}")
        for i in np.flatnonzero(want != OK):
            assert_fallback(mixed[s], i, n, Qf[i], Rf[i], KERNEL[s])


def pivot_breakdown_problem(n):
    """tests/test_gpu_parity.py::test_dense_dare_row_exchange_fallback's
    eps = 0 problem: the first doubling's W = I + G Q has W[0][0] = 0, so the
    inverse without row exchanges breaks down and the wave takes the pivoted
    branch."""
    b = np.zeros((n, 1))
    b[:2, 0] = [1.0, 2.0]
    c = np.zeros(n)
    c[:2] = [1.0, -1.0]
    Q = np.outer(c, c) + np.diag([0.0, 0.0] + [1.0] * (n - 2))
    assert (np.eye(n) + b @ b.T @ Q)[0, 0] == 0.0
    return DR.Problem(0.5 * np.eye(n), b, Q, np.eye(1))


@pytest.mark.parametrize("n", [2, 7, 11])
def test_dense_neighbours_of_failed_problems(qt, n):
    """24 general problems (six waves of the row kernel; n = 2, 7 and 11 reach
    its three sizes): good ones, the pivot-breakdown problem, and failing
    ones (-I for Q, 0 for R, the two unstabilisable problems).  As above;
    without a hover model a failed problem's K is zero."""
    rng = np.random.default_rng(1900 + n)
    m, p = 24, 1
    goods = [DR.Problem(0.5 * np.eye(n) + 0.1 * rng.normal(size=(n, n)), rng.normal(size=(n, p)), np.eye(n),
                        np.eye(p)) for _ in range(3)] + [pivot_breakdown_problem(n)]
    refs = [dense_ref(q) for q in goods]
    fails = [(DR.Problem(goods[0].A, goods[0].B, -np.eye(n), np.eye(p)), Q_NOT_PSD),
             (DR.Problem(goods[1].A, goods[1].B, np.eye(n), np.zeros((p, p))), R_NOT_PD),
             (DR.unstabilisable(1.0, n), NO_CONVERGE), (DR.unstabilisable(2.0, n), NO_CONVERGE)]
    clean = [goods[i % 4] for i in range(m)]
    mixed, want, k = list(clean), [OK] * m, 0
    for i in range(m):
        if failed_slot(i):
            mixed[i], want[i] = fails[k % 4]
            k += 1
    check_wave_mix(m, 4)
    assert k >= 8 and any(not failed_slot(i) and i % 4 == 3 for i in range(m))  # the pivot problem stays in
    om = run_dense(qt.core, *(np.stack([getattr(x, f) for x in mixed]) for f in "ABQR"))
    oc = run_dense(qt.core, *(np.stack([getattr(x, f) for x in clean]) for f in "ABQR"))
    assert om.st.tolist() == want and oc.st.tolist() == [OK] * m
    good = np.flatnonzero(np.array(want) == OK)
    assert_same_bits(om, oc, good)
    for i in good:
        check_accuracy(om, i, refs[i % 4], None, f"dense neighbours n={n}")
    for i in np.flatnonzero(np.array(want) != OK):
        assert not om.K[i].any() and not om.P[i].any()
    unst = [i for i in range(m) if want[i] == NO_CONVERGE]
    assert {int(om.it[i]) == MAX_ITER for i in unst} == {True, False}


@pytest.mark.parametrize("n", [6, 9])
def test_device_fallback_gains(qt, n):
    """Hover problems that fail validation, from both kernels: K[:, :6] is
    the heuristic gain matrix of the oracle bit for bit (a negative q gives
    NaNs, a zero r infinities, in the same places), the integral columns and
    the yaw row are zero, P is zero."""
    W = DR.set_W(n)
    Q, R = np.stack([q.Q.copy() for q in W]), np.stack([q.R.copy() for q in W])
    want = []
    for i in range(len(W)):
        if i % 2 == 0:
            Q[i, i % 6, i % 6] *= -1.0
            want.append(Q_NOT_PSD)
        else:
            R[i, i % 4, i % 4] = 0.0 if i % 4 == 1 else -R[i, i % 4, i % 4]
            want.append(R_NOT_PD)
    out = run_hover(qt.core, n, 0.02, 9.81, np.array([q.mass for q in W]), Q, R)
    for s in (True, False):
        assert out[s].st.tolist() == want, KERNEL[s]
        for i in range(len(W)):
            assert_fallback(out[s], i, n, Q[i], R[i], KERNEL[s])


# ---------------------------------------------------------------- small paths


@pytest.mark.parametrize("n", [6, 9])
def test_axis_kernel_batch_sizes(qt, n):
    """structured=True at batch sizes around a wave (16 problems) and a block
    (64): the first m problems of a 65-problem launch, bit for bit."""
    W = DR.set_W(n)
    pick = [(7 * i) % 16 for i in range(65)]
    Q, R = np.stack([W[k].Q for k in pick]), np.stack([W[k].R for k in pick])
    mass = torch.as_tensor(np.array([W[k].mass for k in pick]), device=_dev())

    def run(m):
        return Out(*qt.core.dare_batched(n, 0.01, 9.81, mass[:m].contiguous(), _soa(Q[:m]), _soa(R[:m]), True), n, 4)

    full = run(65)
    assert full.st.tolist() == [OK] * 65
    for m in (1, 15, 16, 17, 63, 64, 65):
        assert_same_bits(run(m), full, slice(0, m))


def test_row_kernel_batch_sizes(qt):
    """The dense entry at m = 1, 3, 4, 5 (a wave holds 4 problems)."""
    G = DR.set_G(6, 4)[:5]
    arrs = [np.stack([getattr(x, f) for x in G]) for f in "ABQR"]
    full = run_dense(qt.core, *arrs)
    assert full.st.tolist() == [OK] * 5
    for m in (1, 3, 4, 5):
        assert_same_bits(run_dense(qt.core, *(a[:m] for a in arrs)), full, slice(0, m))


def test_null_P_and_iters(qt):
    """The ABI allows P == NULL and iters == NULL: K and status are those of
    the full call, bit for bit (hover entry, both kernels, and dense entry)."""
    from quadtrack import _abi

    lib, ptr, dev = _abi.load(), _abi.ptr, _dev()
    for n in (6, 9):
        W = DR.set_W(n)
        Q, R = _soa(np.stack([q.Q for q in W])), _soa(np.stack([q.R for q in W]))
        m = len(W)
        mass = torch.as_tensor(np.array([q.mass for q in W]), device=dev)
        for s in (True, False):
            full = Out(*qt.core.dare_batched(n, 0.01, 9.81, mass, Q, R, s), n, 4)
            K = torch.full((4 * n, m), np.nan, dtype=torch.float64, device=dev)
            st = torch.full((m,), -1, dtype=torch.int8, device=dev)
            rc = lib.qt_dare_batched(n, m, 0.01, 9.81, ptr(mass), ptr(Q), ptr(R), int(s), ptr(K), None, ptr(st), None,
                                     _abi.stream_of(dev))
            assert rc == 0
            lean = Out(K, None, st, None, n, 4)
            assert _bits(lean.K) == _bits(full.K) and lean.st.tolist() == full.st.tolist() == [OK] * m
    G = DR.set_G(9, 4)
    A, B, Q, R = (_soa(np.stack([getattr(x, f) for x in G])) for f in "ABQR")
    m = len(G)
    full = Out(*qt.core.dare_dense(A, B, Q, R, True), 9, 4)
    K = torch.full((4 * 9, m), np.nan, dtype=torch.float64, device=dev)
    st = torch.full((m,), -1, dtype=torch.int8, device=dev)
    rc = lib.qt_dare_dense(9, 4, m, ptr(A), ptr(B), 1, ptr(Q), ptr(R), ptr(K), None, ptr(st), None,
                           _abi.stream_of(dev))
    assert rc == 0
    lean = Out(K, None, st, None, 9, 4)
    assert _bits(lean.K) == _bits(full.K) and lean.st.tolist() == full.st.tolist() == [OK] * m


def test_shared_system_matrices(qt):
    """ab_per_problem = False with 5 different (Q, R): as the same problems
    with A and B replicated, bit for bit."""
    G = DR.set_G(9, 4)
    A, B = G[0].A, G[0].B
    Q, R = np.stack([x.Q for x in G[:5]]), np.stack([x.R for x in G[:5]])
    shared = run_dense(qt.core, A[None], B[None], Q, R, ab_per_problem=False)
    own = run_dense(qt.core, np.stack([A] * 5), np.stack([B] * 5), Q, R, ab_per_problem=True)
    assert_same_bits(shared, own, slice(0, 5))
    assert shared.st.tolist() == [OK] * 5 and len({_bits(k) for k in shared.K}) == 5
