"""The elementary functions of csrc/ (qt_math.hpp, qt_device.hpp,
qt_crtrig.hpp, qt_glibc.hpp) as compiled for gfx950, called one lane per
argument through the test-only probe libraries (tests/probe/, built by
build() with the Makefile's own flag sets): "exact" = HIPFLAGS, "fast" =
HIPFLAGS + FASTFLAGS (qt_rollout_fast.hip).  tests/test_math.py checks a host
build of the same headers; this file checks the code the GPU runs, and the
device-only functions on v_rsq_f64 / v_rcp_f64 that no host test reaches.

References are numpy (IEEE sqrt, remainder, clip, separately rounded a + b * c),
mpmath at 200 bits, exact rationals for single-rounding (fma) values, and a
host build with the device's contraction rule for bit equality.  NaN and Inf
arguments go to the exact flavour only: the fast flavour promises nothing for
them.  Every launch has a ragged last wave (n % 64 in {1, 63}).  Lines
starting with RECORD carry the measured maxima (profiles/r12)."""

import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

import test_horizon_cpu as TH
import test_math as TM
from conftest import ROOT

pytestmark = pytest.mark.gpu

PROBE_DIR = os.path.join(ROOT, "tests", "probe", "_lib")
FLAVOURS = ("exact", "fast")
DBL_MAX, DBL_MIN = np.finfo(np.float64).max, np.finfo(np.float64).tiny
TWO_PI = 2 * np.pi


class Probe:
    """One probe library on the current torch device."""

    def __init__(self, flavour):
        import torch

        import quadtrack

        self.torch, self.abi, self.flavour = torch, quadtrack._abi, flavour
        self.dev = quadtrack._abi.require_gpu()
        path = os.path.join(PROBE_DIR, f"libqtprobe_{flavour}.so")
        if not os.path.exists(path):
            pytest.fail(f"device probe library {path} missing: run build() (`make probe` in the package)")
        self.lib = C.CDLL(path)
        self.exact = flavour == "exact"

    def call(self, name, rows, *ins):
        """Launch `name` on the arrays `ins` (equal lengths); returns [rows, n]."""
        ins = [np.ascontiguousarray(a, dtype=np.float64).ravel() for a in ins]
        n = ins[0].size
        assert all(a.size == n for a in ins) and n > 0
        pad = 0 if n % 64 in (1, 63) else (63 - n) % 64  # every launch ends in a ragged wave
        if pad:
            ins = [np.concatenate([a, np.resize(a, pad)]) for a in ins]
        m = n + pad
        assert m % 64 in (1, 63)
        torch, abi = self.torch, self.abi
        dins = [torch.from_numpy(a).to(self.dev) for a in ins]
        out = torch.full((rows, m), float("nan"), dtype=torch.float64, device=self.dev)
        fn = getattr(self.lib, name)
        fn.restype = C.c_int
        fn.argtypes = [C.c_int64] + [C.c_void_p] * (len(ins) + 2)
        with abi.on_device(self.dev):
            rc = fn(m, *[abi.ptr(t) for t in dins], abi.ptr(out), abi.raw_stream(self.dev))
        abi.check(rc, name)
        return out.cpu().numpy()[:, :n]


@pytest.fixture(scope="module", params=FLAVOURS)
def probe(request):
    return Probe(request.param)


@pytest.fixture(scope="module")
def mp():
    return pytest.importorskip("mpmath")


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    """Bitwise equal, any NaN matching any NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def step(x, k):
    """x moved by k units in the last place (x > 0 and the result > 0)."""
    return (bits(x) + k).view(np.float64)


def ulp_err(a, ref):
    return np.abs(a - ref) / np.spacing(np.abs(ref))


def record(probe, what, value):
    print(f"RECORD {probe.flavour:5s} {what}: {value}")


def layouts(special, group, n, rng):
    """Three arrangements of the same n-element multiset (n % 64 == 63), as
    index arrays (position -> element): every `special` element of a group
    inside one wave (one wave per group), exactly one special element per wave,
    and shuffled.  The other elements fill the remaining lanes."""
    sp, rest = np.flatnonzero(special), list(np.flatnonzero(~special))
    assert n % 64 == 63 and n // 64 >= sp.size
    groups = [sp[group[sp] == g] for g in np.unique(group[sp])]
    assert all(g.size <= 64 for g in groups)
    a, fill = [], iter(rest)
    for g in groups:
        a += list(g) + [next(fill) for _ in range(64 - g.size)]
    a += list(fill)
    b, fill = [], iter(rest)
    for w, s in enumerate(sp):
        lane = (7 * w + 3) % 64
        b += [next(fill) for _ in range(lane)] + [s] + [next(fill) for _ in range(63 - lane)]
    b += list(fill)
    out = [np.array(a), np.array(b), rng.permutation(n)]
    for p in out:
        assert np.array_equal(np.sort(p), np.arange(n))
    in_wave = lambda p: np.add.reduceat(special[p].astype(int), np.arange(0, n, 64))  # noqa: E731
    assert np.count_nonzero(in_wave(out[0])) == len(groups) and in_wave(out[1]).max() == 1
    return out


def run_layouts(fn, arrays, perms):
    """fn(*arrays permuted) for each arrangement, mapped back to element
    order; asserts every element's result is the same in all of them."""
    res = []
    for p in perms:
        r = fn(*[a[p] for a in arrays])
        back = np.empty_like(r)
        back[:, p] = r
        res.append(back)
    for r in res[1:]:
        assert np.all(same_bits(r, res[0])), "a lane's result depends on its wave's other lanes"
    return res[0]


# ------------------------------------------------------------ square roots

def sqrt_hard_cases(rng, count):
    """Arguments whose square root lies next to a rounding boundary, built with
    integers and scaled by even powers of two (which the square root halves
    exactly).  First the closest there are: 1 + j 2^-52 and 4 (1 - j 2^-53) for
    odd j, whose roots 1 + j 2^-53 - j^2 2^-107 .. and 2 (1 - j 2^-54 - ..) miss
    a midpoint by j^2 2^-55 ulp.  Then the doubles just below and above
    (m + 1/2)^2 for random 53-bit m."""
    out = []
    for k in (-383, -100, 0, 1, 300, 511):
        for j in range(1, 64, 2):
            out += [np.ldexp(float((1 << 52) + j), 2 * k - 52), np.ldexp(float((1 << 53) - j), 2 * k - 51)]
    for m in rng.integers(1 << 52, 1 << 53, count):
        v = (2 * int(m) + 1) ** 2  # 4 (m + 1/2)^2, odd
        sh = v.bit_length() - 53
        lo = v >> sh
        for k in (-430, -300, -53, -52, 0, 200, 450):
            for q in (lo, lo + 1):  # q 2^sh < v < (q + 1) 2^sh
                out.append(np.ldexp(float(q), sh - 2 + 2 * k))
    return np.array(out)


@pytest.fixture(scope="module")
def sqrt_inputs():
    rng = np.random.default_rng(31)
    m = rng.integers(1, 1 << 26, 4000).astype(np.float64)
    sq = np.concatenate([m * m * 4.0 ** k for k in (-300, -20, 0, 7, 200)])
    hard = sqrt_hard_cases(rng, 600)
    x = np.concatenate([
        np.ldexp(1.0 + rng.random((1023 + 767 + 1, 40)), np.arange(-767, 1024)[:, None]).ravel(),
        np.ldexp(1.0, np.arange(-767, 1024)),
        10.0 ** rng.uniform(-20, 4, 40000),  # the loop's sums of squares
        sq, step(sq, -1), step(sq, 1), hard,
        [2.0 ** -767, step(2.0 ** -767, 1), step(2.0 ** -767, 2), DBL_MAX, step(DBL_MAX, -1), 1.0, 2.0, 4.0]])
    assert x.min() >= 2.0 ** -767 and np.all(np.isfinite(x)) and x.size <= 200000
    return x, hard


def test_sqrt_reference_is_correctly_rounded(sqrt_inputs, mp):
    """np.sqrt on the rounding hard cases against mpmath (the reference of the tests below)."""
    _, hard = sqrt_inputs
    with mp.workprec(200):
        ref = np.array([float(mp.sqrt(mp.mpf(float(v)))) for v in hard[:4000]])
    np.testing.assert_array_equal(np.sqrt(hard[:4000]), ref)


def test_square_roots_bitwise(probe, sqrt_inputs):
    """x >= 2^-767: the device sqrt, sqrt_noscale and sqrt_pos are np.sqrt bit
    for bit; sqrt_sum is within an ulp."""
    x, _ = sqrt_inputs
    out = probe.call("qtp_sqrt", 4, x)
    ref = np.sqrt(x)
    for row, name in enumerate(("sqrt", "sqrt_noscale", "sqrt_pos")):
        bad = np.flatnonzero(bits(out[row]) != bits(ref))
        record(probe, f"{name} bits differing from IEEE sqrt, x >= 2^-767", f"{bad.size} of {x.size}")
        assert bad.size == 0, (name, x[bad[:5]], out[row][bad[:5]], ref[bad[:5]])
    e = ulp_err(out[3], ref)
    record(probe, "sqrt_sum max ulp, x >= 2^-767", f"{e.max():.3f} (share not exact {np.mean(e > 0):.4f})")
    assert e.max() <= 1.0 and np.all(out[3] > 0)


def test_square_roots_small_arguments(probe):
    """Below 2^-767.  The device sqrt stays IEEE (subnormals, 0).  sqrt_noscale
    keeps 0.  sqrt_pos / sqrt_sum return for every x < 2^-1000, subnormals and
    0 included, exactly what they return for 2^-1000, a positive value; from
    there to 2^-767 the result is finite, positive and monotone (no bit claim:
    the measured error is recorded)."""
    rng = np.random.default_rng(32)
    tiny = np.concatenate([np.ldexp(1.0 + rng.random(2000), rng.integers(-1074, -1000, 2000)),
                           [0.0, 5e-324, DBL_MIN, step(DBL_MIN, -1), step(2.0 ** -1000, -1)]])
    assert tiny.max() < 2.0 ** -1000
    mid = np.sort(np.concatenate([np.ldexp(1.0 + rng.random(20000), rng.integers(-1000, -767, 20000)),
                                  [2.0 ** -1000, step(2.0 ** -1000, 1), step(2.0 ** -767, -1)]]))
    assert mid.min() == 2.0 ** -1000 and mid.max() < 2.0 ** -767
    x = np.concatenate([tiny, mid])
    out = probe.call("qtp_sqrt", 4, x)
    assert np.all(bits(out[0]) == bits(np.sqrt(x)))  # the device library's sqrt: every double
    assert out[1][tiny.size - 5] == 0.0 and not np.signbit(out[1][tiny.size - 5])  # sqrt_noscale(0) == 0
    for row, name in ((2, "sqrt_pos"), (3, "sqrt_sum")):
        floor = out[row][tiny.size]  # the value at 2^-1000
        assert floor > 0 and np.isfinite(floor)
        assert np.all(bits(out[row][:tiny.size]) == bits(floor)), name
        r = out[row][tiny.size:]
        record(probe, f"{name} max ulp on [2^-1000, 2^-767)", f"{ulp_err(r, np.sqrt(mid)).max():.3f}")
        assert np.all(np.isfinite(r)) and np.all(r > 0) and np.all(np.diff(r) >= 0), name
    if probe.exact:
        assert np.isnan(probe.call("qtp_sqrt", 4, np.array([np.nan]))[1, 0])  # sqrt_noscale(NaN)


# ------------------------------------------------- squared-norm comparisons

RADII = (0.5, 0.3, 50.0, 1e-3, 1e3, 0.0)  # 50.0: the default max_velocity


def norm_cases(exact):
    """(s, r, in-band mask, group) with every s of the issue's list, then
    values far from r^2 to fill the waves."""
    s, r = [], []
    for rad in RADII:
        r2 = rad * rad
        if rad > 0:
            lo, hi = r2 * (1.0 - 1e-14), r2 * (1.0 + 1e-14)
            v = [step(np.float64(r2), k) for k in range(-4, 5)]
            v += [step(np.float64(e), k) for e in (lo, hi) for k in range(-2, 3)]
            v += [0.0, 0.5 * r2, 2.0 * r2]
        else:
            v = [0.0, 5e-324, 1e-300, 1.0]
        v += [np.inf, np.nan] if exact else []
        s += [float(q) for q in v]
        r += [rad] * len(v)
    s, r = np.array(s), np.array(r)
    r2 = r * r
    band = ~(s < r2 * (1.0 - 1e-14)) & ~(s > r2 * (1.0 + 1e-14))  # the band, or NaN
    n = 64 * int(band.sum()) + 63
    rng = np.random.default_rng(33)
    fr = rng.choice(np.array(RADII), n - s.size)
    fs = fr * fr * np.where(rng.random(fr.size) < 0.5, rng.uniform(0.0, 0.5, fr.size), rng.uniform(2.0, 4.0, fr.size))
    fs = np.where(fr == 0.0, rng.uniform(1e-6, 1.0, fr.size), fs)
    s, r = np.concatenate([s, fs]), np.concatenate([r, fr])
    band = np.concatenate([band, np.zeros(fr.size, bool)])
    group = np.searchsorted(np.sort(RADII), r)
    return s, r, band, group, rng


def test_norm_comparisons(probe):
    """norm_gt / norm_le against np.sqrt(s) > r and np.sqrt(s) <= r on every
    value around r^2 and around the band edges r^2 (1 +- 1e-14), in three
    arrangements of the same lanes (the wave-uniform branch of norm_le)."""
    s, r, band, group, rng = norm_cases(probe.exact)
    # the list holds values whose square root rounds to r although s != r^2 (only the square root decides them),
    # for the radii that have any: around 50^2 and 1000^2 the square root separates neighbouring doubles
    tie = (np.sqrt(s) == r) & (s != r * r)
    assert all(np.any(tie & (r == rad)) for rad in (0.5, 0.3, 1e-3))
    out = run_layouts(lambda a, b: probe.call("qtp_norm", 2, a, b), (s, r), layouts(band, group, s.size, rng))
    with np.errstate(invalid="ignore"):
        gt, le = np.sqrt(s) > r, np.sqrt(s) <= r
    assert not gt[np.isnan(s)].any() and not le[np.isnan(s)].any()
    bad = np.flatnonzero((out[0] != gt) | (out[1] != le))
    assert bad.size == 0, (s[bad[:8]], r[bad[:8]], out[:, bad[:8]])
    record(probe, "norm_gt / norm_le decisions differing from sqrt(s) > r, <= r",
           f"0 of {s.size} ({int(band.sum())} in the band, {int(tie.sum())} ties)")


def fma_exact(a, b, c):
    """a * b + c rounded once."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def test_constrain_speed_clamp(probe):
    """constrain's near-limit test and clamp on velocities whose squared speed
    (dot3_blas: a * a, then two fmas) lies around max_velocity^2: clamped
    exactly when np.sqrt(s) > max_velocity, to v / sqrt(s) * max_velocity."""
    rng = np.random.default_rng(34)
    u = rng.normal(size=(3, 3000))
    u /= np.linalg.norm(u, axis=0)
    r = rng.choice(np.array([0.5, 0.3, 50.0, 1e-3, 1e3]), 3000)
    scale = np.concatenate([np.ones(1000), 1.0 + rng.uniform(-1.5e-14, 1.5e-14, 1500), rng.uniform(0.1, 3.0, 500)])
    v = u * r * scale
    v[1:, :200] = 0.0  # along one axis: s = vx^2, and vx = r gives s = r^2 exactly
    v[0, :100] = r[:100]
    v[0, 100:200] = step(r[100:200], 1)
    out = probe.call("qtp_constrain", 4, v[0], v[1], v[2], r)
    s = np.array([fma_exact(c, c, fma_exact(b, b, a * a)) for a, b, c in v.T])
    assert np.all(bits(out[3]) == bits(s))
    clamp = np.sqrt(s) > r
    assert 200 < clamp.sum() < 2800 and np.any((np.sqrt(s) == r) & (s != r * r))
    ref = np.where(clamp, v / np.sqrt(s) * r, v)
    bad = np.flatnonzero(~np.all(bits(out[:3]) == bits(ref), axis=0))
    assert bad.size == 0, (v[:, bad[:5]], r[bad[:5]], out[:, bad[:5]])


# ---------------------------------------------------------------- angle wrap

def wrap_inputs(exact):
    rng = np.random.default_rng(1)  # the host test's arguments (test_angle_wrap_bit_identical_to_numpy)
    a = np.concatenate([rng.uniform(-4 * np.pi, 4 * np.pi, 200000) + np.pi, rng.uniform(-100, 100, 20000),
                        np.array([0.0, -0.0, 2 * np.pi, -2 * np.pi, 4 * np.pi, -4 * np.pi])])
    edge = []
    for k in (0, 1, -1, 2, -2):  # a + pi at 0, +-2 pi, +-4 pi and around
        c = np.float64(k * TWO_PI - np.pi)
        edge += [float(step(np.abs(c), j) * np.sign(c)) for j in range(-2, 3)]
        edge += [float(np.float64(k * TWO_PI) - np.pi), float(np.nextafter(k * TWO_PI, 9.0) - np.pi)]
    rng = np.random.default_rng(35)
    a = np.concatenate([a[::2], a[-6:], edge, [np.pi, -np.pi, -0.0, 0.0, 1e6, -1e6, 3 * np.pi, -3 * np.pi,
                                                5 * np.pi, -5 * np.pi],
                        rng.uniform(-1e6, 1e6, 20000), rng.uniform(-40, 40, 20000)])
    if exact:
        a = np.concatenate([a, [np.inf, -np.inf, np.nan]])
    return a


def wrap_ref(a):
    with np.errstate(invalid="ignore"):
        return (a + np.pi) % (2 * np.pi) - np.pi


def test_angle_wrap_bitwise(probe):
    """wrap_angles and the device py_mod_2pi against numpy's remainder, bit for
    bit, the sign of a zero included."""
    a0 = wrap_inputs(probe.exact)
    rng = np.random.default_rng(36)
    a1, a2 = a0[::-1].copy(), rng.permutation(a0)
    out = probe.call("qtp_wrap", 4, a0, a1, a2)
    for row, a in enumerate((a0, a1, a2)):
        assert np.all(same_bits(out[row], wrap_ref(a))), row
    with np.errstate(invalid="ignore"):
        ref = a0 % (2 * np.pi)
    assert np.all(same_bits(out[3], ref))
    assert not np.any(np.signbit(out[3][out[3] == 0]))
    record(probe, "wrap_angles / py_mod_2pi bits differing from numpy", f"0 of {3 * a0.size} / {a0.size}")


def test_angle_wrap_big_lane_among_small(probe):
    """A lane whose a + pi lies outside (-4 pi, 4 pi) takes the wave into the
    fmod branch: every lane's result is the same whichever lanes share its wave."""
    rng = np.random.default_rng(37)
    nbig = 40
    n = 64 * nbig + 63
    a = rng.uniform(-3 * np.pi, 3 * np.pi, (3, n))
    big = np.zeros(n, bool)
    big[:nbig] = True
    vals = np.concatenate([rng.uniform(4 * np.pi, 1e6, nbig // 2), -rng.uniform(6 * np.pi, 1e6, nbig // 2)])
    if probe.exact:
        vals[:3] = [np.inf, -np.inf, 1e300]
    a[np.arange(nbig) % 3, np.arange(nbig)] = vals  # one big angle per big lane, in each of the three slots
    assert np.all((np.abs(a + np.pi) >= 4 * np.pi).any(axis=0) == big)
    out = run_layouts(lambda x, y, z: probe.call("qtp_wrap", 4, x, y, z), tuple(a),
                      layouts(big, np.zeros(n, int), n, rng))
    assert np.all(same_bits(out[:3], wrap_ref(a)))


# ------------------------------------------- clips, the two-rounding product

def test_clips(probe):
    """clipd (np.clip with its NaN propagation) and clip_num (v_max / v_min, on
    numbers) against np.clip, bitwise: v below, inside, above, on a bound, and
    a zero of either sign inside the bounds.  Only where v and a bound are
    zeros of opposite sign is the comparison by value: maximum(-0.0, 0.0) may
    return either zero."""
    rng = np.random.default_rng(38)
    n = 60000
    lo, hi = -np.abs(rng.normal(size=n)) - 0.01, np.abs(rng.normal(size=n)) + 0.01
    v = rng.normal(size=n) * 1.5
    v[:1000], v[1000:2000] = lo[:1000], hi[1000:2000]
    v[2000:2500], v[2500:3000] = 0.0, -0.0
    lo[3000:3100], v[3000:3100] = 0.0, -0.0  # opposite zeros
    hi[3100:3200], v[3100:3200], lo[3100:3200] = -0.0, 0.0, -1.0
    lo[3200:3300] = hi[3200:3300]  # lo == hi
    v[3300:3310] = [DBL_MAX, -DBL_MAX, 5e-324, -5e-324, DBL_MIN, 1e300, -1e300, 1.0, -1.0, 0.5]
    assert np.all(lo <= hi)
    out = probe.call("qtp_clip", 2, v, lo, hi)
    ref = np.clip(v, lo, hi)
    ambiguous = (ref == 0) & (v == 0) & ((lo == 0) | (hi == 0))
    for row in (0, 1):
        assert np.all(out[row] == ref)
        assert np.all((bits(out[row]) == bits(ref)) | ambiguous)
    assert np.signbit(out[:, 2500:3000]).all() and not np.signbit(out[:, 2000:2500]).any()
    if probe.exact:
        v[:64] = np.nan
        out = probe.call("qtp_clip", 2, v, lo, hi)
        assert np.isnan(out[0, :64]).all() and np.all(out[0, 64:] == np.clip(v, lo, hi)[64:])


def test_add_product_two_roundings(probe):
    """add_product_rn(a, b, c) is numpy's a + b * c (product rounded, then the
    sum), not the fma, on uniform(-1, 1) triples; the share of triples on which
    a fused result would differ is measured, so the test cannot pass vacuously."""
    rng = np.random.default_rng(39)
    a, b, c = rng.uniform(-1, 1, (3, 100031))
    out = probe.call("qtp_add_product", 1, a, b, c)[0]
    ref = a + b * c
    fused = np.array([fma_exact(y, z, x) for x, y, z in zip(a[:20000], b[:20000], c[:20000])])
    share = np.mean(fused != ref[:20000])
    record(probe, "add_product_rn bits differing from a + b * c", f"{int(np.sum(bits(out) != bits(ref)))} of {a.size} "
           f"(an fma would differ on {share:.1%})")
    assert share >= 0.10
    assert np.all(bits(out) == bits(ref))


# --------------------------------------------------------- polynomial trig

def trig_probe(probe):
    """The device probe in the shape of test_math.py's host probe."""
    def run(x, rotate=False):
        x = np.ascontiguousarray(x, dtype=np.float64)
        if rotate:
            return probe.call("qtp_rotate", 2, *x.reshape(-1, 4).T).T
        return probe.call("qtp_trig", TM.PROBE_COLS, x).T

    return run


HOST_GATES = (TM.test_sincos_accuracy, TM.test_small_angle_sincos_and_rotation, TM.test_tilt_sincos_accuracy,
              TM.test_rate_sincos_accuracy, TM.test_residual_sincos_accuracy, TM.test_tiny_sincos_and_rotate_cm)


@pytest.mark.parametrize("gate", HOST_GATES, ids=lambda t: t.__name__[5:])
def test_polynomial_trig_host_gates(probe, gate):
    """The accuracy tests of tests/test_math.py themselves (same arguments,
    same bounds, numpy as the reference) on the device build."""
    gate(trig_probe(probe))


def test_polynomial_trig_nonfinite_and_wrap_host_gates():
    """The host tests with NaN / Inf arguments: the exact flavour only."""
    run = trig_probe(Probe("exact"))
    TM.test_sincos_nonfinite(run)
    TM.test_angle_wrap_bit_identical_to_numpy(run)


# (function, probe columns, |x| limit, ulp bound sin, ulp bound cos): the bounds of tests/test_math.py
TRIG_DOMAINS = (("fast_sincos", 0, np.pi + 0.2, 2.0, 2.0), ("small_sincos", 3, 0.125, 1.0, 1.0),
                ("sincos_tilt", 5, np.pi / 3, 1.0, 2.0), ("rate_sincos", 7, 0.031, 1.0, 1.0),
                ("resid_sincos", 9, 4e-3, 1.0, None), ("tiny_sincos", 11, 1e-4, 1.0, None))


@pytest.fixture(scope="module")
def trig_mp_reference(mp):
    """Per domain: 3,300 arguments with sin, cos and cos - 1 correctly rounded
    from mpmath (19,800 arguments in all)."""
    ref = {}
    with mp.workprec(200):
        for i, (name, _, lim, _, _) in enumerate(TRIG_DOMAINS):
            x = np.concatenate([np.random.default_rng(40 + i).uniform(-lim, lim, 3298), [lim, -lim]])
            vals = [(mp.sin(v), mp.cos(v)) for v in map(mp.mpf, x.tolist())]
            ref[name] = (x, np.array([float(s) for s, _ in vals]), np.array([float(c) for _, c in vals]),
                         np.array([float(c - 1) for _, c in vals]))
    return ref


def test_polynomial_trig_vs_mpmath(probe, trig_mp_reference):
    """Each function on its own domain against mpmath, to the bounds
    tests/test_math.py asserts: ulp bounds for sin / cos (where |sin|, |cos| >
    1e-3 for fast_sincos, as there), and the absolute bounds 6e-18 / 4.2e-18
    (+ 2 ulp) for the cos - 1 of resid_sincos / tiny_sincos."""
    for name, col, _, bs, bc in TRIG_DOMAINS:
        x, rs, rc, rcm = trig_mp_reference[name]
        out = probe.call("qtp_trig", TM.PROBE_COLS, x)
        s, c = out[col], out[col + 1]
        ok = np.abs(rs) > 1e-3 if name == "fast_sincos" else np.abs(x) > 1e-300
        es = ulp_err(s[ok], rs[ok]).max()
        assert es <= bs, (name, es)
        if bc is not None:
            okc = np.abs(rc) > 1e-3
            ec = ulp_err(c[okc], rc[okc]).max()
            record(probe, f"{name} max ulp vs mpmath (sin, cos)", f"{es:.2f}, {ec:.2f}")
            assert ec <= bc, (name, ec)
        else:
            ea = np.max(np.abs(c - rcm) - 2 * np.spacing(np.abs(rcm)))
            record(probe, f"{name} max ulp vs mpmath (sin), max |cm - (cos - 1)| - 2 ulp", f"{es:.2f}, {ea:.2e}")
            assert ea <= (6e-18 if name == "resid_sincos" else 4.2e-18), (name, ea)


def test_polynomial_trig_bit_equal_to_contracting_host_build(probe, tmp_path_factory):
    """The device code rounds as the host build with the same contraction rule
    does (clang, -ffp-contract=on, FMA): bit-equal on every argument, for the
    functions made of multiplications, additions and fmas only."""
    host = TM.build_host_probe(tmp_path_factory.mktemp("contract"), "contract")
    rng = np.random.default_rng(46)
    x = np.concatenate([rng.uniform(-np.pi - 0.2, np.pi + 0.2, 100000), rng.uniform(-2000.0, 2000.0, 50000),
                        np.arange(-64, 65) * (np.pi / 4), [0.0, -0.0, 1e-300, -1e-20, 5e-9]] +
                       [rng.uniform(-lim, lim, 8000) for _, _, lim, _, _ in TRIG_DOMAINS[1:]])
    dev, ref = probe.call("qtp_trig", TM.PROBE_COLS, x), host(x).T
    names = ("fast_sincos s", "fast_sincos c", "py_mod_2pi", "small_sincos s", "small_sincos c", "sincos_tilt s",
             "sincos_tilt c", "rate_sincos s", "rate_sincos c", "resid_sincos s", "resid_sincos cm", "tiny_sincos s",
             "tiny_sincos cm")
    shares = {nm: float(np.mean(~same_bits(dev[i], ref[i]))) for i, nm in enumerate(names)}
    quads = np.stack([dev[5], dev[6], dev[9], dev[10]], axis=1)  # rotate_cm on (tilt s, c; resid s, cm) of x
    shares["rotate_cm"] = float(np.mean(~same_bits(probe.call("qtp_rotate", 2, *quads.T), host(quads, rotate=True).T)))
    record(probe, "share of results differing in bits from the contracting host build", shares)
    assert all(v == 0.0 for v in shares.values()), shares


def test_rk4_linear_vs_mpmath(probe, mp):
    """rk4_linear (the closed-form step's coefficients) against its Python
    restatement (tests/test_horizon_cpu.py) evaluated in mpmath: every output
    within 4 ulp of the largest stage magnitude (|y|, |y2..4|, |h k1..4|), for
    lam h in [0, 0.5]."""
    rng = np.random.default_rng(47)
    n = 4000
    h = rng.choice(np.array([0.005, 0.01, 0.02, 0.05]), n)
    lam = rng.uniform(0.0, 0.5, n) / h
    y, f = rng.uniform(-1, 1, n), rng.uniform(-10, 10, (4, n))
    y[:300], f[:, :300] = 1.0, 0.0  # the unit inputs of make_rate_lin / make_vel_lin
    y[300:600], f[:, 300:600] = 0.0, 10.0
    y[600:1000], f[:, 600:1000] = 0.0, np.eye(4)[:, np.arange(400) % 4]
    lam[:10] = 0.0
    out = probe.call("qtp_rk4", 5, lam, h, y, *f)
    worst = 0.0
    with mp.workprec(200):
        for i in range(n):
            L, H, Y, F = mp.mpf(lam[i]), mp.mpf(h[i]), mp.mpf(y[i]), [mp.mpf(v) for v in f[:, i]]
            o = TH.rk4_linear(L, H, Y, F)
            ks = [F[0] - L * Y, F[1] - L * o[0], F[2] - L * o[1], F[3] - L * o[2]]
            mag = max([abs(Y)] + [abs(v) for v in o[:3]] + [abs(H * k) for k in ks])
            unit = np.spacing(float(mag))
            worst = max(worst, max(float(abs(mp.mpf(out[k, i]) - o[k])) / unit for k in range(5)))
    record(probe, "rk4_linear max error in ulp of the largest stage magnitude", f"{worst:.2f}")
    assert worst <= 4.0


# ------------------------------- correctly rounded and glibc trig on the device

@pytest.fixture(scope="module")
def cr_reference(mp):
    x = TM._angles(16000, 11)
    with mp.workprec(200):
        return x, np.array([float(mp.sin(mp.mpf(float(v)))) for v in x]), np.array(
            [float(mp.cos(mp.mpf(float(v)))) for v in x])


def test_cr_sincos_bitwise_vs_mpmath(probe, cr_reference):
    x, rs, rc = cr_reference
    out = probe.call("qtp_cr", 2, x)
    record(probe, "cr_sincos bits differing from mpmath (sin, cos)",
           f"{int(np.sum(bits(out[0]) != bits(rs)))}, {int(np.sum(bits(out[1]) != bits(rc)))} of {x.size}")
    np.testing.assert_array_equal(bits(out[0]), bits(rs))
    np.testing.assert_array_equal(bits(out[1]), bits(rc))
    if probe.exact:
        assert np.isnan(probe.call("qtp_cr", 2, np.array([np.inf, -np.inf, np.nan]))).all()


@pytest.fixture(scope="module")
def glibc_reference():
    """The edge list of test_glibc_edge_arguments and 1e5 arguments in the
    eight classes of the host probe, with numpy's scalar results."""
    if not TM._host_has_fma():
        pytest.skip("host libm would run its non-FMA variants, which qt_glibc.hpp does not restate")
    rng = np.random.default_rng(48)
    n = 12500
    u = lambda: rng.random(n)  # noqa: E731
    cls = [(2 * u() - 1) * 8.0, (2 * u() - 1) * 200.0, np.ldexp(1.0 + u(), rng.integers(-30, 0, n)), 0.8 + u() * 1.7,
           (2 * u() - 1) * 1e7, rng.integers(-2 ** 63, 2 ** 63 - 1, n).view(np.float64), (2 * u() - 1) * 2.0,
           np.ldexp(u(), rng.integers(-1074, 1026, n))]
    x = np.concatenate([TM.glibc_edge_arguments()] + cls)
    with np.errstate(all="ignore"):
        xs = x.tolist()
        ref = np.array([[np.sin(v) for v in xs], [np.cos(v) for v in xs], [np.float64(v) ** 2 for v in xs]])
    return x, ref


def test_glibc_restatements_bitwise(probe, glibc_reference):
    """glibc::sin / cos / pow2 on the device against np.sin, np.cos and x**2
    of Python floats (trig for |x| < 105414350, the restated range)."""
    x, ref = glibc_reference
    if not probe.exact:
        keep = np.isfinite(x)
        x, ref = x[keep], ref[:, keep]
    out = probe.call("qtp_glibc", 3, x)
    trig = ~(np.abs(x) >= 105414350.0) | ~np.isfinite(x)
    bad = [int(np.sum(~same_bits(out[0], ref[0]) & trig)), int(np.sum(~same_bits(out[1], ref[1]) & trig)),
           int(np.sum(~same_bits(out[2], ref[2])))]
    record(probe, "glibc sin / cos / pow2 bits differing from numpy", f"{bad} of {int(trig.sum())} / {x.size}")
    assert bad == [0, 0, 0]


# ------------------------------------------------------- figure-8 reciprocal

def test_figure8_reciprocal(probe):
    """figure8_recip's reciprocal alone (amplitude 1, center 0, ct = 1.0: p[0]
    is r): within an ulp of the correctly rounded 1 / den, den = fma(st, st, 1)
    as the device forms it."""
    rng = np.random.default_rng(49)
    h = np.sqrt(0.5)
    st = np.concatenate([rng.uniform(-1, 1, 19000), [0.0, -0.0, 1.0, -1.0, 1e-9, 1e-160],
                         [s * step(np.float64(h), k) for s in (1, -1) for k in range(-3, 4)],
                         rng.uniform(h - 1e-6, h + 1e-6, 400), -rng.uniform(h - 1e-6, h + 1e-6, 400)])
    one = np.ones_like(st)
    r = probe.call("qtp_figure8", 4, one, st, one, one)[0]
    ref = np.array([float(1 / Fraction(fma_exact(v, v, 1.0))) for v in st])
    e = ulp_err(r, ref)
    record(probe, "figure8_recip reciprocal max ulp vs correctly rounded 1 / den",
           f"{e.max():.2f} (share not exact {np.mean(e > 0):.4f})")
    assert e.max() <= 1.0


@pytest.fixture(scope="module")
def figure8_reference(mp):
    """st, ct = sin, cos of theta in [-60, 60], omega in [0.1, 2], amplitude in
    [0.5, 4]; the exact quotient formulas of the target (p0, p1, v0, v1) at
    those doubles from mpmath; and the worst error per component of the same
    expressions in float64 with a correctly rounded 1 / den and with that value
    +- 1 ulp (the model the device bound comes from)."""
    rng = np.random.default_rng(50)
    n = 20000
    th, om, sc = rng.uniform(-60, 60, n), rng.uniform(0.1, 2.0, n), rng.uniform(0.5, 4.0, n)
    st, ct = np.sin(th), np.cos(th)
    exact = []
    with mp.workprec(200):
        for s, c, w, a in zip(*(v.tolist() for v in (st, ct, om, sc))):
            s, c, w, a = mp.mpf(s), mp.mpf(c), mp.mpf(w), mp.mpf(a)
            den, dcos, dsin = 1 + s * s, -s * w, c * w
            dden = 2 * s * dsin
            exact.append((a * c / den, a * s * c / den, a * ((dcos * den - c * dden) / den ** 2),
                          a * (((dsin * c + s * dcos) * den - s * c * dden) / den ** 2)))
    unit = np.empty((4, n))
    for k in range(3):
        unit[k] = np.spacing(np.abs(np.array([float(e[k]) for e in exact])))
    unit[3] = np.spacing(sc * om)  # v1's numerator cancels: in ulp of amplitude * omega

    def errors(vals):
        with mp.workprec(200):
            return np.array([[float(abs(mp.mpf(float(vals[k][i])) - exact[i][k])) for i in range(n)]
                             for k in range(4)]) / unit

    den = 1.0 + st * st
    dcos, dsin = -st * om, ct * om
    dden = 2.0 * st * dsin
    model = np.zeros(4)
    for r in (1.0 / den, np.nextafter(1.0 / den, 0.0), np.nextafter(1.0 / den, 2.0)):
        r2 = r * r
        vals = (sc * ct * r, sc * st * ct * r, sc * ((dcos * den - ct * dden) * r2),
                sc * (((dsin * ct + st * dcos) * den - st * ct * dden) * r2))
        model = np.maximum(model, errors(vals).max(axis=1))
    return (om, st, ct, sc), errors, model


def test_figure8_components(probe, figure8_reference):
    """p[0], p[1], v[0] in ulp of the exact value and v[1] in ulp of amplitude *
    omega: within the float64 model's worst case (reciprocal correctly rounded
    or 1 ulp off) plus 1 ulp for the placement of contractions."""
    (om, st, ct, sc), errors, model = figure8_reference
    e = errors(probe.call("qtp_figure8", 4, om, st, ct, sc)).max(axis=1)
    record(probe, "figure8_recip max ulp p0 p1 v0 v1 (device | model)",
           f"{np.round(e, 2).tolist()} | {np.round(model, 2).tolist()}")
    assert np.all(e <= model + 1.0), (e, model)
