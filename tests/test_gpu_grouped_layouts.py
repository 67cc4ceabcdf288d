"""The grouped rollout's segment layouts (qt_rollout.hip grouped_waves;
qt_kernels.hpp slot_at, wave_motion, slot_motion and rollout_grouped_kernel's
switch) against a reference that never passes through them.

Every layout of tests/grouped_layout_ref.py's table runs as a grouped batch
(EpisodeBatch.groups exactly as the table lists the segments, empty ones
included) and is held to one homogeneous run per motion type of the same
episodes, in the same mode and chunking, scattered back by episode: metrics,
state, time, accumulators, target observation and controller integral with
torch.equal.  The yaw-at-rest variants (one-lane, pair, DUAL, EQR, UNI, the
rider select, the fresh prologue against reset + rollout) all claim the same
bits, so a grouped run and its per-motion reference may take different ones.

Independent of any reference values, every episode still running at the end
must have taken max_steps steps: a slot the layout drops is named with its
segment.

The deferred mode alone compares at 1e-9 (steps exactly), against the same
launches under recording, which take the exact step everywhere
(tests/test_gpu_workloads.py test_riders_bitwise_and_deferred)."""

import dataclasses
import functools

import numpy as np
import pytest
import torch

import grouped_layout_ref as G

pytestmark = pytest.mark.gpu

LOOP_LAYOUTS = ("twice_stationary", "riders_run_out", "stationary_middle")
ORDER_LAYOUTS = ("twice_stationary", "stationary_middle", "eight_segments")
DEFERRED_LAYOUTS = ("twice_stationary", "stationary_middle")


@pytest.fixture(scope="module")
def qt():
    import quadtrack

    quadtrack._abi.require_gpu()
    return quadtrack


@pytest.fixture(autouse=True)
def _riders_default(monkeypatch):
    monkeypatch.delenv("QT_RIDERS", raising=False)


def _mass(n):
    return 0.8 + 0.4 * np.random.default_rng(5).random(n)


@functools.lru_cache(maxsize=None)
def _controller(loop, n):
    """The loops of tests/test_gpu_workloads.py test_riders_bitwise_other_loops, and plain Riccati-LQR."""
    from quadtrack.controllers import BatchedPID, BatchedRiccatiLQR

    if loop == "lqr":
        return BatchedRiccatiLQR({"dt": 0.01})
    if loop == "lqi":
        return BatchedRiccatiLQR({"dt": 0.01, "use_lqi": True, "q_int": [1e-3, 1e-3, 1e-2], "integral_limit": 10.0,
                                  "integral_zero_threshold": 0.01})
    if loop == "pid":
        return BatchedPID({})
    if loop == "feedforward":
        return BatchedRiccatiLQR({"dt": 0.01, "feedforward_enabled": True, "ff_velocity_gain": 0.5,
                                  "ff_acceleration_gain": 0.2})
    assert loop == "mass"
    return BatchedRiccatiLQR({"dt": 0.01}, mass=_mass(n))


def _setup(layout, loop="lqr", order_seed=None):
    segs = G.LAYOUTS[layout]
    n = sum(c for _, c in segs)
    ctl = _controller(loop, n if loop == "mass" else 0)
    mass = _mass(n) if loop == "mass" else None
    return segs, ctl, mass, G.build_grouped(ctl, segs, order_seed=order_seed, plant_mass=mass)


_RUNNERS = {"fresh": G.run_fresh, "chunked": G.run_chunks,
            "once": functools.partial(G.run_chunks, chunks=(G.MAX_STEPS,))}


@functools.lru_cache(maxsize=None)
def _reference(layout, loop, mode, order_seed=None):
    """Computed once per (layout, loop, mode) and shared; nobody writes to it."""
    _, ctl, mass, batch = _setup(layout, loop, order_seed)
    return G.reference(ctl, batch, _RUNNERS[mode], plant_mass=mass)


def _check(segs, batch, got, ref):
    """Every running episode stepped to the end; then every field bit for bit."""
    from quadtrack._abi import MET

    (met, st), (rmet, rst) = got, ref
    slot_of = torch.arange(batch.n) if batch.order is None else torch.argsort(batch.order.cpu().to(torch.int64))
    running = met[MET["termination_code"]] == 0
    lost = running & ((met[MET["steps"]] != G.MAX_STEPS) | (st.t != rst.t))
    if bool(lost.any()):
        eps = torch.nonzero(lost).reshape(-1).cpu().tolist()
        names, per_segment = [], {}
        for e in eps:
            i = G.segment_of(segs, int(slot_of[e]))
            per_segment[i] = per_segment.get(i, 0) + 1
        names.append("per segment " + ", ".join(f"{i} {segs[i]}: {k}" for i, k in sorted(per_segment.items())))
        for e in eps[:6]:
            slot = int(slot_of[e])
            i = G.segment_of(segs, slot)
            names.append(f"slot {slot} (segment {i} {segs[i]}: steps {int(met[MET['steps'], e])}, "
                         f"t {float(st.t[e])} for {float(rst.t[e])})")
        raise AssertionError(f"{len(eps)} running episodes never stepped to the end: " + "; ".join(names))
    assert torch.equal(met, rmet), "metrics"
    for f in G.STATE_FIELDS:
        assert torch.equal(getattr(st, f), getattr(rst, f)), f


@pytest.mark.parametrize("layout", list(G.LAYOUTS))
def test_layout_fresh(qt, layout):
    """One launch set (core.rollout_fresh)."""
    segs, ctl, _, batch = _setup(layout)
    _check(segs, batch, G.run_fresh(ctl, {}, batch), _reference(layout, "lqr", "fresh"))


@pytest.mark.parametrize("layout", list(G.LAYOUTS))
def test_layout_chunked(qt, layout):
    """core.reset, then launches of 7, 130 and 263 steps: the target phase and
    the riders' state carried across launches."""
    segs, ctl, _, batch = _setup(layout)
    _check(segs, batch, G.run_chunks(ctl, {}, batch), _reference(layout, "lqr", "chunked"))


@pytest.mark.parametrize("layout", list(G.LAYOUTS))
def test_layout_riders_off(qt, monkeypatch, layout):
    """QT_RIDERS=0: the same reference, so the same bits as with riders."""
    monkeypatch.setenv("QT_RIDERS", "0")
    segs, ctl, _, batch = _setup(layout)
    _check(segs, batch, G.run_fresh(ctl, {}, batch), _reference(layout, "lqr", "fresh"))


@pytest.mark.parametrize("layout", ORDER_LAYOUTS)
def test_layout_permuting_order(qt, layout):
    """A logical batch whose `order` (a seeded permutation) realises the slot
    layout, given to core.rollout as it is: episode_of with riders."""
    segs, ctl, _, batch = _setup(layout, order_seed=31)
    assert batch.order is not None
    got = G.run_chunks(ctl, {}, batch, chunks=(G.MAX_STEPS,))
    _check(segs, batch, got, _reference(layout, "lqr", "once", 31))


@pytest.mark.parametrize("mode", ["fresh", "chunked"])
@pytest.mark.parametrize("loop", ["lqi", "pid", "feedforward", "mass"])
@pytest.mark.parametrize("layout", LOOP_LAYOUTS)
def test_layout_other_loops(qt, layout, loop, mode):
    """LQI, PID, feed-forward, per-episode plant mass with per-episode gains."""
    segs, ctl, _, batch = _setup(layout, loop)
    _check(segs, batch, _RUNNERS[mode](ctl, {}, batch), _reference(layout, loop, mode))


def test_layout_without_per_episode_motion(qt):
    """batch.motion None: the kernel trusts seg_motion and rollout_batch gives
    no riders.  (The reset still needs each episode's motion, so it takes the
    batch with them; the rollout the one without.)"""
    segs, ctl, _, batch = _setup("stationary_middle")
    got = G.run_chunks(ctl, {}, batch, chunks=(G.MAX_STEPS,), roll_batch=dataclasses.replace(batch, motion=None))
    _check(segs, batch, got, _reference("stationary_middle", "lqr", "once"))


@pytest.mark.parametrize("layout", DEFERRED_LAYOUTS)
def test_layout_deferred(qt, layout):
    """Three slots start beyond the tilt clamp (roll 1.2), so their waves go to
    the exact pass: a rider, a host lane of the wave it sits in, and a slot in
    the last wave of the second stationary segment (stationary_middle: of the
    stationary segment).  Against the same launches under recording."""
    from quadtrack._abi import MET

    segs, ctl, _, batch = _setup(layout)
    lay = G.fixed_layout(segs)
    pos = G.positions(lay)
    # the first segment that hosts riders: its first rider (ride_lo) follows its
    # last own slot (seg_end - 1) in launch order, so both sit in its last wave
    host = next(i for i, c in enumerate(lay.ride_cnt) if c > 0)
    rider, lane = lay.ride_lo[host], lay.seg_end[host] - 1
    # the last slot of the last stationary segment lies in that segment's last wave
    last = max(i for i, m in enumerate(lay.seg_motion) if m == G.STATIONARY)
    tail = lay.seg_end[last] - 1
    assert pos[rider][1] and not pos[lane][1] and pos[rider][0] >> 6 == pos[lane][0] >> 6
    assert not pos[tail][1] and pos[tail][0] >> 6 == lay.wave_end[last] - 1 and len({rider, lane, tail}) == 3
    if layout == "twice_stationary":
        assert last != lay.seg_motion.index(G.STATIONARY)  # the segment that gives no riders
    slots = (rider, lane, tail)
    mf, sf = G.run_chunks(ctl, {}, batch, chunks=(150, 250), perturb=slots)
    me, se = G.run_chunks(ctl, {}, batch, chunks=(150, 250), perturb=slots, record=True)
    assert torch.equal(mf[MET["steps"]], me[MET["steps"]])
    assert bool((mf[MET["steps"]][mf[MET["termination_code"]] == 0] == G.MAX_STEPS).all())
    np.testing.assert_allclose(mf.cpu().numpy(), me.cpu().numpy(), rtol=1e-9, atol=1e-9)
    for f in ("x", "t", "target"):
        np.testing.assert_allclose(getattr(sf, f).cpu().numpy(), getattr(se, f).cpu().numpy(), rtol=1e-9, atol=1e-9,
                                   err_msg=f)
