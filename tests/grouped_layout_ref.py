"""Helpers of the grouped-layout tests (tests/test_gpu_grouped_layouts.py,
tests/test_validate_cpu.py): the table of segment layouts, the layout rule
restated in plain Python, the batch builder and the reference that does not
go through segments.

Layout rule (qt_rollout.hip grouped_waves, the specification the C side is
held to): the non-empty segments, in slot order, each start a new wavefront.
Riders are the first episodes of the first non-empty stationary segment; in
segment order they fill the free lanes of the last wave of every segment
whose motion is not stationary, and the giving segment's own waves hold what
is left.  No stationary segment hosts riders.  More than eight non-empty
segments take one launch set per segment and no riders.

Reference: for each motion type present, a homogeneous batch of exactly those
episodes (the env's target.motion_type, no per-episode motion, no groups, the
grouped batch's own draws) through the plain qt_rollout / qt_rollout_fresh
path, in the same mode and chunking; the per-motion results are scattered
back by episode.  This module imports without a GPU.
"""

from __future__ import annotations

import dataclasses
import types

import numpy as np
import torch

STATIONARY = 0
MAX_STEPS = 400
CHUNKS = (7, 130, 263)
STATE_FIELDS = ("x", "t", "acc", "target", "integ")

_EIGHT = [(3, 64), (4, 70), (2, 30), (1, 64), (3, 10), (4, 1), (2, 1), (0, 200)]

# id -> segments (motion, count) in slot order
LAYOUTS = {
    "twice_stationary": [(0, 100), (1, 100), (0, 100)],
    "adjacent_stationary": [(0, 64), (0, 36), (2, 70)],
    "riders_run_out": [(3, 70), (4, 70), (2, 70), (1, 70), (0, 10)],
    "stationary_all_ride": [(1, 100), (2, 100), (0, 56)],
    "stationary_first": [(0, 150), (1, 70)],
    "stationary_middle": [(1, 70), (0, 150), (2, 70)],
    "full_waves_no_gap": [(1, 128), (0, 50), (2, 64)],
    "eight_segments": list(_EIGHT),
    "nine_segments": _EIGHT[:7] + [(1, 5)] + _EIGHT[7:],
    "empty_segments": [(1, 0), (2, 70), (0, 0), (0, 90), (3, 0)],
    "singles": [(1, 1), (2, 1), (3, 1), (4, 1), (0, 1)],
    "one_wave_of_riders": [(1, 1), (0, 63)],
    "one_rider_left_over": [(1, 1), (0, 64)],
    "no_stationary": [(1, 70), (2, 70)],
    "one_segment_stationary": [(0, 100)],
    "one_segment_figure8": [(4, 65)],
}

# id -> (waves with riders, waves without), counted by hand from the rule above
WAVES = {
    "twice_stationary": (6, 6),
    "adjacent_stationary": (4, 4),
    "riders_run_out": (8, 9),
    "stationary_all_ride": (4, 5),
    "stationary_first": (4, 5),
    "stationary_middle": (5, 7),
    "full_waves_no_gap": (4, 4),
    "eight_segments": (8, 12),
    "nine_segments": (13, 13),
    "empty_segments": (3, 4),
    "singles": (4, 5),
    "one_wave_of_riders": (1, 2),
    "one_rider_left_over": (2, 2),
    "no_stationary": (4, 4),
    "one_segment_stationary": (2, 2),
    "one_segment_figure8": (2, 2),
}


def groups_of(segments):
    """(seg_motion, seg_end) as EpisodeBatch.groups takes them, empty entries kept."""
    return [m for m, _ in segments], [int(v) for v in np.cumsum([c for _, c in segments])]


def slot_motions(segments) -> np.ndarray:
    """The motion of every slot, int8 [n]."""
    return np.concatenate([np.full(c, m, np.int8) for m, c in segments] + [np.empty(0, np.int8)])


def segment_of(segments, slot: int) -> int:
    """Index, in the table's list, of the segment holding `slot`."""
    end = 0
    for i, (_, c) in enumerate(segments):
        end += c
        if slot < end:
            return i
    raise IndexError(slot)


@dataclasses.dataclass
class Layout:
    """BatchDev's segment fields of a one-launch grouped rollout (non-empty segments only)."""

    seg_motion: list
    seg_lo: list
    seg_end: list
    ride_lo: list
    ride_cnt: list
    wave_end: list

    @property
    def waves(self) -> int:
        return self.wave_end[-1] if self.wave_end else 0


def fixed_layout(segments, riders: bool = True) -> Layout | None:
    """The layout the rule above gives; None when the batch has more non-empty
    segments than the one-launch form takes."""
    sm, lo, end, prev = [], [], [], 0
    for m, c in segments:
        if c > 0:
            sm.append(m), lo.append(prev), end.append(prev + c)
        prev += c
    if len(sm) > 8:
        return None
    ride_lo, ride_cnt = [0] * len(sm), [0] * len(sm)
    stat = next((i for i, m in enumerate(sm) if m == STATIONARY), None)
    if riders and stat is not None:
        nxt, avail = lo[stat], end[stat] - lo[stat]
        for i, m in enumerate(sm):
            if m == STATIONARY:
                continue
            take = min((64 - (end[i] - lo[i]) % 64) % 64, avail)
            ride_lo[i], ride_cnt[i] = nxt, take
            nxt, avail = nxt + take, avail - take
        lo[stat] = nxt
    wave_end, waves = [], 0
    for i in range(len(sm)):
        waves += (end[i] - lo[i] + ride_cnt[i] + 63) // 64
        wave_end.append(waves)
    return Layout(sm, lo, end, ride_lo, ride_cnt, wave_end)


def slot_at(lay: Layout, p: int):
    """qt_kernels.hpp slot_at restated: (slot or -1, rider?) of launch position p."""
    w, w0 = p >> 6, 0
    for i in range(len(lay.seg_motion)):
        if w < lay.wave_end[i]:
            q = ((w - w0) << 6) + (p & 63)
            own = lay.seg_end[i] - lay.seg_lo[i]
            if q < own:
                return lay.seg_lo[i] + q, False
            q -= own
            return (lay.ride_lo[i] + q, True) if q < lay.ride_cnt[i] else (-1, False)
        w0 = lay.wave_end[i]
    return -1, False


def wave_motion(lay: Layout, p: int) -> int:
    """qt_kernels.hpp wave_motion restated."""
    for i in range(len(lay.seg_motion)):
        if (p >> 6) < lay.wave_end[i]:
            return lay.seg_motion[i]
    return -1


def positions(lay: Layout) -> dict:
    """slot -> (launch position, rider?) over the whole launch; raises on a slot visited twice."""
    out = {}
    for p in range(64 * lay.waves):
        slot, ride = slot_at(lay, p)
        if slot >= 0:
            if slot in out:
                raise AssertionError(f"slot {slot} at launch positions {out[slot][0]} and {p}")
            out[slot] = (p, ride)
    return out


# ---------------------------------------------------------------- GPU side


def build_grouped(ctl, segments, order_seed: int | None = None, plant_mass=None):
    """The grouped batch of a layout.  order_seed None: a physical batch (slot
    = episode, order None).  Else a logical batch whose `order` is a seeded
    permutation realising the same slot layout: motion[order[slot]] is the
    slot's motion.  Episode e has seed e either way."""
    from quadtrack.rollout import build_batch

    by_slot = slot_motions(segments)
    n = by_slot.size
    if order_seed is None:
        motion, order = by_slot, None
    else:
        order = np.random.default_rng(order_seed).permutation(n).astype(np.int32)
        motion = np.empty(n, np.int8)
        motion[order] = by_slot
    batch = build_batch(ctl, {}, n, seeds=np.arange(n), motion=motion, plant_mass=plant_mass, order=order,
                        group_motion=False)
    return dataclasses.replace(batch, groups=groups_of(segments))


def _columns(ctl, idx: torch.Tensor):
    """The controller as build_batch reads it, restricted to the problems idx
    (per-episode gains, hover thrust and feed-forward rows column for column)."""
    col = lambda t: None if t is None else t.index_select(-1, idx).contiguous()  # noqa: E731
    per = bool(ctl.per_episode)
    ff = getattr(ctl, "ff", None)
    return types.SimpleNamespace(
        K=col(ctl.K) if ctl.K.shape[1] != 1 else ctl.K, k_cols=ctl.k_cols, k_structured=ctl.k_structured,
        hover=col(ctl.hover), ff=ff if ff is None or ff.shape[1] == 1 else col(ff), per_episode=per,
        num_problems=idx.numel() if per else ctl.num_problems, device=ctl.device, ctrl=ctl.ctrl)


def run_fresh(ctl, env_cfg, batch):
    """One launch set: core.rollout_fresh through run_closed_loop."""
    from quadtrack.rollout import run_closed_loop

    res = run_closed_loop(ctl, env_cfg, n=batch.n, batch=batch, max_steps=MAX_STEPS)
    return res.metrics, res.state


def run_chunks(ctl, env_cfg, batch, chunks=CHUNKS, roll_batch=None, perturb=(), record=False):
    """core.reset, then (perturb: st.x[6, column] = 1.2) core.rollout in `chunks`;
    roll_batch: the batch the rollouts take when it is not the reset's."""
    from quadtrack import core
    from quadtrack.env.config import as_env_config

    env, crit = as_env_config(env_cfg).to_params(), core.criteria()
    st = core.RolloutState.empty(batch.n, batch.device)
    core.reset(env, batch, st)
    for col in perturb:
        st.x[6, col] = 1.2
    for k in chunks:
        rec = torch.full((k, 16, batch.n), float("nan"), dtype=torch.float64, device=batch.device) if record else None
        core.rollout(env, ctl.ctrl, crit, roll_batch if roll_batch is not None else batch, st, k, rec)
    return core.episode_metrics(crit, st), st


def reference(ctl, batch, runner, plant_mass=None):
    """(metrics [MET_ROWS, n], state) in episode order from one homogeneous
    run per motion type present: runner(view of ctl, env config, sub-batch)
    -> (metrics, state)."""
    from quadtrack import core
    from quadtrack._abi import MET_ROWS, MOTIONS
    from quadtrack.rollout import build_batch

    n, dev = batch.n, batch.device
    met = torch.full((MET_ROWS, n), float("nan"), dtype=torch.float64, device=dev)
    st = core.RolloutState.empty(n, dev)
    for f in STATE_FIELDS:
        getattr(st, f).fill_(float("nan"))
    for m in sorted(set(batch.motion.tolist())):
        idx = torch.nonzero(batch.motion == m).reshape(-1)
        view = _columns(ctl, idx)
        pm = None if plant_mass is None else np.asarray(plant_mass)[idx.cpu().numpy()]
        sub = build_batch(view, {"target": {"motion_type": MOTIONS[m]}}, idx.numel(), plant_mass=pm,
                          draws=(batch.pattern.index_select(1, idx), batch.offset.index_select(1, idx)))
        assert sub.motion is None and sub.groups is None and sub.order is None
        sm, ss = runner(view, {"target": {"motion_type": MOTIONS[m]}}, sub)
        met.index_copy_(1, idx, sm)
        for f in STATE_FIELDS:
            getattr(st, f).index_copy_(getattr(st, f).dim() - 1, idx, getattr(ss, f))
    return met, st
