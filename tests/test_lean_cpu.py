"""Host-side checks of the lean per-step frames (include/quadtrack.h ABI 10,
quadtrack.step.LeanFrame): the C declarations against the ctypes side, the
byte count the layout was chosen for, the time table, and the lazy
observation / info containers against a stub source.  No GPU needed."""

import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

from quadtrack import _abi
from quadtrack.step import (INFO_KEYS, Frame, FramePool, LazyInfo, LazyObservation, LeanFrame, TimeTable, lean_words,
                            time_table)

HEADER = os.path.join(ROOT, "include", "quadtrack.h")
LEAN_ENTRY_POINTS = ("qt_lean_reset", "qt_lean_closed_step", "qt_lean_step", "qt_lean_expand")


def test_lean_entry_points_declared_bound_and_exported():
    declared = set(re.findall(r"^int (qt_\w+)\(", open(HEADER).read(), flags=re.M))
    lib = _abi.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r" T (qt_\w+)", nm.stdout))
    for name in LEAN_ENTRY_POINTS:
        assert name in _abi.EXPORTS and name in declared and name in exported, name
        assert getattr(lib, name).argtypes is not None, name
    assert _abi.ABI_VERSION == 10 and lib.qt_abi_version() == 10


PROBE = r"""
#include <stdio.h>
#include "quadtrack.h"
int main(void) {
  printf("QT_ABI_VERSION %d\nQT_LR_X %d\nQT_LR_REWARD %d\nQT_LR_ROWS %d\nQT_FC_ROWS %d\nQT_FB_ROWS %d\n",
         QT_ABI_VERSION, QT_LR_X, QT_LR_REWARD, QT_LR_ROWS, QT_FC_ROWS, QT_FB_ROWS);
  printf("QT_LEAN_BYTES_1000 %lld\nQT_LEAN_BYTES_7 %lld\n", (long long)QT_LEAN_BYTES(1000), (long long)QT_LEAN_BYTES(7));
  return 0;
}
"""


def test_lean_layout_matches_c(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines())}
    assert out["QT_ABI_VERSION"] == _abi.ABI_VERSION
    assert (out["QT_LR_X"], out["QT_LR_REWARD"], out["QT_LR_ROWS"]) == (_abi.LR_X, _abi.LR_REWARD, _abi.LR_ROWS)
    assert (out["QT_FC_ROWS"], out["QT_FB_ROWS"]) == (_abi.FC_ROWS, _abi.FB_ROWS)
    assert out["QT_LEAN_BYTES_1000"] == _abi.lean_bytes(1000) == 121000
    assert out["QT_LEAN_BYTES_7"] == _abi.lean_bytes(7)


def _contract_bytes():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import step_api_bench
    finally:
        sys.path.pop(0)
    return step_api_bench.contract_bytes


def test_config2_closed_step_moves_at_most_300_bytes():
    """The byte condition of the lean layout: config 2's per-step loop (shared
    structured LQR gain, linear target: 3 pattern doubles, freeze_done), counted
    as the full frame's 462 B are counted."""
    contract_bytes = _contract_bytes()
    full = contract_bytes("closed", False, 3, True)
    assert full == {"closed_step": 462}  # the count of the default frame is unchanged
    lean = contract_bytes("closed", False, 3, True, lean=True)
    assert set(lean) == {"closed_step"}
    assert lean["closed_step"] <= 300
    # state, counters and done flag in, pattern in, lean frame out, command out
    assert lean["closed_step"] == (96 + 12 + 1) + 24 + _abi.lean_bytes(1) + 32 == 286


@pytest.mark.parametrize("dt", [0.005, 0.01, 0.02, 1.0 / 3.0])
def test_time_table_is_the_episode_accumulation(dt):
    """ttab[k] is `t = 0.0; t += dt` k times, bit for bit (quadcopter_env.py:191),
    and an extended table keeps its prefix."""
    n = 5000
    ref, t = [], 0.0
    for _ in range(n):
        ref.append(t)
        t += dt
    ref = np.array(ref)
    tab = time_table(dt, n)
    assert tab.dtype == np.float64 and tab.shape == (n,) and tab[0] == 0.0
    np.testing.assert_array_equal(tab.view(np.int64), ref.view(np.int64))
    short = time_table(dt, 37)
    np.testing.assert_array_equal(short.view(np.int64), ref[:37].view(np.int64))
    grown = time_table(dt, n, short)
    np.testing.assert_array_equal(grown.view(np.int64), ref.view(np.int64))
    # the env's table: cover(max_step) makes ttab[max_step + 1] exist, with max_step + 1 < len
    tt = TimeTable(dt, 13, torch.device("cpu"))
    assert tt.len == 13
    tt.cover(10)
    assert tt.len == 13
    first = tt.host.copy()
    for max_step in (12, 99, 4000):
        tt.cover(max_step)
        assert max_step + 1 < tt.len
        np.testing.assert_array_equal(tt.host[:13].view(np.int64), first.view(np.int64))
        np.testing.assert_array_equal(tt.host.view(np.int64), ref[:tt.len].view(np.int64))
        assert tt.dev.shape == (tt.len,) and tt.ptr == tt.dev.data_ptr()
        np.testing.assert_array_equal(tt.dev.numpy().view(np.int64), tt.host.view(np.int64))


def test_lean_env_without_gpu_fails_loudly():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from quadtrack import BatchedQuadcopterEnv

    with pytest.raises(_abi.QuadtrackError):
        BatchedQuadcopterEnv(4, lean=True)


@pytest.mark.parametrize("n", [0, 1, 7, 64, 1001])
def test_lean_frame_views_follow_the_c_layout(n):
    fr = LeanFrame(n, torch.device("cpu"))
    assert lean_words(n) * 8 - _abi.lean_bytes(n) < 8 and fr.buf.numel() == lean_words(n) + 4 * n
    if n == 0:
        return
    base = fr.buf.data_ptr()
    assert fr.f.data_ptr() == base and fr.f.shape == (_abi.LR_ROWS, n) and fr.f.dtype == torch.float64
    assert fr.c.data_ptr() == base + _abi.LR_ROWS * 8 * n and fr.c.shape == (_abi.FC_ROWS, n)
    assert fr.c.dtype == torch.int32
    assert fr.b.data_ptr() == base + (_abi.LR_ROWS * 8 + _abi.FC_ROWS * 4) * n and fr.b.shape == (_abi.FB_ROWS, n)
    assert fr.b.dtype == torch.int8
    assert fr.act_ptr == fr.act.data_ptr() == base + lean_words(n) * 8 and fr.act.shape == (4, n)
    raw = fr.buf.numpy().view(np.uint8)
    f = raw[:_abi.LR_ROWS * 8 * n].view(np.float64).reshape(_abi.LR_ROWS, n)
    f[:] = np.arange(_abi.LR_ROWS * n, dtype=float).reshape(_abi.LR_ROWS, n)
    b = raw[(_abi.LR_ROWS * 8 + _abi.FC_ROWS * 4) * n:_abi.lean_bytes(n)].reshape(_abi.FB_ROWS, n)
    b[:] = 0
    b[_abi.FB_DONE, ::2] = 1
    obs, rew, done, info = fr.step_result(None, with_action=True)
    np.testing.assert_array_equal(obs["quadcopter"]["position"].numpy(), f[0:3].T)
    np.testing.assert_array_equal(obs["quadcopter"]["angular_velocity"].numpy(), f[9:12].T)
    np.testing.assert_array_equal(rew.numpy(), f[_abi.LR_REWARD])
    np.testing.assert_array_equal(done.numpy(), np.arange(n) % 2 == 0)
    assert info["action"].shape == (n, 4) and info["action"].data_ptr() == fr.act_ptr


class StubSource:
    """Stands for LeanSource: hands out a prepared full Frame and counts."""

    def __init__(self, full):
        self.full, self.calls = full, 0

    def frame_of(self, lean):
        if lean.full is None:
            self.calls += 1
            lean.full = self.full
        return lean.full


def _lean_and_stub(n=6):
    dev = torch.device("cpu")
    full = Frame(n, dev)
    full.buf.copy_(torch.arange(full.buf.numel(), dtype=torch.float64))
    lean = LeanFrame(n, dev)
    lean.buf.zero_()
    return lean.seal(), StubSource(full.seal())


def test_lazy_containers_report_every_key_without_expanding():
    lean, src = _lean_and_stub()
    ref_obs, _, _, ref_info = src.full.step_result(with_action=True)
    assert tuple(k for k, _ in src.full.info_items()) == INFO_KEYS
    obs, rew, done, info = lean.step_result(src, with_action=True)
    assert isinstance(obs, LazyObservation) and isinstance(obs, dict) and isinstance(info, LazyInfo)
    # key sets: keys(), in, iteration, len — nothing is expanded by them
    assert list(obs.keys()) == list(ref_obs.keys()) == list(obs) and len(obs) == 3
    assert list(info.keys()) == list(ref_info.keys()) == list(info) and len(info) == len(ref_info)
    assert "target" in obs and "time" in obs and "tracking_error" in info and "nope" not in info
    assert info.get("nope") is None and obs.get("nope", 5) == 5
    # what the lean frame serves
    assert obs["quadcopter"]["velocity"].shape == (6, 3) and rew.shape == (6,) and done.dtype == torch.bool
    assert info["action"].shape == (6, 4) and info.get("action") is info["action"]
    assert src.calls == 0
    # one expansion serves the observation and the info of the step
    assert obs["target"]["position"] is ref_obs["target"]["position"]
    assert src.calls == 1
    assert obs["time"] is ref_obs["time"] and obs.get("time") is ref_obs["time"] and obs.frame is src.full
    assert info["tracking_error"] is ref_info["tracking_error"]
    assert info.get("step") is ref_info["step"]
    assert {k: v for k, v in info.items()}.keys() == ref_info.keys()
    assert all(v is ref_info[k] for k, v in info.items() if k != "action")  # the command is the lean frame's
    assert info["action"].data_ptr() == lean.act_ptr
    assert src.calls == 1


@pytest.mark.parametrize("read", [lambda o, i: o.frame, lambda o, i: o.get("time"), lambda o, i: dict(o),
                                  lambda o, i: {**i}, lambda o, i: list(i.values()), lambda o, i: i.items(),
                                  lambda o, i: i["success"], lambda o, i: o.copy(), lambda o, i: repr(i),
                                  lambda o, i: i == {}])
def test_every_read_of_a_lazy_value_expands_once(read):
    lean, src = _lean_and_stub()
    obs, _, _, info = lean.step_result(src)
    assert "action" not in info and src.calls == 0
    out = read(obs, info)
    assert src.calls == 1
    if isinstance(out, dict):
        assert all(isinstance(v, (torch.Tensor, dict)) for v in out.values())
    read(obs, info)
    assert obs["target"]["velocity"].shape == (6, 3) and info["on_target_ratio"].shape == (6,)
    assert src.calls == 1


def test_a_replaced_lazy_entry_is_kept():
    lean, src = _lean_and_stub()
    obs, _, _, info = lean.step_result(src)
    obs["time"] = 1.5
    del info["violation"]
    assert obs["target"]["position"].shape == (6, 3) and info["step"].shape == (6,)
    assert obs["time"] == 1.5 and "violation" not in info


def test_lean_frames_are_held_and_recycled_like_full_ones():
    """The hold-and-recycle test is the full frame's (one implementation): a
    lean frame is recyclable once every tensor it handed out is dropped; a
    held lazy container pins the frame object itself."""
    lean, src = _lean_and_stub()
    assert not lean.recyclable()  # never handed out

    def hold(pick):
        return pick(*lean.step_result(src, with_action=True))

    hold(lambda o, r, d, i: None)
    assert lean.recyclable()
    for pick in (lambda o, r, d, i: r, lambda o, r, d, i: d, lambda o, r, d, i: i["action"],
                 lambda o, r, d, i: o["quadcopter"], lambda o, r, d, i: o["quadcopter"]["attitude"][:, 1]):
        kept = hold(pick)
        assert not lean.recyclable()
        del kept
        assert lean.recyclable()
    pool = FramePool(4, torch.device("cpu"), size=3, kind=LeanFrame)
    cur, seen = None, []
    for _ in range(6):
        fr = pool.take(cur)
        assert isinstance(fr, LeanFrame)
        out = fr.step_result(src)
        cur = fr
        seen.append(id(fr))
        del fr, out
    assert len(set(seen)) == 2 and len(pool.frames) == 2
    obs = cur.step_result(src)[0]  # a held lazy observation keeps its frame out of the cycle
    nxt = pool.take(None)
    assert nxt is not cur
    nxt2 = pool.take(nxt)
    assert nxt2 is not cur and nxt2 is not nxt
    # once released it is taken again, and a recycled frame forgets its expansion
    cur.full = src.full
    cur_id = id(cur)
    del obs, cur
    again = pool.take(nxt)
    assert id(again) == cur_id and again.full is None


def test_in_place_change_of_a_lean_view_is_detected():
    lean, src = _lean_and_stub()
    obs = lean.observation(src)
    lean.check_intact()
    obs["quadcopter"]["position"].add_(1.0)
    with pytest.raises(RuntimeError, match="modified in place"):
        lean.check_intact()
