"""The supervised policy rollout, the parts that need no GPU: the exports and
the struct layout, the C entry point's refusals before any launch, the sample
step schedule, and the reference fixture (tests/golden/imitation.npz) pinned
against the CPU oracle's controllers."""

import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import oracle as O
import quadtrack
from quadtrack import _abi
from quadtrack.policy import sample_steps

HEADER = os.path.join(ROOT, "include", "quadtrack.h")
ENTRY_POINTS = ("qt_policy_supervised_version", "qt_policy_supervised_rollout")


def test_version_and_exports():
    lib = _abi.load()
    assert lib.qt_policy_supervised_version() == 1 == _abi.POLICY_SUPERVISED_VERSION
    assert _abi.has_policy_supervised()
    src = open(HEADER).read()
    declared = set(re.findall(r"^int (qt_\w+)\(", src, flags=re.M))
    for name in ENTRY_POINTS:
        assert name in declared and name in _abi.EXPORTS and hasattr(lib, name), name
    assert "typedef struct qt_policy_supervision" in src and _abi.SUP_ROWS == 26
    # additive: the other versions are unchanged
    assert lib.qt_abi_version() == 10 and lib.qt_policy_version() == 1 and lib.qt_policy_population_version() == 1
    for name in ("run_policy_supervised", "SupervisedResult", "train_imitation", "ImitationResult"):
        assert name in quadtrack.__all__ and hasattr(quadtrack, name), name
    assert hasattr(quadtrack.BatchedDeepPolicy, "rollout_supervised")
    assert quadtrack.train_imitation is quadtrack.train.train_imitation


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "quadtrack.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f));
int main(void) {
  printf("qt_policy_supervision %zu\n", sizeof(qt_policy_supervision));
  F(qt_policy_supervision, samples) F(qt_policy_supervision, pad_) F(qt_policy_supervision, sample_steps)
  F(qt_policy_supervision, sample) F(qt_policy_supervision, loss) F(qt_policy_supervision, teacher_rec)
  printf("QT_SUP_ROWS %d\n", QT_SUP_ROWS);
  return 0;
}
"""


def test_ctypes_mirror_qt_policy_supervision(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    assert len(lines) == 8
    for line in lines:
        k, v = line.split()
        if "." in k:
            assert getattr(_abi.PolicySupervision, k.split(".")[1]).offset == int(v), k
        elif k == "QT_SUP_ROWS":
            assert int(v) == _abi.SUP_ROWS
        else:
            assert C.sizeof(_abi.PolicySupervision) == int(v)


def test_c_entry_point_refuses_before_any_launch():
    """QT_EINVAL for every refusal the header lists (no GPU needed: nothing is launched)."""
    lib = _abi.load()
    dummy = (C.c_double * 4)()
    addr = C.addressof(dummy)

    def policy(n_hidden=2, widths=(64, 64), activation=0, params=True):
        p = _abi.Policy()
        p.n_hidden = n_hidden
        for i, w in enumerate(widths):
            p.width[i] = w
        p.activation = activation
        p.params = addr if params else None
        return p

    def rc(pol=None, n=5, nsteps=0, k_cols=6, K=True, use_lqi=None, ff=0, batch_ff=False, order=False, integ=True,
           samples=0, sample_steps=False, sample=False, loss=True, null=()):
        pol = policy() if pol is None else pol
        env, crit, ctrl, b, sup, st = (_abi.EnvParams(), _abi.Criteria(), _abi.CtrlParams(), _abi.Batch(),
                                       _abi.PolicySupervision(), _abi.State())
        ctrl.use_lqi = int(k_cols == 9) if use_lqi is None else use_lqi
        ctrl.feedforward_enabled = ff
        b.n, b.k_cols = n, k_cols
        b.K = addr if K else None
        b.order = addr if order else None
        b.ff = addr if batch_ff else None
        st.integ = addr if integ else None
        sup.samples = samples
        sup.sample_steps = addr if sample_steps else None
        sup.sample = addr if sample else None
        sup.loss = addr if loss else None
        ref = lambda name, v: None if name in null else C.byref(v)  # noqa: E731
        return lib.qt_policy_supervised_rollout(ref("env", env), ref("ctrl", ctrl), ref("policy", pol),
                                                ref("crit", crit), ref("batch", b), st, nsteps, ref("sup", sup),
                                                None, None)

    # valid, nothing to do: nsteps == 0 or n == 0
    for kc in (3, 6, 9):
        assert rc(k_cols=kc) == 0
    assert rc(n=0, nsteps=7) == 0
    assert rc(samples=3, sample_steps=True, sample=True) == 0
    assert rc(k_cols=6, integ=False) == 0  # k_cols 6 carries no integral
    # qt_policy_rollout's rules
    assert rc(nsteps=3) == -1  # NULL state arrays, refused before the launch
    for name in ("env", "policy", "crit", "batch"):
        assert rc(null=(name,)) == -1, name
    assert rc(policy(params=False)) == -1
    assert rc(policy(n_hidden=0)) == -1
    assert rc(policy(n_hidden=5, widths=(8, 8, 8, 8))) == -1
    assert rc(policy(widths=(64, 129))) == -1
    assert rc(policy(widths=(0, 64))) == -1
    assert rc(policy(activation=4)) == -1
    assert rc(policy(activation=-1)) == -1
    assert rc(n=-1) == -1
    assert rc(nsteps=-1) == -1
    assert rc(order=True) == -1
    # the teacher's
    assert rc(null=("ctrl",)) == -1
    assert rc(null=("sup",)) == -1
    assert rc(loss=False) == -1
    assert rc(K=False) == -1
    for kc in (0, 4, 8, 12, -3):
        assert rc(k_cols=kc, use_lqi=0) == -1, kc
    assert rc(k_cols=9, use_lqi=0) == -1
    assert rc(k_cols=6, use_lqi=1) == -1
    assert rc(k_cols=3, use_lqi=1) == -1
    assert rc(k_cols=9, integ=False) == -1
    assert rc(k_cols=3, integ=False) == -1
    assert rc(samples=-1) == -1
    assert rc(samples=2) == -1
    assert rc(samples=2, sample_steps=True) == -1
    assert rc(samples=2, sample=True) == -1
    assert rc(ff=1) == -1
    assert rc(batch_ff=True) == -1
    # the order of the checks: an invalid argument is refused for n == 0 and nsteps == 0 too
    assert rc(n=0, k_cols=5) == -1 and rc(n=0, ff=1) == -1 and rc(n=0, loss=False) == -1


# ------------------------------------------------------------------ sample steps

@pytest.mark.parametrize("n,S,H", [(1, 1, 1), (7, 32, 3000), (130, 8, 40), (5, 40, 40), (3, 7, 40), (4, 0, 10),
                                   (0, 4, 10), (2, 3, 301)])
def test_sample_steps_properties(n, S, H):
    s = sample_steps(n, S, H, seed=4)
    assert s.dtype == np.int32 and s.shape == (S, n)
    lo = np.arange(S) * H // max(S, 1)
    hi = (np.arange(S) + 1) * H // max(S, 1)
    assert ((s >= lo[:, None]) & (s < hi[:, None])).all()  # slot j in its stratum
    assert (np.diff(s.astype(np.int64), axis=0) > 0).all()  # strictly ascending per episode, so distinct
    assert np.array_equal(s, sample_steps(n, S, H, seed=4))  # a function of its arguments
    if S == H:
        assert np.array_equal(s, np.repeat(np.arange(H, dtype=np.int32)[:, None], n, axis=1))


def test_sample_steps_seed_and_refusals():
    a, b = sample_steps(64, 8, 400, seed=0), sample_steps(64, 8, 400, seed=1)
    assert not np.array_equal(a, b)
    # an episode's steps do not depend on the call's global numpy state
    np.random.seed(0)
    c = sample_steps(64, 8, 400, seed=0)
    assert np.array_equal(a, c)
    # every step of a stratum is drawn (uniform over it, both ends reached)
    wide = sample_steps(4000, 4, 20, seed=2)
    for j in range(4):
        assert set(np.unique(wide[j])) == set(range(5 * j, 5 * j + 5))
    with pytest.raises(ValueError, match="do not fit"):
        sample_steps(4, 41, 40)
    with pytest.raises(ValueError):
        sample_steps(4, -1, 40)
    with pytest.raises(ValueError):
        sample_steps(-1, 1, 40)


def test_python_refusals_need_no_launch():
    with pytest.raises(TypeError):
        quadtrack.train_imitation({"hidden_sizes": [8]}, epochs=1, episodes_per_epoch=1)
    pol = quadtrack.DeepTrackingPolicy({"hidden_sizes": [8]}, device="cpu")
    for kw in ({"epochs": 0}, {"episodes_per_epoch": 0}, {"batch_size": 0}, {"samples_per_episode": 0}):
        with pytest.raises(ValueError):
            quadtrack.train_imitation(pol, **{"epochs": 1, "episodes_per_epoch": 1, **kw})
    with pytest.raises(ValueError, match="Unknown optimizer"):
        quadtrack.train_imitation(pol, epochs=1, episodes_per_epoch=1, optimizer="lion")


# ------------------------------------------------------------------ the fixture against the oracle

FX = np.load(os.path.join(GOLDEN, "imitation.npz"))
META = json.loads(str(FX["meta_json"]))
RUNS = [(n, s["name"], m) for n in META["nets"] for s in META["supervisors"] for m in META["motions"]]


def test_fixture_shape():
    assert META["nets"] == ["lqr", "n1"] and META["motions"] == ["stationary", "circular"]
    assert [s["name"] for s in META["supervisors"]] == ["pid", "lqr", "riccati", "lqi"]
    assert META["steps"] == 300 and META["episodes"] == 4
    assert META["stored"] == list(range(10)) + list(range(10, 300, 10))
    base = json.loads(str(np.load(os.path.join(GOLDEN, "deep_policy.npz"))["meta_json"]))["base_seeds"]
    for net in META["nets"]:
        for motion in META["motions"]:
            assert FX[f"{net}/{motion}/seeds"].tolist() == [base[f"{net}/{motion}"] + i for i in range(4)]
    assert os.path.getsize(os.path.join(GOLDEN, "imitation.npz")) < 200 * 1024


@pytest.mark.parametrize("net,supervisor,motion", RUNS, ids=["-".join(r) for r in RUNS])
def test_fixture_commands_are_the_oracles(net, supervisor, motion):
    """Every stored supervisor command from the stored observation (and, for a stateful supervisor, its stored
    state before the call) through the oracle's controller, at tests/test_oracle.py's controller tolerances."""
    spec = next(s for s in META["supervisors"] if s["name"] == supervisor)
    key = f"{net}/{supervisor}/{motion}"
    obs, times, cmd = FX[f"{net}/{motion}/obs"], FX[f"{net}/{motion}/time"], FX[f"{key}/cmd"]
    assert cmd.shape == (4, len(META["stored"]), 4) and np.isfinite(cmd).all()
    assert FX[f"{key}/cmd_gap"].shape == (len(META["stored"]), 4) and FX[f"{key}/loss"].shape == (4,)
    cfg = dict(spec["config"])
    if spec["type"] != "riccati_lqr":
        cfg["controller"] = spec["type"]
    c, K, kc, fallback, _ = O.controller(cfg)
    assert not fallback and kc == {"pid": 3, "lqr": 6, "riccati": 6, "lqi": 9}[supervisor]
    state = FX[f"{key}/state"] if kc != 6 else None
    tol = 1e-9 if spec["type"] == "riccati_lqr" else 1e-12  # test_compute_action_sequences / test_pid_lqr_actions
    for e in range(4):
        for j, k in enumerate(META["stored"]):
            assert times[e, j] == pytest.approx(k * 0.01, abs=1e-12)
            o15 = np.concatenate([obs[e, j], np.zeros(3)])  # no feed-forward: the target acceleration is not read
            if kc == 3:
                u, st, _ = O.compute_action_pid(c, K, np.append(o15, times[e, j]), state[e, j])
            else:
                u, st, _ = O.compute_action(c, K, kc, o15, state[e, j, :3] if kc == 9 else np.zeros(3))
            np.testing.assert_allclose(u, cmd[e, j], rtol=tol, atol=tol, err_msg=f"{key} episode {e} step {k}")
            if kc != 6 and k < 9:  # steps 0-9 are consecutive: the state after this call is the stored next one
                rows = 4 if kc == 3 else 3
                np.testing.assert_allclose(st[:rows], state[e, j + 1, :rows], rtol=1e-12, atol=1e-14)
    if kc == 3:
        assert np.isnan(state[:, 0, 3]).all()  # a fresh PID has no last observation time
