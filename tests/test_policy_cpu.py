"""Deep tracking policy, the parts that need no GPU: the ABI additions, the
parameter-block packing, the checkpoint format, host feature extraction
against the reference fixture, and argument rejection."""

import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

import quadtrack
from quadtrack import _abi
from quadtrack.controllers import deep

from policy_model import check_pack_layout

HEADER = os.path.join(ROOT, "include", "quadtrack.h")
FX = np.load(os.path.join(GOLDEN, "deep_policy.npz"))
META = json.loads(str(FX["meta_json"]))
ENTRY_POINTS = ("qt_policy_version", "qt_policy_action", "qt_policy_rollout")


def state_dict_of(name):
    pre = f"{name}/sd/"
    return {k[len(pre):]: torch.from_numpy(FX[k]) for k in FX.files if k.startswith(pre)}


def spec_of(name):
    return next(s for s in META["nets"] if s["name"] == name)


def test_entry_points_declared_and_exported():
    src = open(HEADER).read()
    declared = set(re.findall(r"^int (qt_\w+)\(", src, flags=re.M))
    lib = _abi.load()
    for name in ENTRY_POINTS:
        assert name in declared and name in _abi.EXPORTS and hasattr(lib, name), name
    assert lib.qt_policy_version() == _abi.POLICY_VERSION == 1
    assert lib.qt_abi_version() == 10  # additive: the ABI version did not move
    for name in ("BatchedDeepPolicy", "DeepTrackingPolicy", "run_policy_loop", "evaluate_policy"):
        assert name in quadtrack.__all__ and hasattr(quadtrack, name), name
    from quadtrack import controllers

    assert "deep" not in controllers.VALID_CONTROLLER_TYPES
    assert {"BatchedDeepPolicy", "DeepTrackingPolicy"} <= set(controllers.__all__)


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "quadtrack.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f));
int main(void) {
  printf("qt_policy %zu\nqt_policy_obs %zu\n", sizeof(qt_policy), sizeof(qt_policy_obs));
  F(qt_policy, n_hidden) F(qt_policy, width) F(qt_policy, activation) F(qt_policy, params) F(qt_policy, lo)
  F(qt_policy, hi) F(qt_policy_obs, att) F(qt_policy_obs, rate) F(qt_policy_obs, tvel)
  printf("ACT %d %d %d %d\n", QT_ACT_RELU, QT_ACT_TANH, QT_ACT_ELU, QT_ACT_LEAKY_RELU);
  printf("LIMITS %d %d %d\n", QT_POLICY_MAX_HIDDEN, QT_POLICY_MAX_WIDTH, QT_POLICY_INPUTS);
  printf("BLOCK %lld %lld %lld\n", (long long)QT_POLICY_BLOCK_FLOATS(2, 2), (long long)QT_POLICY_BLOCK_FLOATS(1, 1),
         (long long)QT_POLICY_BLOCK_FLOATS(4, 4));
  return 0;
}
"""


def test_ctypes_mirror_qt_policy(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    cls = {"qt_policy": _abi.Policy, "qt_policy_obs": _abi.PolicyObs}
    for line in lines:
        k, *v = line.split()
        if k in cls:
            assert C.sizeof(cls[k]) == int(v[0]), k
        elif "." in k:
            s, f = k.split(".")
            assert getattr(cls[s], f).offset == int(v[0]), k
        elif k == "ACT":
            assert [int(x) for x in v] == list(range(len(_abi.ACTIVATIONS)))
            assert _abi.ACTIVATIONS == ("relu", "tanh", "elu", "leaky_relu")
        elif k == "LIMITS":
            assert [int(x) for x in v] == [_abi.POLICY_MAX_HIDDEN, _abi.POLICY_MAX_WIDTH, _abi.POLICY_INPUTS]
        elif k == "BLOCK":
            assert [int(x) for x in v] == [_abi.policy_block_floats(2, 2), _abi.policy_block_floats(1, 1),
                                           _abi.policy_block_floats(4, 4)]


@pytest.mark.parametrize("name", ["n0", "n3", "n4", "n5"])
def test_pack_params_layout(name):
    """Every element of the packed block, read back through the layout the
    header documents, is the state dict's weight (or an exact zero of padding)
    (the check itself: policy_model.check_pack_layout, shared with the
    architecture matrix of tests/test_policy_model_cpu.py)."""
    spec, sd = spec_of(name), state_dict_of(name)
    sizes = spec["hidden_sizes"]
    assert deep.policy_tiles(sizes) == {"n0": 2, "n3": 2, "n4": 1, "n5": 4}[name]
    check_pack_layout(sd, sizes)


def test_pack_params_rejects_wrong_shapes():
    sd = state_dict_of("n0")
    with pytest.raises(ValueError, match="expected weight"):
        deep.pack_params(sd, [64, 32])
    with pytest.raises(KeyError):
        deep.pack_params(sd, [64, 64, 64])


def test_xavier_init_matches_torch_generator():
    """torch.manual_seed gives the weights the reference network gets: the same
    modules built in the same order (every nn.Linear draws its default
    initialisation first), then Xavier-uniform weights and zero biases."""
    torch.manual_seed(7)
    pol = quadtrack.DeepTrackingPolicy({"hidden_sizes": [5, 3], "activation": "tanh"}, device="cpu")
    torch.manual_seed(7)
    lin = [torch.nn.Linear(18, 5), torch.nn.Linear(5, 3), torch.nn.Linear(3, 4)]
    for m in lin:
        torch.nn.init.xavier_uniform_(m.weight)
    sd = pol.network.state_dict()
    assert list(sd) == ["feature_extractor.0.weight", "feature_extractor.0.bias", "feature_extractor.2.weight",
                        "feature_extractor.2.bias", "output_layer.weight", "output_layer.bias"]
    for m, k in zip(lin, ("feature_extractor.0", "feature_extractor.2", "output_layer")):
        assert torch.equal(sd[k + ".weight"], m.weight) and not sd[k + ".bias"].any()


def test_checkpoint_round_trip_and_errors(tmp_path):
    spec, sd = spec_of("n3"), state_dict_of("n3")
    # a file as the reference's save_checkpoint writes it
    ref_file = tmp_path / "ref.pt"
    torch.save({"model_state_dict": sd, "config": {"hidden_sizes": spec["hidden_sizes"]}, "input_dim": 18,
                "hidden_sizes": spec["hidden_sizes"], "activation": spec["activation"],
                "output_bounds": dict(deep.DEFAULT_OUTPUT_BOUNDS), "metadata": {"epoch": 3}}, ref_file)
    cfg = {"hidden_sizes": spec["hidden_sizes"], "activation": spec["activation"]}
    pol = quadtrack.DeepTrackingPolicy(cfg, device="cpu")
    assert pol.load_checkpoint(ref_file) == {"epoch": 3}
    for k, v in pol.network.state_dict().items():
        assert torch.equal(v, sd[k]), k
    via_config = quadtrack.DeepTrackingPolicy({**cfg, "checkpoint_path": str(ref_file)}, device="cpu")
    assert torch.equal(via_config.network.state_dict()["output_layer.weight"], sd["output_layer.weight"])
    out = tmp_path / "sub" / "mine.pt"
    pol.save_checkpoint(out, metadata={"note": "x"})
    ck = torch.load(out, map_location="cpu", weights_only=False)
    assert set(ck) == {"model_state_dict", "config", "input_dim", "hidden_sizes", "activation", "output_bounds",
                       "metadata"}
    assert ck["input_dim"] == 18 and ck["hidden_sizes"] == spec["hidden_sizes"] and ck["activation"] == "leaky_relu"
    assert ck["output_bounds"]["thrust"] == (0.0, 20.0) and ck["metadata"] == {"note": "x"}
    assert list(ck["model_state_dict"]) == list(sd)
    pol.save_checkpoint(tmp_path / "plain.pt")
    assert "metadata" not in torch.load(tmp_path / "plain.pt", map_location="cpu", weights_only=False)
    assert quadtrack.DeepTrackingPolicy(cfg, device="cpu").load_checkpoint(tmp_path / "plain.pt") == {}
    # the reference's errors
    missing = tmp_path / "none.pt"
    with pytest.raises(FileNotFoundError, match=re.escape(f"Checkpoint not found: {missing}")):
        pol.load_checkpoint(missing)
    other = quadtrack.DeepTrackingPolicy({"hidden_sizes": [32, 32]}, device="cpu")
    with pytest.raises(ValueError, match=re.escape("Hidden sizes mismatch: checkpoint has [32, 64, 16], but network is "
                                                   "configured with [32, 32]. Cannot load incompatible model.")):
        other.load_checkpoint(ref_file)
    bad = dict(ck, input_dim=12)
    torch.save(bad, tmp_path / "bad.pt")
    with pytest.raises(ValueError, match=re.escape("Input dim mismatch: checkpoint has 12, network has 18")):
        pol.load_checkpoint(tmp_path / "bad.pt")


def test_host_features_equal_fixture_bitwise():
    obs = FX["obs"]
    want = FX["n0/features"]
    assert want.dtype == np.float32 and want.shape == (512, 18)
    for r, w in zip(obs, want):
        f = deep.extract_features({"quadcopter": {"position": r[0], "velocity": r[1], "attitude": r[2],
                                                  "angular_velocity": r[3]},
                                   "target": {"position": r[4], "velocity": r[5]}})
        assert f.dtype == np.float32 and f.tobytes() == w.tobytes()


def test_rejections():
    with pytest.raises(ValueError, match=re.escape("Unknown activation: gelu. Valid: ['relu', 'tanh', 'elu', 'leaky_relu']")):
        quadtrack.DeepTrackingPolicy({"activation": "gelu"}, device="cpu")
    with pytest.raises(ValueError, match="1..4 layers"):
        quadtrack.DeepTrackingPolicy({"hidden_sizes": [8] * 5}, device="cpu")
    with pytest.raises(ValueError, match="1..128"):
        quadtrack.DeepTrackingPolicy({"hidden_sizes": [64, 129]}, device="cpu")
    with pytest.raises(ValueError, match="1..128"):
        deep.validate_architecture([0], "relu")
    assert deep.validate_architecture([128, 128], "tanh") == [128, 128]
    assert deep.validate_architecture([64] * 4, "elu") == [64] * 4
    # a mixed-device call: observation tensors that are not on the policy's device
    z = torch.zeros(3, 3, dtype=torch.float64)
    obs = {"quadcopter": {"position": z, "velocity": z, "attitude": z, "angular_velocity": z},
           "target": {"position": z, "velocity": z}}
    with pytest.raises(ValueError, match="must be a float64"):
        deep.policy_obs_view(obs, 3, torch.device("cuda", 0))
    # the classical entry points still do not know the policy
    with pytest.raises(ValueError, match="Unknown controller type"):
        quadtrack.batched_controller("deep", {})
    with pytest.raises(NotImplementedError):
        quadtrack.load_controller("deep")


def test_c_entry_points_reject_invalid_policies():
    """QT_EINVAL before anything is launched (no GPU needed): sizes, activation, NULL params, order."""
    lib = _abi.load()
    dummy = C.c_float(0.0)

    def policy(n_hidden=2, widths=(64, 64), activation=0, params=True):
        p = _abi.Policy()
        p.n_hidden = n_hidden
        for i, w in enumerate(widths):
            p.width[i] = w
        p.activation = activation
        p.params = C.addressof(dummy) if params else None
        return p

    obs = _abi.PolicyObs()
    rc = lambda p, n=0: lib.qt_policy_action(C.byref(p), n, C.byref(obs), None, None, None)  # noqa: E731
    assert rc(policy()) == 0  # n == 0: nothing to do
    assert rc(policy(n_hidden=5, widths=(8, 8, 8, 8))) == -1
    assert rc(policy(n_hidden=0)) == -1
    assert rc(policy(widths=(64, 129))) == -1
    assert rc(policy(widths=(0, 64))) == -1
    assert rc(policy(activation=4)) == -1
    assert rc(policy(activation=-1)) == -1
    assert rc(policy(params=False)) == -1
    assert rc(policy(), n=-1) == -1
    assert rc(policy(), n=4) == -1  # NULL observation views and action
    env, crit, b = _abi.EnvParams(), _abi.Criteria(), _abi.Batch()
    roll = lambda p: lib.qt_policy_rollout(C.byref(env), C.byref(p), C.byref(crit), C.byref(b), _abi.State(), 3,  # noqa: E731
                                           None, None)
    assert roll(policy()) == 0  # n == 0
    assert roll(policy(widths=(64, 200))) == -1
    b.n = 4
    assert roll(policy()) == -1  # NULL state
    b.order = C.addressof(dummy)
    b.n = 0
    assert roll(policy()) == -1  # order must be NULL
