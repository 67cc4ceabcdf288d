"""Policy populations, the parts that need no GPU: the flat-vector packing
index against pack_params, the container's and the search driver's argument
refusals, the C entry point's refusals before any launch, and the exports."""

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

import policy_model as M
import quadtrack
from quadtrack import _abi
from quadtrack.controllers import deep

HEADER = os.path.join(ROOT, "include", "quadtrack.h")
ENTRY_POINTS = ("qt_policy_population_version", "qt_policy_population_rollout")


def network(sizes, activation="relu", seed=0, bounds=None):
    torch.manual_seed(seed)
    cfg = {"hidden_sizes": list(sizes), "activation": activation}
    if bounds is not None:
        cfg["output_bounds"] = bounds
    pol = quadtrack.DeepTrackingPolicy(cfg, device="cpu")
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for p in pol.network.parameters():  # biases too: the default ones are zero
            p.copy_((torch.rand(p.shape, generator=g) - 0.5) * 0.8)
    return pol


# ------------------------------------------------------------------ packing

@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("spec", M.MATRIX_SPECS, ids=M.MATRIX_IDS)
def test_pack_index_gathers_pack_params(spec, seed):
    """A flat parameter vector gathered through pack_index is pack_params of the same state dict bit for
    bit, padding zeros included, and the inverse index returns the vector."""
    activation, sizes = spec
    pol = network(sizes, activation, seed)
    theta = torch.nn.utils.parameters_to_vector(pol.network.parameters()).detach()
    assert theta.dtype == torch.float32 and theta.numel() == deep.flat_size(sizes)
    idx = deep.pack_index(sizes)
    assert idx.dtype == np.int64 and idx.shape == (_abi.policy_block_floats(len(sizes), deep.policy_tiles(sizes)),)
    assert deep.pack_index(list(sizes)) is idx  # cached per shape
    src = np.concatenate([theta.numpy(), np.zeros(1, np.float32)])
    block = src[np.where(idx == deep.PAD, theta.numel(), idx)]
    want = deep.pack_params(pol.network.state_dict(), sizes)
    assert block.dtype == np.float32 and block.tobytes() == want.tobytes()
    assert not block[idx == deep.PAD].any()
    # every parameter exactly once
    real = idx[idx != deep.PAD]
    assert np.array_equal(np.sort(real), np.arange(theta.numel()))
    # flat(): the scatter index of the container, on the host
    scatter = np.empty(theta.numel(), np.int64)
    scatter[real] = np.flatnonzero(idx != deep.PAD)
    assert block[scatter].tobytes() == theta.numpy().tobytes()
    # the state dict of the flat vector is the network's
    sd = deep.unflatten(theta, sizes)
    for k, v in pol.network.state_dict().items():
        assert torch.equal(sd[k], v), k
    assert deep.population_stride(sizes) % 64 == 0 and deep.population_stride(sizes) >= idx.size


# ------------------------------------------------------------------ Python refusals

def test_population_refuses_mixed_members():
    a = network([8, 8], "relu", 0)
    with pytest.raises(ValueError, match="hidden sizes"):
        quadtrack.PolicyPopulation([a, network([8, 9], "relu", 1)])
    with pytest.raises(ValueError, match="hidden sizes"):
        quadtrack.PolicyPopulation([a, network([8], "relu", 1)])
    with pytest.raises(ValueError, match="activation"):
        quadtrack.PolicyPopulation([a, network([8, 8], "tanh", 1)])
    other = dict(deep.DEFAULT_OUTPUT_BOUNDS, thrust=(0.0, 25.0))
    with pytest.raises(ValueError, match="output bounds"):
        quadtrack.PolicyPopulation([a, network([8, 8], "relu", 1, bounds=other)])
    # state dicts: shape read from the weights, activation and bounds from the arguments
    with pytest.raises(ValueError, match="hidden sizes"):
        quadtrack.PolicyPopulation([a.network.state_dict(), network([8, 16], "relu", 1).network.state_dict()])
    with pytest.raises(ValueError, match="activation"):
        quadtrack.PolicyPopulation([a, a.network.state_dict()], activation="elu")
    with pytest.raises(ValueError, match="at least one"):
        quadtrack.PolicyPopulation([])
    with pytest.raises(TypeError):
        quadtrack.PolicyPopulation([a, 3])


def test_from_flat_refuses_wrong_theta():
    a = network([8, 8], "relu", 0)
    p = deep.flat_size([8, 8])
    assert p == 18 * 8 + 8 + 8 * 8 + 8 + 8 * 4 + 4
    for theta in (torch.zeros(3, p + 1), torch.zeros(3, p - 1), torch.zeros(p), torch.zeros(0, p),
                  torch.zeros(3, p, dtype=torch.float64)):
        with pytest.raises(ValueError, match="theta must be"):
            quadtrack.PolicyPopulation.from_flat(a, theta)
    with pytest.raises(ValueError, match="theta must be"):
        quadtrack.PolicyPopulation.from_flat({"hidden_sizes": [8, 8]}, torch.zeros(2, p + 3))
    with pytest.raises(ValueError, match="parameters"):
        deep.unflatten(torch.zeros(p + 1), [8, 8])


def test_search_policy_refuses_bad_arguments():
    cfg = {"hidden_sizes": [8]}
    for kw in ({"population": 7}, {"population": 0}, {"population": -2}, {"sigma": 0.0}, {"sigma": -0.1},
               {"sigma": float("nan")}, {"episodes_per_member": 0}, {"episodes_per_member": -3}):
        with pytest.raises(ValueError):
            quadtrack.search_policy(cfg, **kw)


# ------------------------------------------------------------------ C refusals

def test_c_entry_point_refuses_before_any_launch():
    """QT_EINVAL for every refusal the header lists (no GPU needed: nothing is launched)."""
    lib = _abi.load()
    dummy = C.c_float(0.0)
    block = _abi.policy_block_floats(2, 2)

    def population(n_hidden=2, widths=(64, 64), activation=0, params=True, members=3, stride=block, episodes=5):
        c = _abi.PolicyPopulation()
        c.shape.n_hidden = n_hidden
        for i, w in enumerate(widths):
            c.shape.width[i] = w
        c.shape.activation = activation
        c.shape.params = C.addressof(dummy) if params else None
        c.members, c.stride, c.episodes_per_member = members, stride, episodes
        return c

    env, crit = _abi.EnvParams(), _abi.Criteria()

    def rc(c, n=15, nsteps=0, order=False, null=False):
        b = _abi.Batch()
        b.n = n
        if order:
            b.order = C.addressof(dummy)
        return lib.qt_policy_population_rollout(C.byref(env), None if null else C.byref(c), C.byref(crit), C.byref(b),
                                                _abi.State(), nsteps, None, None)

    assert rc(population()) == 0  # valid, nsteps == 0: nothing to do
    assert rc(population(stride=block + 60)) == 0
    assert rc(population(), nsteps=3) == -1  # NULL state, refused before the launch
    assert rc(population(), null=True) == -1
    assert rc(population(params=False)) == -1
    assert rc(population(n_hidden=5, widths=(8, 8, 8, 8))) == -1
    assert rc(population(n_hidden=0)) == -1
    assert rc(population(widths=(64, 129))) == -1
    assert rc(population(widths=(0, 64))) == -1
    assert rc(population(activation=4)) == -1
    assert rc(population(activation=-1)) == -1
    assert rc(population(members=0), n=0) == -1
    assert rc(population(members=-1), n=-5) == -1
    assert rc(population(episodes=0), n=0) == -1
    assert rc(population(episodes=-5), n=-15) == -1
    assert rc(population(stride=block - 1)) == -1
    assert rc(population(stride=0)) == -1
    # the block size is that of the shape's own NT: a [64, 64] stride is too short for [128, 128]
    assert rc(population(widths=(128, 128))) == -1
    assert rc(population(widths=(128, 128), stride=_abi.policy_block_floats(2, 4))) == 0
    assert rc(population(), n=14) == -1
    assert rc(population(), n=16) == -1
    assert rc(population(), n=0) == -1
    assert rc(population(), order=True) == -1
    # a slot count whose grid does not fit an int: 2^31 - 1 members of 257 episodes (320 slots each)
    big = 2 ** 31 - 1
    assert rc(population(members=big, episodes=257), n=big * 257) == -1
    assert rc(population(members=big, episodes=64), n=big * 64) == 0  # 2^29 blocks: fits (nsteps == 0)
    assert rc(population(members=big, episodes=2 ** 62), n=0) == -1  # members * episodes overflows int64
    assert rc(population(), nsteps=-1) == -1


# ------------------------------------------------------------------ exports

def test_exports_and_versions():
    src = open(HEADER).read()
    declared = set(re.findall(r"^int (qt_\w+)\(", src, flags=re.M))
    lib = _abi.load()
    for name in ENTRY_POINTS:
        assert name in declared and name in _abi.EXPORTS and hasattr(lib, name), name
    assert "typedef struct qt_policy_population" in src
    assert lib.qt_policy_population_version() == _abi.POLICY_POPULATION_VERSION == 1
    assert lib.qt_policy_version() == 1 and lib.qt_abi_version() == 10  # additive
    for name in ("PolicyPopulation", "run_policy_population", "evaluate_population", "search_policy"):
        assert name in quadtrack.__all__ and hasattr(quadtrack, name), name
    from quadtrack import policy

    assert quadtrack.PolicyPopulation is policy.PolicyPopulation is deep.PolicyPopulation
    assert {"PolicyPopulation", "run_policy_population", "evaluate_population"} <= set(policy.__all__)
    assert quadtrack.search_policy is quadtrack.train.search_policy


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "quadtrack.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f));
int main(void) {
  printf("qt_policy_population %zu\n", sizeof(qt_policy_population));
  F(qt_policy_population, shape) F(qt_policy_population, members) F(qt_policy_population, stride)
  F(qt_policy_population, episodes_per_member)
  return 0;
}
"""


def test_ctypes_mirror_qt_policy_population(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    assert len(lines) == 5
    for line in lines:
        k, v = line.split()
        if "." in k:
            assert getattr(_abi.PolicyPopulation, k.split(".")[1]).offset == int(v), k
        else:
            assert C.sizeof(_abi.PolicyPopulation) == int(v)
