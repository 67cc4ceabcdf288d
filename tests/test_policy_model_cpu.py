"""The deep-policy tests' own instruments, checked without a GPU
(tests/policy_model.py): the float64 restatement against the reference
fixture, the exact host model against that restatement, the power of the
summation-order probe, and the packing of every net of the architecture
matrix."""

import numpy as np
import pytest

import policy_model as M
from quadtrack.controllers import deep


# ------------------------------------------------------------ B1. the reference is the reference

@pytest.mark.parametrize("name", M.FIXTURE_IDS)
def test_float64_restatement_reproduces_fixture(name):
    """torch.nn.Sequential in float64 on the fixture's features gives the fixture's act64 (the reference's
    own PolicyNetwork in float64) within 1e-12: a float64 sum of at most 128 terms with sum |w h| <~ 100,
    the bound the suite uses for float64 sums."""
    assert np.array_equal(M.FX[f"{name}/features"], M.features())
    a64 = M.reference(name)[1]
    err = np.abs(a64 - M.FX[f"{name}/act64"])
    print(name, "max |restatement - fixture act64|", err.max())
    assert a64.shape == (512, 4) and (err <= 1e-12).all(), err.max()


# ------------------------------------------------------------ B2. the model against float64

@pytest.mark.parametrize("name", M.FIXTURE_EXACT_IDS + M.MATRIX_EXACT_IDS)
def test_model_against_float64(name):
    """The host model's commands (its logits, then f32 sigmoid, mul and add on the host) under the rule the
    device is held to (tests/test_gpu_policy.py): within max(4 x gap, 1e-5 + 1e-8 |ref|) of torch's f32
    commands, gap the per-component maximum of |torch f32 - torch float64| over the 512 rows."""
    net = M.any_net(name)
    a32, _, gap = M.reference(name)
    u = M.host_commands(net, M.model_logits(net, M.features()))
    err = np.abs(u - a32)
    print(name, "max |model - torch f32|", err.max(axis=0), "gap", gap, "ratio", err.max(axis=0) / np.maximum(gap, 1e-300))
    assert u.shape == (512, 4) and np.isfinite(u).all()
    assert (err <= M.tol_of(gap[None, :], a32)).all(), (err.max(axis=0), gap)


def test_model_rejects_what_it_does_not_restate():
    with pytest.raises(ValueError, match="relu and leaky_relu only"):
        M.model_logits(M.matrix_net("tanh-65"), M.features()[:1])


# ------------------------------------------------------------ B3. the order probe can tell the orders apart

@pytest.mark.parametrize("name", M.ORDER_PROBE_IDS)
def test_order_probe_has_power(name):
    """A condition of tests/test_gpu_policy_model.py's order probe, from the model alone: with every
    output bias -12 and bounds (0, 1), the documented order and plain index order give commands that differ
    by more than rule T2 allows in at least 10 % of the 4 k outputs.  So a device that sums a hidden layer
    in index order fails that test."""
    net = M.order_probe_net(name)
    f = M.features(M.ORDER_ROWS)
    y = M.model_logits(net, f, "documented")
    assert ((y >= -16.0) & (y < -8.0)).all(), (y.min(), y.max())
    u, tol = M.t2_tolerance(net, y)
    u_idx = M.exact_commands(net, M.model_logits(net, f, "index"))[1]
    d = np.abs(u_idx - u)
    over = d > tol
    print(name, "outputs over the tolerance", over.mean(), "smallest excess ratio",
          (d[over] / tol[over]).min() if over.any() else None, "logits", y.min(), y.max())
    assert over.mean() >= 0.10, over.mean()


# ------------------------------------------------------------ B4. packing of the matrix

@pytest.mark.parametrize("name,nt", list(zip(M.MATRIX_IDS, M.MATRIX_NT)))
def test_pack_params_layout_matrix(name, nt):
    net = M.matrix_net(name)
    assert deep.policy_tiles(net.sizes) == M.policy_tiles(net.sizes) == nt
    assert M.check_pack_layout(net.sd, net.sizes) == nt


def test_policy_tiles_at_the_tile_edges():
    for w, nt in ((1, 1), (32, 1), (33, 2), (64, 2), (65, 4), (96, 4), (97, 4), (128, 4)):
        assert deep.policy_tiles([w]) == nt, w
        assert deep.policy_tiles([1, w, 7]) == nt, w


def test_matrix_covers_every_variant():
    """Every activation at NT = 1, 2 and 4; one to four layers; widths at, one under and one over each
    tile edge; and the weights are the seeded recipe's (two builds agree bit for bit)."""
    nets = M.matrix_nets()
    assert len(nets) == 13
    assert {(n.activation, deep.policy_tiles(n.sizes)) for n in nets} == {(a, t) for a in M.ACTIVATIONS for t in (1, 2, 4)}
    assert {len(n.sizes) for n in nets} == {1, 2, 3, 4}
    widths = {w for n in nets for w in n.sizes}
    assert {1, 31, 32, 33, 64, 65, 96, 97, 127, 128} <= widths
    again = M.random_state_dict(nets[2].sizes, M.MATRIX_SEEDS[2])
    for k, v in nets[2].sd.items():
        assert v.dtype == again[k].dtype and np.array_equal(v.numpy(), again[k].numpy()), k
    b = np.concatenate([v.numpy().ravel() for k, v in nets[2].sd.items() if k.endswith("bias")])
    assert b.size == 96 + 96 + 4 and (np.abs(b) <= 0.1).all() and np.abs(b).max() > 0.05
