"""The imitation gradient's yardstick on the CPU (tests/policy_grad_ref.py):
the rule that tests/test_gpu_policy_grad.py holds the kernels to is wide
enough for a correct f32 gradient in another summation order and narrow enough
to catch a wrong one; and the flat layout the gradient is returned in."""

import dataclasses

import numpy as np
import pytest
import torch

import policy_grad_ref as R
import policy_model as M

SANITY_NETS = [("relu", (64, 64), 301), ("tanh", (32,), 302), ("elu", (128, 128), 303), ("relu", (64, 64, 64, 64), 304)]
PAD_WIDTHS = [1, 31, 33, 65, 97]


@pytest.mark.parametrize("m", [5, 64, 65, 256])
@pytest.mark.parametrize("spec", SANITY_NETS, ids=[M.net_id(a, s) for a, s, _ in SANITY_NETS])
def test_permuted_f32_gradient_is_inside_the_rule(spec, m):
    """torch's f32 gradient with the samples in another order: a correct gradient in another summation order."""
    net = R.extra_net(*spec)
    feats, targets = R.sample_features(m), R.seeded_targets(net, m)
    ref = R.Reference(net, feats, targets)
    perm = np.random.default_rng(m).permutation(m)
    loss_p, g_p, _ = R.torch_gradient(net, feats[perm], targets[perm], 1.0, torch.float32)
    frac = ref.fractions(g_p)
    print(f"{net.name} m={m}: gap {ref.gap:.3e}, permuted f32 at {frac.max():.3f} of the bound, "
          f"loss at {ref.loss_fraction(loss_p):.3f}")
    assert 1e-8 < ref.gap < 1e-5
    assert (frac <= 1.0).all(), frac  # (the loss of the permuted run is printed only: its bound can be the 2^-24 floor)


def _reference(m=64):
    net = R.extra_net("relu", (64, 64), 301)
    feats, targets = R.sample_features(m), R.seeded_targets(net, m)
    return net, feats, targets, R.Reference(net, feats, targets)


def test_transposed_weight_tensor_fails_the_rule():
    _, _, _, ref = _reference()
    g = [a.copy() for a in ref.g64]
    g[2] = np.ascontiguousarray(g[2].T)  # the [64, 64] hidden layer
    frac = ref.fractions(g)
    assert frac[2] > 1e3 and (np.delete(frac, 2) == 0).all(), frac


def test_shifted_bias_fails_the_rule():
    _, _, _, ref = _reference()
    for k in (1, 3, 5):
        g = [a.copy() for a in ref.g64]
        g[k] = np.roll(g[k], 1)
        assert ref.fractions(g)[k] > 1e3, k


def test_relu_derivative_of_one_at_zero_fails_the_rule():
    base = R.extra_net("relu", (64, 64), 301)
    sd = dict(base.sd)
    sd["feature_extractor.0.bias"] = torch.zeros(64)
    net = dataclasses.replace(base, name=base.name + "-zero-bias", sd=sd)
    feats = R.sample_features(8)
    feats[3] = 0.0  # every first-layer pre-activation of this sample is exactly 0
    targets = R.seeded_targets(net, 8)
    ref = R.Reference(net, feats, targets)
    right = R.relu_manual_gradient(net, feats, targets, slope_at_zero=0.0)
    wrong = R.relu_manual_gradient(net, feats, targets, slope_at_zero=1.0)
    assert (ref.fractions(right) <= 1.0).all(), ref.fractions(right)
    frac = ref.fractions(wrong)
    assert frac[1] > 1e3, frac  # the first layer's bias


@pytest.mark.parametrize("width", PAD_WIDTHS)
def test_flat_layout_round_trip(width):
    """flat_size / unflatten / pack_index: every parameter has one place in the packed block, padding has none."""
    from quadtrack.controllers import deep

    sizes = [width, width]
    P = deep.flat_size(sizes)
    assert P == 18 * width + width + width * width + width + 4 * width + 4
    theta = torch.from_numpy(np.random.default_rng(width).standard_normal(P).astype(np.float32))
    sd = deep.unflatten(theta, sizes)
    assert torch.equal(torch.cat([sd[f"{n}.{k}"].reshape(-1) for n in deep.layer_names(2) for k in ("weight", "bias")]),
                       theta)
    net = M.Net("flat", sizes, "relu", sd)
    for got, (w, b) in zip(np.split(np.arange(6), 3), net.layers()):
        parts = R.split(theta.numpy(), net)
        assert np.array_equal(parts[got[0]], w.numpy()) and np.array_equal(parts[got[1]], b.numpy())
    idx = deep.pack_index(sizes)
    real = idx != deep.PAD
    assert np.array_equal(np.sort(idx[real]), np.arange(P))
    block = deep.pack_params(sd, sizes)
    assert np.array_equal(block[real], theta.numpy()[idx[real]]) and not block[~real].any()
