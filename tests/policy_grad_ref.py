"""Helpers of the imitation-gradient tests (tests/test_policy_grad_cpu.py,
tests/test_gpu_policy_grad.py): the float64 reference of the loss and its
gradient, the yardstick and the rule both files hold a gradient to.

Reference g64: torch autograd in float64 on the CPU of
weight * F.mse_loss(sigmoid(net(f)) * scale + lo, t) for the f32 weights,
features and labels widened, scale = float32(hi - lo) and lo = float32(lo)
widened (the numbers the kernels and train_imitation use).

Yardstick gap: torch's own f32 CPU autograd of the same expression against
g64, one scalar per network and minibatch: the maximum over the parameter
tensors of max|g32 - g64| / max|g64| of that tensor.

Rule: for every parameter tensor max|g - g64| / max|g64| <= 4 x gap (the 4 x
gap rule of tests/policy_model.tol_of, taken network-wide); for the loss
|loss - loss64| <= max(4 |loss32 - loss64|, 2^-24 loss64).
"""

from __future__ import annotations

import functools

import numpy as np
import torch

import policy_model as M


ROW0 = 60  # the fixture's rows from here on are plain random ones (rows before: zeros and extreme values, at
# which the sigmoid saturates and a whole tensor's gradient underflows in f32, so that the gap is 1)


def sample_features(m: int) -> np.ndarray:
    """[m, 18] float32: the fixture's plain random feature rows ROW0.., repeated in a cycle beyond its end."""
    f = M.features()
    return np.ascontiguousarray(f[ROW0 + np.arange(m) % (len(f) - ROW0)])


def seeded_targets(net: M.Net, k: int, seed: int = 77) -> np.ndarray:
    """[k, 4] float32 labels, uniform in the net's output bounds."""
    lo, hi = net.lo_hi
    r = np.random.default_rng(seed).random((k, 4))
    return (lo[None] + r * (hi - lo)[None]).astype(np.float32)


def torch_gradient(net: M.Net, feats, targets, weight: float = 1.0, dtype=torch.float64):
    """(loss, [gradient per parameter tensor in parameters_to_vector order], commands [k, 4]) as float64 numpy."""
    seq = M.sequential(net, dtype)
    lo, hi = net.lo_hi
    scale = torch.from_numpy((hi - lo).astype(np.float32)).to(dtype)
    low = torch.from_numpy(lo.astype(np.float32)).to(dtype)
    f = torch.from_numpy(np.ascontiguousarray(feats, dtype=np.float32)).to(dtype)
    t = torch.from_numpy(np.ascontiguousarray(targets, dtype=np.float32)).to(dtype)
    u = torch.sigmoid(seq(f)) * scale + low
    loss = weight * torch.nn.functional.mse_loss(u, t)
    loss.backward()
    return (float(loss.detach().double()), [p.grad.double().numpy() for p in seq.parameters()],
            u.detach().double().numpy())


def rel_errors(g, g64) -> np.ndarray:
    """max|g - g64| / max|g64| per parameter tensor (0 / 0 = 0)."""
    out = []
    for a, b in zip(g, g64):
        num, den = float(np.abs(np.asarray(a, np.float64) - b).max()), float(np.abs(b).max())
        out.append(0.0 if num == 0.0 else (np.inf if den == 0.0 or not np.isfinite(num) else num / den))
    return np.array(out)


def split(flat, net: M.Net) -> list:
    """A flat gradient in parameters_to_vector order as the list of parameter tensors (unflatten's layout)."""
    flat = np.asarray(flat)
    dims = [18] + list(net.sizes) + [4]
    assert flat.shape == (sum(dims[i + 1] * dims[i] + dims[i + 1] for i in range(len(dims) - 1)),)
    out, off = [], 0
    for i in range(len(dims) - 1):
        o, k = dims[i + 1], dims[i]
        out += [flat[off:off + o * k].reshape(o, k), flat[off + o * k:off + o * k + o]]
        off += o * k + o
    return out


class Reference:
    """g64, the gap and the loss bound of one (net, features, labels, weight)."""

    def __init__(self, net, feats, targets, weight=1.0):
        old = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            self.loss64, self.g64, self.u64 = torch_gradient(net, feats, targets, weight, torch.float64)
            self.loss32, self.g32, _ = torch_gradient(net, feats, targets, weight, torch.float32)
        finally:
            torch.set_num_threads(old)
        self.net = net
        self.gap = float(rel_errors(self.g32, self.g64).max())
        self.loss_bound = max(4.0 * abs(self.loss32 - self.loss64), 2.0 ** -24 * abs(self.loss64))

    def fractions(self, g) -> np.ndarray:
        """Per parameter tensor, the error as a fraction of the rule's bound 4 x gap."""
        g = split(g, self.net) if isinstance(g, np.ndarray) and g.ndim == 1 else g
        return rel_errors(g, self.g64) / (4.0 * self.gap)

    def loss_fraction(self, loss) -> float:
        return abs(float(loss) - self.loss64) / self.loss_bound


@functools.lru_cache(maxsize=None)
def extra_net(activation: str, sizes: tuple, seed: int) -> M.Net:
    return M.Net(M.net_id(activation, sizes), list(sizes), activation, M.random_state_dict(list(sizes), seed))


def relu_manual_gradient(net: M.Net, feats, targets, weight: float = 1.0, slope_at_zero: float = 0.0):
    """A relu net's float64 gradient by hand, with a chosen derivative at a
    pre-activation of exactly 0: 0 is torch's; 1 is the mistake the rule must catch."""
    assert net.activation == "relu"
    lo, hi = net.lo_hi
    scale = (hi - lo).astype(np.float32).astype(np.float64)
    low = lo.astype(np.float32).astype(np.float64)
    layers = [(np.asarray(w, np.float64), np.asarray(b, np.float64)) for w, b in net.layers()]
    x = np.asarray(feats, np.float64)
    t = np.asarray(targets, np.float64)
    hs, zs = [x], []
    for w, b in layers[:-1]:
        z = hs[-1] @ w.T + b
        zs.append(z)
        hs.append(np.maximum(z, 0.0))
    raw = hs[-1] @ layers[-1][0].T + layers[-1][1]
    s = 1.0 / (1.0 + np.exp(-raw))
    u = s * scale + low
    delta = weight * 2.0 / u.size * (u - t) * scale * s * (1.0 - s)
    grads = []
    for i in range(len(layers) - 1, -1, -1):
        grads[:0] = [delta.T @ hs[i], delta.sum(axis=0)]
        if i > 0:
            z = zs[i - 1]
            delta = (delta @ layers[i][0]) * np.where(z > 0, 1.0, np.where(z == 0, slope_at_zero, 0.0))
    return grads
