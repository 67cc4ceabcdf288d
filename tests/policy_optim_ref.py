"""Helpers of the optimiser-step tests (tests/test_policy_optim_cpu.py,
tests/test_gpu_policy_optim.py): the float64 reference of one clip + optimiser
step, the yardstick, the rule both files hold a step to, a numpy restatement
of the kernel's arithmetic with switchable mistakes, and the closed form of
the packed block's layout.

Reference x64: clip_grad_norm_ and torch.optim.{Adam, AdamW, SGD(momentum)} in
float64 on the CPU, one parameter tensor per layer tensor (unflatten's
layout), the f32 inputs (theta, m, v, g) widened; for step > 0 the state is
preloaded through optimizer.state.

Yardstick gap: the same run in torch float32 (one thread) against x64, per
quantity (dtheta = theta' - theta, m', v'): max|x32 - x64| / max|x64| over the
whole flat vector.

Rule: max|x - x64| / max|x64| <= 4 x gap per quantity (the 4 x gap rule of
tests/policy_model.tol_of); grad_norm within 2^-23 relative of the float64
norm (the f32 rounding of an FP64 sum of exact squares, 2^-24, plus the
square root's share of the sum's rounding; 2^-23 leaves a factor of two).
"""

from __future__ import annotations

import functools

import numpy as np
import torch

import policy_model as M

KINDS = ("adam", "adamw", "sgd")
BETAS, EPS, MOMENTUM = (0.9, 0.999), 1e-8, 0.9  # torch's defaults; the trainer's SGD momentum
LR = 1e-3
NORM_RTOL = 2.0 ** -23


def dims_of(sizes):
    return [18] + [int(h) for h in sizes] + [4]


def flat_size(sizes) -> int:
    d = dims_of(sizes)
    return sum(d[i + 1] * d[i] + d[i + 1] for i in range(len(d) - 1))


def split(flat, sizes) -> list:
    """A flat vector in parameters_to_vector order as the list of layer tensors (weight [out, in], bias)."""
    d, out, off = dims_of(sizes), [], 0
    for i in range(len(d) - 1):
        o, k = d[i + 1], d[i]
        out += [flat[off:off + o * k].reshape(o, k), flat[off + o * k:off + o * k + o]]
        off += o * k + o
    assert off == flat.shape[0]
    return out


def join(parts) -> np.ndarray:
    return np.concatenate([np.asarray(p.detach() if isinstance(p, torch.Tensor) else p).reshape(-1) for p in parts])


# --------------------------------------------------------------------- inputs

def trained_theta(sizes, seed=400) -> np.ndarray:
    """theta at random_state_dict's scale (Xavier-uniform weights, biases in +-0.1), float32."""
    sd = M.random_state_dict(list(sizes), seed)
    names = [f"feature_extractor.{2 * i}" for i in range(len(sizes))] + ["output_layer"]
    return join([sd[f"{n}.{k}"] for n in names for k in ("weight", "bias")]).astype(np.float32)


def small_theta(sizes, seed=401, lr=LR) -> np.ndarray:
    """|theta| <= lr with exact zeros: theta' is essentially fl(dtheta), so the rule measures the update."""
    r = np.random.default_rng(seed)
    th = r.uniform(-lr, lr, flat_size(sizes)).astype(np.float32)
    th[r.random(th.size) < 0.1] = 0.0
    return th


def seeded_gradient(sizes, seed) -> np.ndarray:
    """float32 gradient whose elements span four decades (1e-5 .. 1e-1 times a unit normal)."""
    r = np.random.default_rng(seed)
    n = flat_size(sizes)
    return (r.standard_normal(n) * 10.0 ** r.uniform(-5.0, -1.0, n)).astype(np.float32)


def seeded_state(sizes, seed):
    """(m, v) float32 of a run in progress: m a signed mean, v a positive mean of squares, of the gradient's scale."""
    r = np.random.default_rng(seed)
    n = flat_size(sizes)
    scale = 10.0 ** r.uniform(-5.0, -1.0, n)
    return (r.standard_normal(n) * scale).astype(np.float32), ((r.standard_normal(n) * scale) ** 2 + 1e-12).astype(np.float32)


# --------------------------------------------------------------------- torch reference

class TorchRun:
    """clip_grad_norm_ + a torch optimiser over steps, in one dtype on the CPU.

    per_tensor=True: one parameter per layer tensor (the trainer's layout);
    False: one flat parameter (the same model, for the round-trip test)."""

    def __init__(self, kind, sizes, theta, m, v, step, *, lr=LR, weight_decay=0.0, max_norm=0.0, dtype=torch.float64,
                 per_tensor=True):
        self.sizes, self.max_norm, self.kind = list(sizes), float(max_norm), kind
        cut = (lambda a: split(a, self.sizes)) if per_tensor else (lambda a: [a])
        self.cut = cut
        as_t = lambda a: torch.from_numpy(np.array(a, dtype=np.float32)).to(dtype)  # noqa: E731
        self.as_t = as_t
        self.params = [torch.nn.Parameter(t.clone()) for t in cut(as_t(theta))]
        if kind == "adam":
            self.opt = torch.optim.Adam(self.params, lr=lr, weight_decay=weight_decay)
        elif kind == "adamw":
            self.opt = torch.optim.AdamW(self.params, lr=lr, weight_decay=weight_decay)
        elif kind == "sgd":
            self.opt = torch.optim.SGD(self.params, lr=lr, weight_decay=weight_decay, momentum=MOMENTUM)
        else:
            raise ValueError(kind)
        if step > 0:
            ms, vs = cut(as_t(m)), (cut(as_t(v)) if kind != "sgd" else None)
            for i, p in enumerate(self.params):
                if kind == "sgd":
                    self.opt.state[p]["momentum_buffer"] = ms[i].clone()
                else:
                    self.opt.state[p].update(step=torch.tensor(float(step)), exp_avg=ms[i].clone(),
                                             exp_avg_sq=vs[i].clone())

    def step(self, g) -> float:
        """One update; returns the total norm before clipping (float)."""
        gs = self.cut(self.as_t(g))
        for p, gp in zip(self.params, gs):
            p.grad = gp.clone()
        if self.max_norm > 0.0:
            norm = torch.nn.utils.clip_grad_norm_(self.params, self.max_norm)
        else:
            norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(gp) for gp in gs]))
        self.opt.step()
        return float(norm)

    def result(self):
        """(theta', m', v') as float64 numpy flat vectors (v' None for SGD)."""
        key = "momentum_buffer" if self.kind == "sgd" else "exp_avg"
        th = join(self.params).astype(np.float64)
        m = join([self.opt.state[p][key] for p in self.params]).astype(np.float64)
        v = None if self.kind == "sgd" else join([self.opt.state[p]["exp_avg_sq"] for p in self.params]).astype(np.float64)
        return th, m, v


def rel_error(x, x64) -> float:
    """max|x - x64| / max|x64| over the flat vector (0 / 0 = 0)."""
    x = np.asarray(x, np.float64)
    if np.isnan(x).any():
        return np.inf
    num, den = float(np.abs(x - x64).max()), float(np.abs(x64).max())
    return 0.0 if num == 0.0 else (np.inf if den == 0.0 or not np.isfinite(num) else num / den)


class Reference:
    """x64, the gaps and the float64 norm of one case: `grads` is one gradient or a sequence of them."""

    def __init__(self, kind, sizes, theta, m, v, grads, step, **hyper):
        grads = [grads] if isinstance(grads, np.ndarray) and grads.ndim == 1 else list(grads)
        self.kind, self.theta = kind, np.asarray(theta, np.float64)
        old = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            runs = {}
            for dtype in (torch.float64, torch.float32):
                run = TorchRun(kind, sizes, theta, m, v, step, dtype=dtype, **hyper)
                norms = [run.step(g) for g in grads]
                runs[dtype] = (run.result(), norms)
        finally:
            torch.set_num_threads(old)
        (self.theta64, self.m64, self.v64), self.norms64 = runs[torch.float64]
        (self.theta32, self.m32, self.v32), self.norms32 = runs[torch.float32]
        self.x64 = self.quantities(self.theta64, self.m64, self.v64)
        x32 = self.quantities(self.theta32, self.m32, self.v32)
        self.gap = {k: rel_error(x32[k], self.x64[k]) for k in self.x64}

    def quantities(self, theta, m, v) -> dict:
        q = {"dtheta": np.asarray(theta, np.float64) - self.theta, "m": np.asarray(m, np.float64)}
        if self.kind != "sgd":
            q["v"] = np.asarray(v, np.float64)
        return q

    def fractions(self, theta, m, v) -> dict:
        """Per quantity, the error as a fraction of the rule's bound 4 x gap (0 / 0 = 0)."""
        out = {}
        for k, x in self.quantities(theta, m, v).items():
            err, bound = rel_error(x, self.x64[k]), 4.0 * self.gap[k]
            out[k] = 0.0 if err == 0.0 else (np.inf if bound == 0.0 else err / bound)
        return out

    def norm_fraction(self, norm, i=-1) -> float:
        return abs(float(norm) - self.norms64[i]) / (NORM_RTOL * self.norms64[i])


def norm64(g) -> float:
    return float(np.sqrt(np.sum(np.asarray(g, np.float64) ** 2)))


# --------------------------------------------------------------------- the kernel's arithmetic, restated

def clip_coef(norm, max_norm):
    """min(1, max_norm / (norm + 1e-6f)) in float32, as clip_grad_norm_ clamps it."""
    c = np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))
    return np.float32(1.0) if c > np.float32(1.0) else c


VARIANTS = ("no_bias_correction", "eps_inside_sqrt", "adamw_l2_decay", "adam_decoupled_decay", "momentum_ema",
            "clip_after_decay")


def model_step(kind, theta, m, v, g, step, *, lr=LR, weight_decay=0.0, max_norm=0.0, variant=None, dtype=np.float32):
    """One step as csrc/qt_policy_optim.hpp states it, every operation rounded to `dtype`; `variant` switches
    in one mistake the rule must catch.  Returns (theta', m', v' or None, norm)."""
    f = dtype
    th, g = np.asarray(theta, f).copy(), np.asarray(g, np.float32)
    norm = np.float32(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
    coef = f(clip_coef(norm, max_norm)) if max_norm > 0.0 else f(1.0)
    g = g.astype(f)
    wd = f(weight_decay)
    late_clip = variant == "clip_after_decay"
    if not late_clip:
        g = g * coef
    decoupled = (kind == "adamw") != (variant in ("adamw_l2_decay", "adam_decoupled_decay"))
    if kind != "sgd" and decoupled:
        th = th * f(1.0 - lr * weight_decay)
    elif weight_decay != 0.0:
        g = g + wd * th
    if late_clip:
        g = g * coef
    if kind == "sgd":
        mom = f(MOMENTUM)
        if variant == "momentum_ema":
            buf = (np.zeros_like(g) if step == 0 else np.asarray(m, f)) * mom + g * f(1.0 - MOMENTUM)
        else:
            buf = g.copy() if step == 0 else np.asarray(m, f) * mom + g
        return th + f(-lr) * buf, buf, None, norm
    b1, b2 = BETAS
    t = step + 1
    bc1, bc2 = (1.0, 1.0) if variant == "no_bias_correction" else (1.0 - b1 ** t, 1.0 - b2 ** t)
    m, v = np.asarray(m, f), np.asarray(v, f)
    m = m + f(1.0 - b1) * (g - m)
    v = v * f(b2) + (f(1.0 - b2) * g) * g
    if variant == "eps_inside_sqrt":
        den = np.sqrt(v / f(bc2) + f(EPS))
    else:
        den = np.sqrt(v) / f(np.sqrt(bc2)) + f(EPS)
    th = th + (f(-(lr / bc1)) * m) / den
    return th, m, v, norm


# --------------------------------------------------------------------- the packed block's layout

def block_source(sizes) -> np.ndarray:
    """int64 [QT_POLICY_BLOCK_FLOATS]: for every element of qt_policy.params its index in the flat parameter
    vector, -1 for padding; the closed form of the layout include/quadtrack.h documents:
      layer 0:       A[NT][9][64], A[mt][s][l] = W0[32 mt + (l & 31)][2 s + (l >> 5)]; bias[HP]
      layer 1..nh-1: A[NT][NT][16][64], A[mt][kt][r][l] = W[32 mt + (l & 31)][32 kt + 8 (r >> 2) + 4 (l >> 5) + (r & 3)]; bias[HP]
      output layer:  W[4][HP] row-major; bias[4]"""
    sizes = [int(h) for h in sizes]
    nh, nt = len(sizes), M.policy_tiles(sizes)
    hp, d = 32 * nt, dims_of(sizes)
    w_off, b_off, off = [], [], 0
    for i in range(nh + 1):
        w_off.append(off)
        b_off.append(off + d[i + 1] * d[i])
        off = b_off[-1] + d[i + 1]

    def weight(L, row, col):
        return np.where((row < d[L + 1]) & (col < d[L]), w_off[L] + row * d[L] + col, -1)

    def bias(L, n):
        i = np.arange(n)
        return np.where(i < d[L + 1], b_off[L] + i, -1)

    parts = []
    mt, s, l = np.meshgrid(np.arange(nt), np.arange(9), np.arange(64), indexing="ij")
    parts += [weight(0, 32 * mt + (l & 31), 2 * s + (l >> 5)).ravel(), bias(0, hp)]
    for L in range(1, nh):
        mt, kt, r, l = np.meshgrid(np.arange(nt), np.arange(nt), np.arange(16), np.arange(64), indexing="ij")
        parts += [weight(L, 32 * mt + (l & 31), 32 * kt + 8 * (r >> 2) + 4 * (l >> 5) + (r & 3)).ravel(), bias(L, hp)]
    i, k = np.meshgrid(np.arange(4), np.arange(hp), indexing="ij")
    parts += [weight(nh, i, k).ravel(), bias(nh, 4)]
    return np.concatenate(parts).astype(np.int64)


@functools.lru_cache(maxsize=None)
def case_inputs(sizes: tuple, family: str, step: int, seed: int = 0):
    """(theta, m, v, g) float32 of one single-step case (read-only: shared among the tests)."""
    theta = trained_theta(sizes) if family == "trained" else small_theta(sizes)
    g = seeded_gradient(sizes, 500 + seed + step)
    if step == 0:
        m, v = np.zeros_like(theta), np.zeros_like(theta)
    else:
        m, v = seeded_state(sizes, 600 + seed + step)
    for a in (theta, m, v, g):
        a.setflags(write=False)
    return theta, m, v, g
