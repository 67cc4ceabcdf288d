"""Helpers of the deep-policy tests (tests/test_policy_model_cpu.py,
tests/test_gpu_policy_model.py): an exact host model of the f32 arithmetic that
csrc/qt_policy.hpp documents, the float64 reference of the same operation, and
the architecture matrix both test files share.

The host model is a small C++ program built with g++ -O2 -std=c++17
-ffp-contract=off (as tests/test_math.py builds its probes).  It restates the
header's documentation and includes nothing from csrc/: every accumulation is
std::fmaf on float, from the bias, over the padded width HP = 32 NT, in the
documented order (first layer inputs 0..17; hidden layers, per input tile of
32, columns crow(r, 0), crow(r, 1) for r = 0..15; output layer in index
order).  Only relu and leaky_relu are modelled: the device's tanh / expm1 are
not glibc's.  A compiled program because numpy cannot do an f32 fma exactly
(through float64 it rounds twice).  order="index" sums the hidden layers in
plain index order instead: the summation order a test must be able to tell
from the documented one.
"""

from __future__ import annotations

import atexit
import functools
import json
import os
import shutil
import subprocess
import tempfile
from dataclasses import dataclass, field

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FX = np.load(os.path.join(GOLDEN, "deep_policy.npz"))
META = json.loads(str(FX["meta_json"]))

KEYS = ("thrust", "roll_rate", "pitch_rate", "yaw_rate")
DEFAULT_BOUNDS = {"thrust": (0.0, 20.0), "roll_rate": (-3.0, 3.0), "pitch_rate": (-3.0, 3.0), "yaw_rate": (-3.0, 3.0)}
ACTIVATIONS = ("relu", "tanh", "elu", "leaky_relu")
EXACT = ("relu", "leaky_relu")  # the activations the host model restates exactly
ATOL, RTOL = 1e-5, 1e-8  # the floor of tests/test_gpu_policy.py's rule


def tol_of(gap, ref):
    """tests/test_gpu_policy.py's rule: 4 x the reference's own f32-vs-float64 gap, floor 1e-5 / 1e-8."""
    return np.maximum(4.0 * np.asarray(gap), ATOL + RTOL * np.abs(ref))


# --------------------------------------------------------------------- networks

@dataclass
class Net:
    name: str
    sizes: list
    activation: str
    sd: dict  # reference-format state dict: feature_extractor.{0,2,..}.{weight,bias}, output_layer.{weight,bias}
    bounds: dict | None = None  # None: the default output bounds
    extra: dict = field(default_factory=dict)

    @property
    def lo_hi(self):
        b = DEFAULT_BOUNDS if self.bounds is None else self.bounds
        return np.array([b[k][0] for k in KEYS], np.float64), np.array([b[k][1] for k in KEYS], np.float64)

    def layers(self):
        names = [f"feature_extractor.{2 * i}" for i in range(len(self.sizes))] + ["output_layer"]
        return [(self.sd[n + ".weight"], self.sd[n + ".bias"]) for n in names]


def policy_tiles(sizes) -> int:
    """NT as the header states it: 32-row tiles of the widest hidden layer, rounded up to 1, 2 or 4."""
    t = -(-max(sizes) // 32)
    return {1: 1, 2: 2, 3: 4, 4: 4}[t]


def random_state_dict(sizes, seed: int) -> dict:
    """tests/golden/gen_deep_policy.py's recipe without the reference: torch.manual_seed(seed), the Linear
    modules built in layer order (each draws its default initialisation), Xavier-uniform weights in the same
    order, then biases uniform in +-0.1 from a generator seeded seed + 1000, the output layer included."""
    torch.manual_seed(seed)
    dims = [18] + list(sizes) + [4]
    lin = [torch.nn.Linear(dims[i], dims[i + 1]) for i in range(len(dims) - 1)]
    g = torch.Generator().manual_seed(seed + 1000)
    sd = {}
    with torch.no_grad():
        for m in lin:
            torch.nn.init.xavier_uniform_(m.weight)
        for i, m in enumerate(lin):
            m.bias.copy_((torch.rand(m.bias.shape, generator=g) - 0.5) * 0.2)
            name = f"feature_extractor.{2 * i}" if i < len(sizes) else "output_layer"
            sd[name + ".weight"] = m.weight.detach().clone()
            sd[name + ".bias"] = m.bias.detach().clone()
    return sd


# activation x NT: widths of 1, one under, at and one over each tile edge, one to four layers, a narrow layer
# inside a wide net; [96, 96] and [65] take the branch that rounds three tiles up to four
MATRIX_SPECS = [
    ("relu", [1]), ("relu", [33, 64]), ("relu", [96, 96]), ("relu", [128, 128, 128, 128]),
    ("tanh", [31, 32]), ("tanh", [64, 1, 64]), ("tanh", [65]),
    ("elu", [32, 1, 32]), ("elu", [48, 64, 33, 40]), ("elu", [128, 7, 97]),
    ("leaky_relu", [17, 9, 32, 5]), ("leaky_relu", [33]), ("leaky_relu", [97, 128, 127, 65]),
]
MATRIX_NT = [1, 2, 4, 4, 1, 2, 4, 1, 2, 4, 1, 2, 4]
# Seeds 200 + i, but for two nets, chosen from the host model alone so that the order probe's conditions hold
# (test_policy_model_cpu.py::test_order_probe_has_power): relu [33, 64] at seed 201 has a probe logit of -7.46,
# outside [-16, -8); leaky_relu [17, 9, 32, 5] sums so few terms per neuron that the two orders differ in
# 4-8 % of the probe's outputs at most seeds (210: 7.7 %), seed 223 gives 10.2 %.
MATRIX_SEEDS = [200, 214, 202, 203, 204, 205, 206, 207, 208, 209, 223, 211, 212]
# wider than the env's action limits (thrust 0..20, rates +-3), so the env has to clip some commands
WIDE_BOUNDS = {"thrust": (-5.0, 30.0), "roll_rate": (-5.0, 5.0), "pitch_rate": (-5.0, 5.0), "yaw_rate": (-5.0, 5.0)}


def net_id(activation, sizes) -> str:
    return activation + "-" + "x".join(str(s) for s in sizes)


@functools.lru_cache(maxsize=None)
def matrix_nets() -> tuple:
    return tuple(Net(net_id(a, s), list(s), a, random_state_dict(s, seed))
                 for (a, s), seed in zip(MATRIX_SPECS, MATRIX_SEEDS))


MATRIX_IDS = [net_id(a, s) for a, s in MATRIX_SPECS]


def matrix_net(name) -> Net:
    return next(n for n in matrix_nets() if n.name == name)


def wide_bounds_net() -> Net:
    base = matrix_net("relu-96x96")
    return Net(base.name + "-wide", base.sizes, base.activation, base.sd, dict(WIDE_BOUNDS))


@functools.lru_cache(maxsize=None)
def fixture_net(name) -> Net:
    s = next(s for s in META["nets"] if s["name"] == name)
    pre = f"{name}/sd/"
    sd = {k[len(pre):]: torch.from_numpy(FX[k]) for k in FX.files if k.startswith(pre)}
    ob = {k: tuple(v) for k, v in s["output_bounds"].items()} if "output_bounds" in s else None
    return Net(name, list(s["hidden_sizes"]), s["activation"], sd, ob)


FIXTURE_IDS = [s["name"] for s in META["nets"]]
FIXTURE_EXACT_IDS = [s["name"] for s in META["nets"] if s["activation"] in EXACT]  # n0, n3, n4, n6, lqr
MATRIX_EXACT_IDS = [net_id(a, s) for a, s in MATRIX_SPECS if a in EXACT]


def any_net(name) -> Net:
    return fixture_net(name) if name in FIXTURE_IDS else matrix_net(name)


# the order probe: multi-layer relu / leaky_relu nets with random weights.  Single-hidden-layer nets have no
# hidden-layer sum, and the lqr net's second layer is an identity on 8 units (one nonzero term per sum), so
# neither has an order to tell apart.
ORDER_PROBE_IDS = [n for n in MATRIX_EXACT_IDS if "x" in n] + ["n0", "n3", "n6"]
ORDER_ROWS = slice(60, 316)  # fixture observations 60-315: the plain random rows


def order_probe_net(name) -> Net:
    """The same weights with every output bias -12 and bounds (0, 1): logits in [-16, -8), where the
    sigmoid is e^y to within 3.4e-4, so one ulp of a logit (2^-20 absolute in [-16, -8)) moves the command
    by 9.5e-7 relative."""
    base = any_net(name)
    sd = dict(base.sd)
    sd["output_layer.bias"] = torch.full((4,), -12.0)
    return Net(base.name + "-order", base.sizes, base.activation, sd, {k: (0.0, 1.0) for k in KEYS})


def features(rows=slice(None)) -> np.ndarray:
    """The fixture's f32 features [k, 18] (the same for every net)."""
    return np.ascontiguousarray(FX["n0/features"][rows], dtype=np.float32)


# --------------------------------------------------------------------- packing

def crow(r, half):
    return 8 * (r >> 2) + 4 * half + (r & 3)


def check_pack_layout(sd, sizes):
    """Every element of pack_params' block, read back through the layout the
    header documents, is the state dict's weight (or an exact zero of padding)."""
    import pytest

    from quadtrack import _abi
    from quadtrack.controllers import deep

    nh, nt = len(sizes), deep.policy_tiles(sizes)
    hp = 32 * nt
    blk = deep.pack_params(sd, sizes)
    assert blk.dtype == np.float32 and blk.size == _abi.policy_block_floats(nh, nt)
    names = deep.layer_names(nh)
    assert names[-1] == "output_layer" and names[0] == "feature_extractor.0"

    def padded(w, rows, cols):
        out = np.zeros((rows, cols), np.float32)
        out[:w.shape[0], :w.shape[1]] = w
        return out

    lane = np.arange(64)
    row, half = lane & 31, lane >> 5
    off = 0
    w0 = padded(sd[names[0] + ".weight"].numpy(), hp, 18)
    a0 = blk[off:off + nt * 9 * 64].reshape(nt, 9, 64)
    for mt in range(nt):
        for s in range(9):
            assert np.array_equal(a0[mt, s], w0[32 * mt + row, 2 * s + half])
    off += nt * 9 * 64
    b0 = sd[names[0] + ".bias"].numpy()
    assert np.array_equal(blk[off:off + sizes[0]], b0) and not blk[off + sizes[0]:off + hp].any()
    off += hp
    for i in range(1, nh):
        w = padded(sd[names[i] + ".weight"].numpy(), hp, hp)
        a = blk[off:off + nt * nt * 1024].reshape(nt, nt, 16, 64)
        for mt in range(nt):
            for kt in range(nt):
                for r in range(16):
                    cols = 32 * kt + np.where(half == 0, crow(r, 0), crow(r, 1))
                    assert np.array_equal(a[mt, kt, r], w[32 * mt + row, cols])
        off += nt * nt * 1024
        b = sd[names[i] + ".bias"].numpy()
        assert np.array_equal(blk[off:off + sizes[i]], b) and not blk[off + sizes[i]:off + hp].any()
        off += hp
    wo = padded(sd["output_layer.weight"].numpy(), 4, hp)
    assert np.array_equal(blk[off:off + 4 * hp].reshape(4, hp), wo)
    off += 4 * hp
    assert np.array_equal(blk[off:off + 4], sd["output_layer.bias"].numpy())
    assert off + 4 == blk.size
    # every real weight appears exactly once: the block's sum of squares is the state dict's
    total = sum(float((v.double() ** 2).sum()) for v in sd.values())
    assert float((blk.astype(np.float64) ** 2).sum()) == pytest.approx(total, rel=1e-12)
    return nt


# ------------------------------------------------------- float64 / f32 torch reference

def _module(name):
    return {"relu": torch.nn.ReLU, "tanh": torch.nn.Tanh, "elu": torch.nn.ELU,
            "leaky_relu": lambda: torch.nn.LeakyReLU(0.1)}[name]()


def sequential(net: Net, dtype) -> torch.nn.Sequential:
    """Linear + activation per hidden layer, Linear(., 4): the reference's PolicyNetwork without its bounds."""
    mods = []
    for i, (w, b) in enumerate(net.layers()):
        lin = torch.nn.Linear(w.shape[1], w.shape[0])
        with torch.no_grad():
            lin.weight.copy_(torch.as_tensor(w))
            lin.bias.copy_(torch.as_tensor(b))
        mods.append(lin)
        if i < len(net.sizes):
            mods.append(_module(net.activation))
    return torch.nn.Sequential(*mods).to(dtype)


def torch_actions(net: Net, feats: np.ndarray, dtype=torch.float64) -> np.ndarray:
    """sigmoid(raw) * (hi - lo) + lo of the f32 features in `dtype`, one row per call as the reference's
    compute_action evaluates it; returned as float64 [k, 4]."""
    seq = sequential(net, dtype)
    lo, hi = net.lo_hi
    lo_t, hi_t = torch.tensor(lo, dtype=dtype), torch.tensor(hi, dtype=dtype)
    out = np.empty((len(feats), 4), np.float64)
    f = torch.from_numpy(np.ascontiguousarray(feats, dtype=np.float32)).to(dtype)
    with torch.no_grad():
        for j in range(len(feats)):
            raw = seq(f[j:j + 1])
            out[j] = (torch.sigmoid(raw) * (hi_t - lo_t) + lo_t).squeeze(0).double().numpy()
    return out


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """(f32 actions, float64 actions, gap) of net `name` on the fixture's 512 rows, computed once: gap is the
    per-component maximum of |f32 - float64|, the input of tol_of."""
    net = wide_bounds_net() if name.endswith("-wide") else any_net(name)
    old = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        a32 = torch_actions(net, features(), torch.float32)
        a64 = torch_actions(net, features(), torch.float64)
    finally:
        torch.set_num_threads(old)
    for a in (a32, a64):
        a.setflags(write=False)
    gap = np.abs(a32 - a64).max(axis=0)
    gap.setflags(write=False)
    return a32, a64, gap


# --------------------------------------------------------------------- the host model

MODEL_SRC = r"""
// Exact f32 model of the deep policy's forward pass, from the documentation
// in csrc/qt_policy.hpp alone.  in: int32 {n_hidden, activation, order, k,
// width[4]}, then per layer weight [out][in] and bias [out] (f32), then
// features [k][18] (f32).  out: logits [k][4] (f32).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

static int crow(int r, int half) { return 8 * (r >> 2) + 4 * half + (r & 3); }

static float activate(int act, float x) {
  if (act == 0) return x < 0.0f ? 0.0f : x;  // relu
  return x > 0.0f ? x : x * 0.1f;            // leaky_relu
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hd[8];
  if (fread(hd, 4, 8, f) != 8) return 2;
  const int nh = hd[0], act = hd[1], order = hd[2], k = hd[3];
  if (nh < 1 || nh > 4 || (act != 0 && act != 3) || (order != 0 && order != 1) || k < 0) return 3;
  int wmax = 0;
  for (int i = 0; i < nh; ++i) {
    if (hd[4 + i] < 1 || hd[4 + i] > 128) return 3;
    wmax = hd[4 + i] > wmax ? hd[4 + i] : wmax;
  }
  const int t = (wmax + 31) / 32, nt = t == 3 ? 4 : t, hp = 32 * nt;
  // every layer zero-padded to hp rows and (after the first) hp columns
  std::vector<std::vector<float>> W(nh + 1), B(nh + 1);
  for (int L = 0; L <= nh; ++L) {
    const int in = L == 0 ? 18 : hd[4 + L - 1], out = L == nh ? 4 : hd[4 + L];
    const int inp = L == 0 ? 18 : hp, outp = L == nh ? 4 : hp;
    W[L].assign((size_t)outp * inp, 0.0f);
    B[L].assign(outp, 0.0f);
    for (int j = 0; j < out; ++j)
      if (fread(&W[L][(size_t)j * inp], 4, in, f) != (size_t)in) return 2;
    if (fread(B[L].data(), 4, out, f) != (size_t)out) return 2;
  }
  std::vector<float> x((size_t)k * 18), y((size_t)k * 4);
  if (fread(x.data(), 4, x.size(), f) != x.size()) return 2;
  fclose(f);
  // the order of a hidden layer's sum over its hp inputs
  std::vector<int> seq;
  for (int kt = 0; kt < nt; ++kt)
    for (int r = 0; r < 16; ++r)
      for (int half = 0; half < 2; ++half) seq.push_back(order == 0 ? 32 * kt + crow(r, half) : 32 * kt + 2 * r + half);
  std::vector<float> h(hp), g(hp);
  for (int e = 0; e < k; ++e) {
    const float* fe = &x[(size_t)e * 18];
    for (int j = 0; j < hp; ++j) {
      float acc = B[0][j];
      for (int i = 0; i < 18; ++i) acc = std::fmaf(W[0][(size_t)j * 18 + i], fe[i], acc);
      h[j] = activate(act, acc);
    }
    for (int L = 1; L < nh; ++L) {
      for (int j = 0; j < hp; ++j) {
        float acc = B[L][j];
        for (int c : seq) acc = std::fmaf(W[L][(size_t)j * hp + c], h[c], acc);
        g[j] = activate(act, acc);
      }
      h.swap(g);
    }
    for (int i = 0; i < 4; ++i) {
      float acc = B[nh][i];
      for (int c = 0; c < hp; ++c) acc = std::fmaf(W[nh][(size_t)i * hp + c], h[c], acc);
      y[(size_t)e * 4 + i] = acc;
    }
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o || fwrite(y.data(), 4, y.size(), o) != y.size()) return 2;
  fclose(o);
  return 0;
}
"""

ORDERS = ("documented", "index")
_dir = None


def _probe() -> str:
    global _dir
    if _dir is None:
        d = tempfile.mkdtemp(prefix="policy_model_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        with open(os.path.join(d, "model.cpp"), "w") as f:
            f.write(MODEL_SRC)
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(d, "model.cpp"),
                        "-o", os.path.join(d, "model")], check=True)
        _dir = d
    return _dir


def model_logits(net: Net, feats: np.ndarray, order: str = "documented") -> np.ndarray:
    """The four f32 logits [k, 4] of the host model (relu and leaky_relu nets only)."""
    if net.activation not in EXACT:
        raise ValueError(f"the host model restates relu and leaky_relu only, not {net.activation}")
    d = _probe()
    feats = np.ascontiguousarray(feats, dtype=np.float32)
    assert feats.ndim == 2 and feats.shape[1] == 18
    hd = np.zeros(8, np.int32)
    hd[:4] = len(net.sizes), ACTIVATIONS.index(net.activation), ORDERS.index(order), len(feats)
    hd[4:4 + len(net.sizes)] = net.sizes
    parts = [hd.tobytes()]
    for w, b in net.layers():
        parts += [np.ascontiguousarray(np.asarray(w), dtype=np.float32).tobytes(),
                  np.ascontiguousarray(np.asarray(b), dtype=np.float32).tobytes()]
    parts.append(feats.tobytes())
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(fin, "wb") as f:
        f.write(b"".join(parts))
    subprocess.run([os.path.join(d, "model"), fin, fout], check=True)
    return np.fromfile(fout, dtype=np.float32).reshape(len(feats), 4)


def host_commands(net: Net, logits: np.ndarray) -> np.ndarray:
    """f32 sigmoid, mul and add of the logits on the host (numpy float32), widened to float64."""
    lo, hi = net.lo_hi
    scale, lo32 = (hi - lo).astype(np.float32), lo.astype(np.float32)
    with np.errstate(over="ignore"):
        s = np.float32(1.0) / (np.float32(1.0) + np.exp(-logits.astype(np.float32)))
    return (s * scale[None, :] + lo32[None, :]).astype(np.float64)


def exact_commands(net: Net, logits: np.ndarray):
    """The output stage of the f32 logits in float64: (m*, u*, scale) with m* = sigmoid(y) scale, u* = m* + lo,
    scale = float32(hi - lo), lo = float32(lo)."""
    lo, hi = net.lo_hi
    scale = (hi - lo).astype(np.float32).astype(np.float64)
    lo32 = lo.astype(np.float32).astype(np.float64)
    with np.errstate(over="ignore"):
        m = scale[None, :] / (1.0 + np.exp(-logits.astype(np.float64)))
    return m, m + lo32[None, :], scale


def t2_tolerance(net: Net, logits: np.ndarray):
    """Rule T2 (tests/test_gpu_policy_model.py): returns (u*, tolerance)."""
    m, u, scale = exact_commands(net, logits)
    tol = 2.0 ** -24 * (5.0 * np.abs(m) + np.abs(u)) * (1.0 + 2.0 ** -10) + 2.0 ** -126 * scale[None, :]
    return u, tol
