"""Deep tracking policy — inference drop-in for the reference's
`controllers/deep_tracking_policy.py` on the HIP kernels of csrc/qt_policy.hip.

`DeepTrackingPolicy` mirrors the reference class for one episode;
`BatchedDeepPolicy` holds the weights as one f32 device block in the kernels'
operand order (`pack_params`, include/quadtrack.h `qt_policy`) and evaluates
n observations per launch (`qt_policy_action`) or runs the fused closed loop
(`qt_policy_rollout`, through `quadtrack.policy.run_policy_loop`).  Every
forward pass runs on the GPU in exact f32; there is no eager fallback.
"""

from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np
import torch

from .. import _abi
from .._abi import ACTIVATIONS, POLICY_INPUTS, POLICY_MAX_HIDDEN, POLICY_MAX_WIDTH, Policy, PolicyObs, check, on_device
from .._abi import raw_stream
from .base import BaseController

F64 = torch.float64

DEFAULT_OUTPUT_BOUNDS = {"thrust": (0.0, 20.0), "roll_rate": (-3.0, 3.0), "pitch_rate": (-3.0, 3.0),
                         "yaw_rate": (-3.0, 3.0)}
BOUND_KEYS = ("thrust", "roll_rate", "pitch_rate", "yaw_rate")


def validate_architecture(hidden_sizes, activation: str) -> list[int]:
    """The sizes the kernels accept: 1..4 hidden layers of 1..128 units, one of
    the reference's activations (PolicyNetwork._get_activation's message)."""
    if activation not in ACTIVATIONS:
        raise ValueError(f"Unknown activation: {activation}. Valid: {list(ACTIVATIONS)}")
    sizes = [int(h) for h in hidden_sizes]
    if not 1 <= len(sizes) <= POLICY_MAX_HIDDEN:
        raise ValueError(f"hidden_sizes must list 1..{POLICY_MAX_HIDDEN} layers, got {len(sizes)}")
    for h in sizes:
        if not 1 <= h <= POLICY_MAX_WIDTH:
            raise ValueError(f"hidden layer widths must be in 1..{POLICY_MAX_WIDTH}, got {h}")
    return sizes


def policy_tiles(hidden_sizes) -> int:
    """NT of the packed block: 32-row tiles of the widest layer, rounded up to 1, 2 or 4."""
    t = (max(hidden_sizes) + 31) // 32
    return 4 if t == 3 else t


def _crow(r: int, half: int) -> int:
    """Row of accumulator register r in lane half `half` of a 32x32 MFMA tile."""
    return 8 * (r >> 2) + 4 * half + (r & 3)


def layer_names(n_hidden: int) -> list[str]:
    """State-dict prefixes in layer order (the reference's Sequential puts an
    activation module after every Linear: indices 0, 2, 4, ...)."""
    return [f"feature_extractor.{2 * i}" for i in range(n_hidden)] + ["output_layer"]


def pack_params(state_dict, hidden_sizes) -> np.ndarray:
    """The qt_policy parameter block (float32, include/quadtrack.h) of a
    reference-format state dict: every layer's weight in the MFMA A-operand
    order of csrc/qt_policy.hpp, zero-padded to HP = 32 NT rows / columns."""
    sizes = [int(h) for h in hidden_sizes]
    nh, nt = len(sizes), policy_tiles(sizes)
    hp = 32 * nt
    W, B = [], []
    dims = [POLICY_INPUTS] + sizes + [4]
    for i, name in enumerate(layer_names(nh)):
        w = np.asarray(state_dict[f"{name}.weight"].detach().cpu() if isinstance(state_dict[f"{name}.weight"], torch.Tensor)
                       else state_dict[f"{name}.weight"], dtype=np.float32)
        b = np.asarray(state_dict[f"{name}.bias"].detach().cpu() if isinstance(state_dict[f"{name}.bias"], torch.Tensor)
                       else state_dict[f"{name}.bias"], dtype=np.float32)
        if w.shape != (dims[i + 1], dims[i]) or b.shape != (dims[i + 1],):
            raise ValueError(f"{name}: expected weight {(dims[i + 1], dims[i])} and bias {(dims[i + 1],)}, "
                             f"got {w.shape} and {b.shape}")
        W.append(w)
        B.append(b)
    lane = np.arange(64)
    row, half = lane & 31, lane >> 5
    parts = []
    # layer 0: A[mt][s][l] = W0[32 mt + (l & 31)][2 s + (l >> 5)]
    w0 = np.zeros((hp, POLICY_INPUTS), np.float32)
    w0[:sizes[0]] = W[0]
    a0 = np.empty((nt, 9, 64), np.float32)
    for mt in range(nt):
        for s in range(9):
            a0[mt, s] = w0[32 * mt + row, 2 * s + half]
    parts += [a0.ravel(), _padded(B[0], hp)]
    # hidden layers: A[mt][kt][r][l] = W[32 mt + (l & 31)][32 kt + crow(r, l >> 5)]
    for i in range(1, nh):
        w = np.zeros((hp, hp), np.float32)
        w[:sizes[i], :sizes[i - 1]] = W[i]
        a = np.empty((nt, nt, 16, 64), np.float32)
        for mt in range(nt):
            for kt in range(nt):
                for r in range(16):
                    a[mt, kt, r] = w[32 * mt + row, 32 * kt + _crow(r, 0) + 4 * half]
        parts += [a.ravel(), _padded(B[i], hp)]
    wo = np.zeros((4, hp), np.float32)
    wo[:, :sizes[-1]] = W[nh]
    parts += [wo.ravel(), B[nh]]
    block = np.concatenate(parts).astype(np.float32)
    assert block.size == _abi.policy_block_floats(nh, nt)
    return block


def _padded(v: np.ndarray, n: int) -> np.ndarray:
    out = np.zeros(n, np.float32)
    out[:v.size] = v
    return out


def extract_features(observation: dict) -> np.ndarray:
    """DeepTrackingPolicy._extract_features on the host (deep_tracking_policy.py:241-286):
    [target - quad position, target - quad velocity, attitude, angular
    velocity, target position, target velocity], float64 then float32.  The
    kernels form the same 18 numbers per episode; this is for callers that
    want to look at them."""
    quad, target = observation["quadcopter"], observation["target"]
    tp, tv = np.array(target["position"]), np.array(target["velocity"])
    return np.concatenate([tp - np.array(quad["position"]), tv - np.array(quad["velocity"]),
                           np.array(quad["attitude"]), np.array(quad["angular_velocity"]), tp, tv]).astype(np.float32)


def policy_obs_view(obs, n: int, device):
    """qt_policy_obs of an observation dict of [n, 3] float64 tensors on `device` (any strides)."""
    from ..step import tensor_view

    q, tg = obs["quadcopter"], obs["target"]
    v = PolicyObs()
    v.pos = tensor_view(q["position"], 3, n, "position", device)
    v.vel = tensor_view(q["velocity"], 3, n, "velocity", device)
    v.att = tensor_view(q["attitude"], 3, n, "attitude", device)
    v.rate = tensor_view(q["angular_velocity"], 3, n, "angular velocity", device)
    v.tpos = tensor_view(tg["position"], 3, n, "target position", device)
    v.tvel = tensor_view(tg["velocity"], 3, n, "target velocity", device)
    return v


def _bounds(output_bounds):
    ob = dict(DEFAULT_OUTPUT_BOUNDS if output_bounds is None else output_bounds)
    lo = [float(ob[k][0]) for k in BOUND_KEYS]
    hi = [float(ob[k][1]) for k in BOUND_KEYS]
    return ob, lo, hi


class BatchedDeepPolicy:
    """The policy for n episodes at once: weights in one f32 device block.

    compute_action(obs) -> [n, 4] float64 tensor (thrust, roll, pitch, yaw
    rate), usable with BatchedQuadcopterEnv.step; BatchedQuadcopterEnv.step_closed
    accepts the policy itself.  reset(n) is a no-op (a feed-forward network
    has no state)."""

    def __init__(self, state_dict, hidden_sizes=(64, 64), activation: str = "relu", output_bounds=None, device=None):
        self.hidden_sizes = validate_architecture(hidden_sizes, activation)
        block = pack_params(state_dict, self.hidden_sizes)
        self.device = _abi.require_gpu(device)
        self._bind(torch.as_tensor(block, device=self.device), activation, output_bounds)

    @classmethod
    def from_block(cls, block: torch.Tensor, hidden_sizes=(64, 64), activation: str = "relu", output_bounds=None):
        """From a packed f32 device block (pack_params' layout), which the policy keeps as it is."""
        self = cls.__new__(cls)
        self.hidden_sizes = validate_architecture(hidden_sizes, activation)
        want = _abi.policy_block_floats(len(self.hidden_sizes), policy_tiles(self.hidden_sizes))
        if block.dtype != torch.float32 or block.dim() != 1 or block.numel() != want or not block.is_contiguous():
            raise ValueError(f"the block must be a contiguous float32 [{want}] tensor")
        self.device = _abi.require_gpu(block.device)
        self._bind(block, activation, output_bounds)
        return self

    def _bind(self, block: torch.Tensor, activation: str, output_bounds) -> None:
        self.activation = activation
        self.output_bounds, lo, hi = _bounds(output_bounds)
        self.params = block
        p = Policy()
        p.n_hidden = len(self.hidden_sizes)
        for i, h in enumerate(self.hidden_sizes):
            p.width[i] = h
        p.activation = ACTIVATIONS.index(activation)
        p.params = self.params.data_ptr()
        for i in range(4):
            p.lo[i], p.hi[i] = lo[i], hi[i]
        self.c_policy = p
        self._ref = C.byref(p)
        lib = _abi.load()
        if lib.qt_policy_version() != _abi.POLICY_VERSION:
            raise ImportError("libquadtrack has another policy ABI than this package")

    @classmethod
    def from_state_dict(cls, state_dict, hidden_sizes=(64, 64), activation: str = "relu", output_bounds=None,
                        device=None) -> "BatchedDeepPolicy":
        return cls(state_dict, hidden_sizes, activation, output_bounds, device)

    @classmethod
    def from_checkpoint(cls, path, device=None) -> "BatchedDeepPolicy":
        """From a reference-format checkpoint file (DeepTrackingPolicy.save_checkpoint)."""
        ck = load_checkpoint_file(path)
        return cls(ck["model_state_dict"], ck["hidden_sizes"], ck.get("activation", "relu"), ck.get("output_bounds"),
                   device)

    def reset(self, n: int | None = None) -> None:
        pass

    def compute_action(self, obs, frozen: torch.Tensor | None = None) -> torch.Tensor:
        """Actions [n, 4] for an observation dict of [n, 3] float64 tensors on
        the policy's device (BatchedQuadcopterEnv's observation, or any
        strides).  frozen: optional [n] int8 / bool tensor; its nonzero
        episodes get a zero action row."""
        n = obs["quadcopter"]["position"].shape[0]
        v = policy_obs_view(obs, n, self.device)
        if frozen is not None and (frozen.device != self.device or frozen.numel() != n or frozen.element_size() != 1
                                   or not frozen.is_contiguous()):
            raise ValueError(f"frozen must be a contiguous one-byte [{n}] tensor on {self.device}")
        out = torch.empty(4, n, dtype=F64, device=self.device)
        with on_device(self.device):
            check(_abi.load().qt_policy_action(self._ref, n, C.byref(v), None if frozen is None else frozen.data_ptr(),
                                               out.data_ptr(), raw_stream(self.device)), "qt_policy_action")
        return out.T

    def rollout(self, env, crit, batch, st, nsteps: int, rec: torch.Tensor | None = None) -> None:
        """qt_policy_rollout on a core.EpisodeBatch / core.RolloutState (in place; chunks allowed)."""
        if batch.order is not None:
            raise ValueError("the policy rollout runs episodes in index order (order must be None)")
        if batch.device != self.device:
            raise ValueError(f"the batch is on {batch.device}, the policy on {self.device}")
        if rec is not None and (rec.numel() < nsteps * 16 * batch.n or rec.dtype != F64 or not rec.is_contiguous()):
            raise ValueError("rec must hold nsteps * 16 * n contiguous float64")
        with torch.cuda.device(self.device):
            check(_abi.load().qt_policy_rollout(C.byref(env), self._ref, C.byref(crit),
                                                C.byref(batch.c_batch(with_k=False)), st.c_state(), int(nsteps),
                                                _abi.ptr(rec), _abi.stream_of(self.device)), "qt_policy_rollout")

    def rollout_supervised(self, env, ctrl, crit, batch, st, nsteps: int, loss: torch.Tensor,
                           sample_steps: torch.Tensor | None = None, sample: torch.Tensor | None = None,
                           rec: torch.Tensor | None = None, teacher_rec: torch.Tensor | None = None) -> None:
        """qt_policy_supervised_rollout (in place; chunks allowed): the policy
        flies, the classical teacher of `batch`'s gains and `ctrl` labels every
        visited state.

        loss          [n] float64, accumulated: sum of squared (policy - f32 teacher) command differences
        sample_steps  [S, n] int32, strictly ascending per episode (or None: no samples)
        sample        [S, 26, n] float32, written where an episode reaches its slot's step
        rec           [nsteps, 16, n] float64 as rollout's
        teacher_rec   [nsteps, 4, n] float64: the teacher's command of this launch's steps"""
        if batch.order is not None:
            raise ValueError("the policy rollout runs episodes in index order (order must be None)")
        if batch.device != self.device:
            raise ValueError(f"the batch is on {batch.device}, the policy on {self.device}")
        n = batch.n

        def want(t, name, numel, dtype):
            if t.device != self.device or t.dtype != dtype or t.numel() < numel or not t.is_contiguous():
                raise ValueError(f"{name} must hold {numel} contiguous {dtype} values on {self.device}")

        want(loss, "loss", n, F64)
        if rec is not None:
            want(rec, "rec", nsteps * 16 * n, F64)
        if teacher_rec is not None:
            want(teacher_rec, "teacher_rec", nsteps * 4 * n, F64)
        sup = _abi.PolicySupervision()
        if (sample_steps is None) != (sample is None):
            raise ValueError("sample_steps and sample go together")
        if sample_steps is not None:
            if sample_steps.dim() != 2 or sample_steps.shape[1] != n:
                raise ValueError(f"sample_steps must be [S, {n}]")
            S = sample_steps.shape[0]
            want(sample_steps, "sample_steps", S * n, torch.int32)
            want(sample, "sample", S * _abi.SUP_ROWS * n, torch.float32)
            if S:
                sup.samples, sup.sample_steps, sup.sample = S, sample_steps.data_ptr(), sample.data_ptr()
        sup.loss = loss.data_ptr()
        sup.teacher_rec = None if teacher_rec is None else teacher_rec.data_ptr()
        lib = _abi.load()
        if not _abi.has_policy_supervised():
            raise ImportError("libquadtrack has another supervised-rollout ABI than this package")
        with torch.cuda.device(self.device):
            check(lib.qt_policy_supervised_rollout(C.byref(env), C.byref(ctrl), self._ref, C.byref(crit),
                                                   C.byref(batch.c_batch()), st.c_state(), int(nsteps), C.byref(sup),
                                                   _abi.ptr(rec), _abi.stream_of(self.device)),
                  "qt_policy_supervised_rollout")

    def imitation_gradient(self, features: torch.Tensor, targets: torch.Tensor, index: torch.Tensor | None = None,
                           weight: float = 1.0, *, grad: torch.Tensor | None = None,
                           pred: torch.Tensor | None = None):
        """qt_policy_imitation_grad: the imitation loss
        weight * F.mse_loss(network(features), targets) of a minibatch and its
        gradient with respect to every weight and bias, on the forward pass's
        MFMA path (csrc/qt_policy_grad.hpp).

        features  [rows, 18] float32, contiguous, on the policy's device
        targets   [rows, 4] float32, contiguous
        index     None: the samples are rows 0..m-1 with m = rows; or an [m]
                  int64 tensor of row numbers (not checked: a row number
                  outside [0, rows) is the caller's error)
        grad      optional [flat_size] float32 output (parameters_to_vector order)
        pred      optional [m, 4] float32 output: the forward commands, bit for
                  bit compute_action's for observations with those features
        Returns (loss [1] float64, grad [flat_size] float32), both on the
        device; no host synchronisation.  The workspace is cached per m."""
        dev = self.device

        def want(t, name, shape, dtype):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
            if t.device != dev:
                raise ValueError(f"{name} is on {t.device}, the policy on {dev}")
            if t.dtype != dtype:
                raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"{name} must have shape {list(shape)}, got {list(t.shape)}")
            if not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous")

        if not isinstance(features, torch.Tensor) or features.dim() != 2:
            raise ValueError(f"features must be a [rows, {POLICY_INPUTS}] tensor")
        rows = features.shape[0]
        want(features, "features", (rows, POLICY_INPUTS), torch.float32)
        want(targets, "targets", (rows, 4), torch.float32)
        if index is None:
            m = rows
        else:
            if not isinstance(index, torch.Tensor) or index.dim() != 1:
                raise ValueError("index must be a one-dimensional int64 tensor")
            m = index.shape[0]
            want(index, "index", (m,), torch.int64)
        if m < 1 or rows < 1:
            raise ValueError("the gradient needs at least one sample")
        weight = float(weight)
        if not np.isfinite(weight):
            raise ValueError(f"weight must be finite, got {weight}")
        size = flat_size(self.hidden_sizes)
        if grad is None:
            grad = torch.empty(size, dtype=torch.float32, device=dev)
        else:
            want(grad, "grad", (size,), torch.float32)
        if pred is not None:
            want(pred, "pred", (m, 4), torch.float32)
        lib = _abi.load()
        if not _abi.has_policy_grad():
            raise ImportError("libquadtrack has another imitation-gradient ABI than this package")
        cache = self.__dict__.setdefault("_grad_workspace", {})
        ws = cache.get(m)
        if ws is None:
            nbytes = lib.qt_policy_grad_workspace(self._ref, m)
            if nbytes < 0:
                raise ValueError(f"no gradient workspace for {m} samples of this policy")
            ws = cache[m] = torch.empty((nbytes + 7) // 8, dtype=F64, device=dev)
        loss = torch.empty(1, dtype=F64, device=dev)
        io = _abi.PolicyGradIO()
        io.features, io.targets = features.data_ptr(), targets.data_ptr()
        io.index = None if index is None else index.data_ptr()
        io.rows, io.m, io.weight = rows, m, weight
        io.grad, io.loss = grad.data_ptr(), loss.data_ptr()
        io.pred = None if pred is None else pred.data_ptr()
        io.workspace, io.workspace_bytes = ws.data_ptr(), ws.numel() * 8
        with on_device(dev):
            check(lib.qt_policy_imitation_grad(self._ref, C.byref(io), raw_stream(dev)), "qt_policy_imitation_grad")
        return loss, grad


def load_checkpoint_file(path) -> dict:
    path = Path(path)
    if not path.exists():
        raise FileNotFoundError(f"Checkpoint not found: {path}")
    # weights_only=False: the reference's checkpoints carry config and metadata dicts
    return torch.load(path, map_location="cpu", weights_only=False)


def _activation_module(name: str) -> torch.nn.Module:
    return {"relu": torch.nn.ReLU, "tanh": torch.nn.Tanh, "elu": torch.nn.ELU,
            "leaky_relu": lambda: torch.nn.LeakyReLU(0.1)}[name]()


class _Weights(torch.nn.Module):
    """The reference network's parameter container (same module names, same
    construction order, so torch.manual_seed gives the reference's weights and
    state dicts interchange).  It only holds weights: inference runs in the
    HIP kernels."""

    def __init__(self, hidden_sizes, activation):
        super().__init__()
        layers, prev = [], POLICY_INPUTS
        for h in hidden_sizes:
            layers += [torch.nn.Linear(prev, h), _activation_module(activation)]
            prev = h
        self.feature_extractor = torch.nn.Sequential(*layers)
        self.output_layer = torch.nn.Linear(prev, 4)
        for m in self.modules():  # Xavier-uniform weights, zero biases (deep_tracking_policy.py:106-112)
            if isinstance(m, torch.nn.Linear):
                torch.nn.init.xavier_uniform_(m.weight)
                torch.nn.init.zeros_(m.bias)
        self.input_dim = POLICY_INPUTS
        self.hidden_sizes = list(hidden_sizes)
        self.activation_name = activation


class DeepTrackingPolicy(BaseController):
    """Drop-in for the reference's DeepTrackingPolicy (inference).

    config keys: hidden_sizes (default [64, 64]), activation ("relu", "tanh",
    "elu", "leaky_relu"), output_bounds, checkpoint_path.  Weights are
    Xavier-uniform with zero biases from torch's generator (torch.manual_seed
    gives the reference's weights) or come from a reference-format checkpoint.
    compute_action runs the network on the GPU (qt_policy_action with n = 1).

    Training: quadtrack.train.train_imitation fits self.network to a classical
    supervisor's commands (the reference trainer's imitation mode) on the
    supervised rollout, with torch autograd or the HIP backward pass
    (backend="hip", BatchedDeepPolicy.imitation_gradient; backend="hip_fused":
    the clip, the optimiser step and the packing on the device too,
    PolicyOptimizer), and leaves the weights here;
    quadtrack.train.search_policy is the gradient-free search.  Weights may
    also come from the reference's trainer through a checkpoint.

    Out of scope: to_onnx, train_mode, get_parameters, and the trainer's other
    modes (tracking / reward_weighted losses, curriculum, diagnostics)."""

    def __init__(self, config: dict | None = None, device: str | None = None):
        super().__init__(name="deep_tracking", config=config)
        config = config or {}
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        hidden_sizes = config.get("hidden_sizes", [64, 64])
        activation = config.get("activation", "relu")
        validate_architecture(hidden_sizes, activation)
        self.network = _Weights(list(hidden_sizes), activation)
        self.network.output_bounds = _bounds(config.get("output_bounds"))[0]
        self._batched: BatchedDeepPolicy | None = None
        if config.get("checkpoint_path") is not None:
            self.load_checkpoint(config["checkpoint_path"])

    def to_batched(self, device=None) -> BatchedDeepPolicy:
        """The same weights as a BatchedDeepPolicy (a snapshot)."""
        net = self.network
        return BatchedDeepPolicy(net.state_dict(), net.hidden_sizes, net.activation_name, net.output_bounds,
                                 device if device is not None else (self.device if self.device.type == "cuda" else None))

    def compute_action(self, observation: dict) -> dict:
        if self._batched is None:
            self._batched = self.to_batched()
        b = self._batched
        row = lambda v: torch.as_tensor(np.asarray(v, dtype=np.float64).reshape(1, 3), device=b.device)  # noqa: E731
        quad, target = observation["quadcopter"], observation["target"]
        obs = {"quadcopter": {k: row(quad[k]) for k in ("position", "velocity", "attitude", "angular_velocity")},
               "target": {k: row(target[k]) for k in ("position", "velocity")}}
        a = b.compute_action(obs)[0].cpu().numpy()
        return {"thrust": float(a[0]), "roll_rate": float(a[1]), "pitch_rate": float(a[2]), "yaw_rate": float(a[3])}

    def reset(self) -> None:
        pass

    def save_checkpoint(self, path, metadata: dict | None = None) -> None:
        """The reference's checkpoint file (deep_tracking_policy.py:304-332)."""
        path = Path(path)
        path.parent.mkdir(parents=True, exist_ok=True)
        net = self.network
        checkpoint = {"model_state_dict": net.state_dict(), "config": self.config, "input_dim": net.input_dim,
                      "hidden_sizes": net.hidden_sizes, "activation": net.activation_name,
                      "output_bounds": net.output_bounds}
        if metadata:
            checkpoint["metadata"] = metadata
        torch.save(checkpoint, path)

    def load_checkpoint(self, path) -> dict:
        """Load a reference-format checkpoint; returns its metadata
        (deep_tracking_policy.py:334-373, the same errors)."""
        checkpoint = load_checkpoint_file(path)
        net = self.network
        if checkpoint.get("input_dim") != net.input_dim:
            raise ValueError(f"Input dim mismatch: checkpoint has {checkpoint.get('input_dim')}, "
                             f"network has {net.input_dim}")
        if checkpoint.get("hidden_sizes") != net.hidden_sizes:
            raise ValueError(f"Hidden sizes mismatch: checkpoint has "
                             f"{checkpoint.get('hidden_sizes')}, but network is configured "
                             f"with {net.hidden_sizes}. Cannot load incompatible model.")
        net.load_state_dict(checkpoint["model_state_dict"])
        self._batched = None
        return checkpoint.get("metadata", {})


# ------------------------------------------------------------------ populations

PAD = -1  # pack_index's marker of a padding zero


def flat_size(hidden_sizes) -> int:
    """Parameters of the network: the length of parameters_to_vector(network.parameters())."""
    dims = [POLICY_INPUTS] + [int(h) for h in hidden_sizes] + [4]
    return sum(dims[i + 1] * dims[i] + dims[i + 1] for i in range(len(dims) - 1))


def unflatten(theta, hidden_sizes) -> dict:
    """The reference-format state dict of a flat parameter vector in
    parameters_to_vector(network.parameters()) order: per layer the weight
    [out][in] row-major, then the bias."""
    sizes = [int(h) for h in hidden_sizes]
    theta = torch.as_tensor(theta).detach().reshape(-1)
    if theta.numel() != flat_size(sizes):
        raise ValueError(f"a {sizes} network has {flat_size(sizes)} parameters, got {theta.numel()}")
    dims = [POLICY_INPUTS] + sizes + [4]
    sd, off = {}, 0
    for i, name in enumerate(layer_names(len(sizes))):
        o, k = dims[i + 1], dims[i]
        sd[f"{name}.weight"] = theta[off:off + o * k].reshape(o, k)
        sd[f"{name}.bias"] = theta[off + o * k:off + o * k + o]
        off += o * k + o
    return sd


_PACK_INDEX: dict = {}


def pack_index(hidden_sizes) -> np.ndarray:
    """int64 [QT_POLICY_BLOCK_FLOATS]: element i of the packed block is element
    pack_index[i] of the flat parameter vector, or an exact zero of padding
    where pack_index[i] == PAD.  Built once per shape by sending every
    parameter's own position through pack_params (positions are far below 2^24,
    so float32 carries them exactly), and cached (read-only)."""
    key = tuple(int(h) for h in hidden_sizes)
    if key not in _PACK_INDEX:
        sizes = validate_architecture(key, "relu")
        tagged = unflatten(torch.arange(1, flat_size(sizes) + 1, dtype=torch.float32), sizes)
        idx = pack_params(tagged, sizes).astype(np.int64) - 1
        idx.setflags(write=False)
        _PACK_INDEX[key] = idx
    return _PACK_INDEX[key]


def population_stride(hidden_sizes) -> int:
    """Floats between two members' blocks: the block rounded up to 256 bytes,
    so every member's A-operand rows start on the alignment member 0's have."""
    nb = _abi.policy_block_floats(len(hidden_sizes), policy_tiles(hidden_sizes))
    return (nb + 63) // 64 * 64


def _member_spec(m, activation, output_bounds):
    """(weights, hidden_sizes, activation, output_bounds) of one member given
    as a policy or a state dict; weights: a state dict or a packed device block."""
    if isinstance(m, DeepTrackingPolicy):
        net = m.network
        return net.state_dict(), list(net.hidden_sizes), net.activation_name, _bounds(net.output_bounds)[0]
    if isinstance(m, BatchedDeepPolicy):
        return m.params, list(m.hidden_sizes), m.activation, m.output_bounds
    if isinstance(m, dict):
        nh = len([k for k in m if k.startswith("feature_extractor.") and k.endswith(".weight")])
        sizes = [int(m[f"feature_extractor.{2 * i}.weight"].shape[0]) for i in range(nh)]
        return m, sizes, activation, _bounds(output_bounds)[0]
    raise TypeError(f"a population member is a DeepTrackingPolicy, a BatchedDeepPolicy or a state dict, "
                    f"not {type(m).__name__}")


class PolicyPopulation:
    """M networks of one shape as one [M, stride] f32 device tensor of packed
    blocks (qt_policy_population): the fused rollout runs every member on its
    own episodes in one launch (quadtrack.policy.run_policy_population).

    members   DeepTrackingPolicy / BatchedDeepPolicy / reference-format state
              dicts; one shape, activation and output bounds (ValueError
              otherwise).  activation / output_bounds describe state dicts.
    from_flat(template, theta) builds it from a [M, P] float32 tensor of flat
    parameter vectors (parameters_to_vector order) with one device gather
    through pack_index: no host packing in an ask / tell loop."""

    def __init__(self, members, activation: str = "relu", output_bounds=None, device=None):
        specs = [_member_spec(m, activation, output_bounds) for m in members]
        if not specs:
            raise ValueError("a population needs at least one member")
        _, sizes, act, bounds = specs[0]
        sizes = validate_architecture(sizes, act)
        for j, (_, s, a, b) in enumerate(specs[1:], 1):
            if list(s) != sizes:
                raise ValueError(f"member {j} has hidden sizes {list(s)}, member 0 has {sizes}")
            if a != act:
                raise ValueError(f"member {j} has activation {a}, member 0 has {act}")
            if _bounds(b)[1:] != _bounds(bounds)[1:]:
                raise ValueError(f"member {j} has other output bounds than member 0")
        nb = _abi.policy_block_floats(len(sizes), policy_tiles(sizes))
        host = [w if isinstance(w, torch.Tensor) else pack_params(w, sizes) for w, *_ in specs]  # checks the shapes
        dev = _abi.require_gpu(device)
        blocks = torch.zeros(len(specs), population_stride(sizes), dtype=torch.float32, device=dev)
        for j, w in enumerate(host):
            blocks[j, :nb] = w.to(dev) if isinstance(w, torch.Tensor) else torch.as_tensor(w, device=dev)
        self._bind(blocks, sizes, act, bounds)

    @classmethod
    def from_flat(cls, template, theta: torch.Tensor, device=None) -> "PolicyPopulation":
        """template: a DeepTrackingPolicy, a BatchedDeepPolicy or a config
        dict (shape, activation and bounds; its weights are not read)."""
        if isinstance(template, dict):
            sizes, act = list(template.get("hidden_sizes", [64, 64])), template.get("activation", "relu")
            bounds = _bounds(template.get("output_bounds"))[0]
        else:
            _, sizes, act, bounds = _member_spec(template, None, None)
        sizes = validate_architecture(sizes, act)
        theta = torch.as_tensor(theta)
        if theta.dim() != 2 or theta.shape[0] < 1 or theta.shape[1] != flat_size(sizes) or theta.dtype != torch.float32:
            raise ValueError(f"theta must be a float32 [M, {flat_size(sizes)}] tensor for hidden sizes {sizes}, "
                             f"got {theta.dtype} {tuple(theta.shape)}")
        dev = _abi.require_gpu(device if device is not None else (theta.device if theta.is_cuda else None))
        self = cls.__new__(cls)
        gather, _ = self._device_index(sizes, dev)
        src = torch.cat([theta.to(dev), torch.zeros(theta.shape[0], 1, dtype=torch.float32, device=dev)], dim=1)
        nb = gather.numel()
        blocks = torch.zeros(theta.shape[0], population_stride(sizes), dtype=torch.float32, device=dev)
        blocks[:, :nb] = src.index_select(1, gather)
        self._bind(blocks, sizes, act, bounds)
        return self

    _INDEX: dict = {}

    @classmethod
    def _device_index(cls, sizes, dev):
        """(gather, scatter) on the device, cached per shape: gather maps the
        block to [theta, 0] columns (padding -> the appended zero), scatter
        gives every parameter's place in the block."""
        key = (tuple(sizes), str(dev))
        if key not in cls._INDEX:
            idx = pack_index(sizes)
            real = np.flatnonzero(idx != PAD)
            scatter = np.empty(flat_size(sizes), np.int64)
            scatter[idx[real]] = real
            gather = np.where(idx == PAD, flat_size(sizes), idx)
            cls._INDEX[key] = (torch.as_tensor(gather, device=dev), torch.as_tensor(scatter, device=dev))
        return cls._INDEX[key]

    def _bind(self, blocks, sizes, act, bounds) -> None:
        self.hidden_sizes, self.activation = list(sizes), act
        self.output_bounds, lo, hi = _bounds(bounds)
        self.device = blocks.device
        self.params = blocks
        self.block_floats = _abi.policy_block_floats(len(sizes), policy_tiles(sizes))
        c = _abi.PolicyPopulation()
        p = c.shape
        p.n_hidden = len(sizes)
        for i, h in enumerate(sizes):
            p.width[i] = h
        p.activation = ACTIVATIONS.index(act)
        p.params = blocks.data_ptr()
        for i in range(4):
            p.lo[i], p.hi[i] = lo[i], hi[i]
        c.members, c.stride = blocks.shape[0], blocks.shape[1]
        self.c_population = c
        if _abi.load().qt_policy_population_version() != _abi.POLICY_POPULATION_VERSION:
            raise ImportError("libquadtrack has another policy-population ABI than this package")

    @property
    def members(self) -> int:
        return self.params.shape[0]

    def __len__(self) -> int:
        return self.members

    def flat(self) -> torch.Tensor:
        """[M, P] float32 device tensor of the members' flat parameter vectors (from_flat's inverse)."""
        _, scatter = self._device_index(self.hidden_sizes, self.device)
        return self.params.index_select(1, scatter)

    def member(self, m: int) -> BatchedDeepPolicy:
        """Member m as a BatchedDeepPolicy holding a copy of its block."""
        if not 0 <= int(m) < self.members:
            raise IndexError(f"member {m} of a population of {self.members}")
        return BatchedDeepPolicy.from_block(self.params[int(m), :self.block_floats].clone(), self.hidden_sizes,
                                            self.activation, self.output_bounds)

    def rollout(self, env, crit, batch, st, nsteps: int, episodes_per_member: int,
                rec: torch.Tensor | None = None) -> None:
        """qt_policy_population_rollout on a core.EpisodeBatch / core.RolloutState of
        members * episodes_per_member episodes (in place; chunks allowed)."""
        if batch.order is not None:
            raise ValueError("the policy rollout runs episodes in index order (order must be None)")
        if batch.device != self.device:
            raise ValueError(f"the batch is on {batch.device}, the population on {self.device}")
        if batch.n != self.members * int(episodes_per_member):
            raise ValueError(f"{batch.n} episodes for {self.members} members x {episodes_per_member}")
        if rec is not None and (rec.numel() < nsteps * 16 * batch.n or rec.dtype != F64 or not rec.is_contiguous()):
            raise ValueError("rec must hold nsteps * 16 * n contiguous float64")
        c = self.c_population
        c.episodes_per_member = int(episodes_per_member)
        with torch.cuda.device(self.device):
            check(_abi.load().qt_policy_population_rollout(C.byref(env), C.byref(c), C.byref(crit),
                                                           C.byref(batch.c_batch(with_k=False)), st.c_state(),
                                                           int(nsteps), _abi.ptr(rec), _abi.stream_of(self.device)),
                  "qt_policy_population_rollout")


# ------------------------------------------------------------------ clip + optimiser step

class PolicyOptimizer:
    """The optimiser of imitation training on the device: clip_grad_norm_,
    torch.optim.{Adam, AdamW, SGD(momentum=0.9)}.step() (the trainer's
    optimisers, train.py:476-500, with torch's default betas and eps) and the
    packing of the new weights, one launch per step (qt_policy_optim_step,
    csrc/qt_policy_optim.hip).

    policy      a DeepTrackingPolicy, a BatchedDeepPolicy or a config dict: the
                shape, activation, output bounds and the starting weights
    grad_clip   clip_grad_norm_'s max_norm; <= 0: no clipping
    skip_nonfinite  a NaN or infinite gradient norm skips the step (counted in
                `skipped`) instead of propagating into the weights

    It owns, on the device: theta / m / v ([flat_size] float32,
    parameters_to_vector order), step / skipped ([1] int64) and block (the
    packed parameters).  `policy` is a BatchedDeepPolicy on that block: every
    step rewrites it in place, so the policy always flies the current weights.
    Nothing here synchronises with the host."""

    def __init__(self, policy, optimizer: str = "adam", learning_rate: float = 1e-3, weight_decay: float = 0.0,
                 grad_clip: float = 1.0, skip_nonfinite: bool = False, *, betas=(0.9, 0.999), eps: float = 1e-8,
                 momentum: float = 0.9, device=None):
        name = str(optimizer).lower()
        if name not in _abi.OPTIMIZERS:
            raise ValueError(f"Unknown optimizer: {name}")
        hyper = {"learning_rate": float(learning_rate), "weight_decay": float(weight_decay), "eps": float(eps),
                 "momentum": float(momentum)}
        for k, x in hyper.items():
            if not (np.isfinite(x) and x >= 0.0):
                raise ValueError(f"{k} must be finite and >= 0, got {x}")
        b1, b2 = (float(b) for b in betas)
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"betas must lie in [0, 1), got {(b1, b2)}")
        if np.isnan(float(grad_clip)):
            raise ValueError("grad_clip must not be NaN")
        if isinstance(policy, dict):
            policy = DeepTrackingPolicy(policy, device="cpu")
        if isinstance(policy, DeepTrackingPolicy):
            net = policy.network
            sizes, act, bounds = list(net.hidden_sizes), net.activation_name, net.output_bounds
            dev = _abi.require_gpu(device if device is not None else
                                   (policy.device if policy.device.type == "cuda" else None))
            with torch.no_grad():
                theta = torch.nn.utils.parameters_to_vector(net.parameters()).detach().to(dev, torch.float32).clone()
        elif isinstance(policy, BatchedDeepPolicy):
            sizes, act, bounds, dev = list(policy.hidden_sizes), policy.activation, policy.output_bounds, policy.device
            theta = policy.params.index_select(0, PolicyPopulation._device_index(sizes, dev)[1])
        else:
            raise TypeError(f"expected a DeepTrackingPolicy, a BatchedDeepPolicy or a config dict, "
                            f"got {type(policy).__name__}")
        if not _abi.has_policy_optim():
            raise ImportError("libquadtrack has another optimiser-step ABI than this package")
        self.optimizer, self.hidden_sizes, self.device = name, sizes, dev
        self.learning_rate, self.weight_decay = hyper["learning_rate"], hyper["weight_decay"]
        self.betas, self.eps, self.momentum = (b1, b2), hyper["eps"], hyper["momentum"]
        self.grad_clip, self.skip_nonfinite = float(grad_clip), bool(skip_nonfinite)
        size = flat_size(sizes)
        self.theta = theta.contiguous()
        self.m = torch.zeros(size, dtype=torch.float32, device=dev)
        self.v = torch.zeros(size, dtype=torch.float32, device=dev)
        self.step_count = torch.zeros(1, dtype=torch.int64, device=dev)
        self.skipped = torch.zeros(1, dtype=torch.int64, device=dev)
        self.grad_norm = torch.zeros(1, dtype=torch.float32, device=dev)
        self.block = torch.empty(_abi.policy_block_floats(len(sizes), policy_tiles(sizes)), dtype=torch.float32,
                                 device=dev)
        self._grad = torch.empty(size, dtype=torch.float32, device=dev)
        self._pack()
        self.policy = BatchedDeepPolicy.from_block(self.block, sizes, act, bounds)
        o = _abi.PolicyOptim()
        o.kind, o.skip_nonfinite = _abi.OPTIMIZERS[name], int(self.skip_nonfinite)
        o.lr, o.weight_decay, o.beta1, o.beta2 = self.learning_rate, self.weight_decay, b1, b2
        o.eps, o.momentum, o.max_norm = self.eps, self.momentum, self.grad_clip
        o.theta, o.m, o.v = self.theta.data_ptr(), self.m.data_ptr(), self.v.data_ptr()
        o.step, o.skipped = self.step_count.data_ptr(), self.skipped.data_ptr()
        o.block, o.grad_norm = self.block.data_ptr(), self.grad_norm.data_ptr()
        self.c_optim = o
        self._ref = C.byref(o)

    def _pack(self) -> None:
        """block from theta with torch's gather (construction and load_state_dict; a step packs in its launch)."""
        gather, _ = PolicyPopulation._device_index(self.hidden_sizes, self.device)
        src = torch.cat([self.theta, torch.zeros(1, dtype=torch.float32, device=self.device)])
        torch.index_select(src, 0, gather, out=self.block)

    def _want(self, t, name, shape, dtype):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
        if t.device != self.device:
            raise ValueError(f"{name} is on {t.device}, the optimiser on {self.device}")
        if t.dtype != dtype:
            raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} must have shape {list(shape)}, got {list(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")

    def step(self, grad: torch.Tensor) -> torch.Tensor:
        """One update from a [flat_size] float32 gradient (imitation_gradient's;
        it is not written).  Returns grad_norm ([1] float32, the norm before
        clipping), which the next step overwrites."""
        self._want(grad, "grad", (self.theta.numel(),), torch.float32)
        with on_device(self.device):
            check(_abi.load().qt_policy_optim_step(self.policy._ref, self._ref, grad.data_ptr(),
                                                   raw_stream(self.device)), "qt_policy_optim_step")
        return self.grad_norm

    def fit(self, features: torch.Tensor, targets: torch.Tensor, order: torch.Tensor, batch_size: int,
            weight: float = 1.0):
        """One pass of minibatch steps enqueued by one call
        (qt_policy_imitation_fit): minibatch k holds the rows
        order[k * batch_size : (k + 1) * batch_size] of features / targets
        ([rows, 18] / [rows, 4] float32; order: [m_total] int64 row numbers,
        not checked), the last one possibly short; each takes
        imitation_gradient's three launches and step's one.  Returns (losses
        [steps] float64, each minibatch's loss before its update; norms [steps]
        float32, its gradient norm before clipping), on the device."""
        if not isinstance(features, torch.Tensor) or features.dim() != 2:
            raise ValueError(f"features must be a [rows, {POLICY_INPUTS}] tensor")
        rows = features.shape[0]
        self._want(features, "features", (rows, POLICY_INPUTS), torch.float32)
        self._want(targets, "targets", (rows, 4), torch.float32)
        if not isinstance(order, torch.Tensor) or order.dim() != 1:
            raise ValueError("order must be a one-dimensional int64 tensor")
        m_total, batch = order.shape[0], int(batch_size)
        self._want(order, "order", (m_total,), torch.int64)
        if m_total < 1 or rows < 1 or batch < 1:
            raise ValueError("fit needs at least one sample and a batch_size >= 1")
        weight = float(weight)
        if not np.isfinite(weight):
            raise ValueError(f"weight must be finite, got {weight}")
        lib = _abi.load()
        widest = min(batch, m_total)
        cache = self.policy.__dict__.setdefault("_grad_workspace", {})
        ws = cache.get(widest)
        if ws is None:
            nbytes = lib.qt_policy_grad_workspace(self.policy._ref, widest)
            if nbytes < 0:
                raise ValueError(f"no gradient workspace for {widest} samples of this policy")
            ws = cache[widest] = torch.empty((nbytes + 7) // 8, dtype=F64, device=self.device)
        steps = -(-m_total // batch)
        losses = torch.empty(steps, dtype=F64, device=self.device)
        norms = torch.empty(steps, dtype=torch.float32, device=self.device)
        io = _abi.PolicyFitIO()
        io.features, io.targets, io.rows = features.data_ptr(), targets.data_ptr(), rows
        io.order, io.m_total, io.batch, io.weight = order.data_ptr(), m_total, batch, weight
        io.grad, io.losses, io.norms = self._grad.data_ptr(), losses.data_ptr(), norms.data_ptr()
        io.workspace, io.workspace_bytes = ws.data_ptr(), ws.numel() * 8
        with on_device(self.device):
            check(lib.qt_policy_imitation_fit(self.policy._ref, self._ref, C.byref(io), raw_stream(self.device)),
                  "qt_policy_imitation_fit")
        return losses, norms

    def state_dict(self) -> dict:
        """Copies of the flat tensors and the two counters (device tensors)."""
        return {"theta": self.theta.clone(), "m": self.m.clone(), "v": self.v.clone(),
                "step": self.step_count.clone(), "skipped": self.skipped.clone()}

    def load_state_dict(self, state: dict) -> None:
        """state_dict's inverse (in place: the policy keeps its block)."""
        size = self.theta.numel()
        for k, t in (("theta", self.theta), ("m", self.m), ("v", self.v), ("step", self.step_count),
                     ("skipped", self.skipped)):
            src = torch.as_tensor(state[k])
            if src.numel() != t.numel() or src.dtype != t.dtype:
                raise ValueError(f"{k} must hold {size if t.numel() == size else 1} {t.dtype} values, "
                                 f"got {src.dtype} {list(src.shape)}")
        for k, t in (("theta", self.theta), ("m", self.m), ("v", self.v), ("step", self.step_count),
                     ("skipped", self.skipped)):
            t.copy_(torch.as_tensor(state[k]).reshape(t.shape))
        self._pack()

    def network_state_dict(self) -> dict:
        """The current weights as a reference-format state dict (device copies)."""
        return unflatten(self.theta.clone(), self.hidden_sizes)
