"""The imitation loss and its gradient on the GPU (qt_policy_imitation_grad,
csrc/qt_policy_grad.hip) against torch's float64 autograd on the CPU, and
train_imitation(backend="hip") on top of it.

Rule (tests/policy_grad_ref.py): for every parameter tensor
max|g_hip - g64| / max|g64| <= 4 x gap, gap = torch's own f32 CPU autograd
against g64, one scalar per network and minibatch; for the loss
|loss - loss64| <= max(4 |loss32 - loss64|, 2^-24 loss64).  Every test prints
the largest fraction of each bound it reached.
"""

import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch

import policy_grad_ref as R
import policy_model as M
import quadtrack
from quadtrack import _abi
from quadtrack.controllers import deep
from quadtrack.policy import imitation_gradient, run_policy_loop

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_POLICIES = {}
DEFAULT = ("relu", (64, 64), 301)
ALL_NETS = list(M.MATRIX_IDS) + ["relu-96x96-wide"]


def net_of(name) -> M.Net:
    return M.wide_bounds_net() if name.endswith("-wide") else M.matrix_net(name)


def device_policy(net: M.Net) -> quadtrack.BatchedDeepPolicy:
    if net.name not in _POLICIES:
        _POLICIES[net.name] = quadtrack.BatchedDeepPolicy.from_state_dict(net.sd, net.sizes, net.activation, net.bounds,
                                                                          device=DEV)
    return _POLICIES[net.name]


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV, dtype=dtype)


def gradient(net, feats, targets, index=None, weight=1.0, want_pred=True):
    """(loss, flat gradient, pred) as numpy from BatchedDeepPolicy.imitation_gradient."""
    m = len(feats) if index is None else len(index)
    pred = torch.full((m, 4), float("nan"), dtype=torch.float32, device=DEV) if want_pred else None
    loss, grad = device_policy(net).imitation_gradient(dev(feats), dev(targets), None if index is None else dev(index),
                                                       weight, pred=pred)
    assert loss.shape == (1,) and loss.dtype == torch.float64 and loss.device.type == "cuda"
    assert grad.shape == (deep.flat_size(net.sizes),) and grad.dtype == torch.float32
    return float(loss.cpu()[0]), grad.cpu().numpy(), None if pred is None else pred.cpu().numpy()


def hold(ref: R.Reference, loss, grad, label):
    frac, lfrac = ref.fractions(grad), ref.loss_fraction(loss)
    print(f"{label}: gap {ref.gap:.3e}, gradient at {frac.max():.3f} of its bound (per tensor {np.round(frac, 3)}), "
          f"loss {ref.loss64:.9g} at {lfrac:.3f} of its bound")
    assert np.isfinite(grad).all() and (frac <= 1.0).all(), (label, frac)
    assert lfrac <= 1.0, (label, loss, ref.loss64, ref.loss_bound)


@functools.lru_cache(maxsize=None)
def case(name, m):
    net = net_of(name)
    feats, targets = R.sample_features(m), R.seeded_targets(net, m)
    return net, feats, targets, R.Reference(net, feats, targets)


# ------------------------------------------------------------------ 1. accuracy matrix

@pytest.mark.parametrize("m", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("name", ALL_NETS)
def test_gradient_against_float64(name, m):
    net, feats, targets, ref = case(name, m)
    loss, grad, pred = gradient(net, feats, targets)
    hold(ref, loss, grad, f"{name} m={m}")
    assert np.abs(pred - ref.u64).max() <= 1e-4 * (net.lo_hi[1] - net.lo_hi[0]).max()


def test_default_net_over_many_workgroups_and_tiles():
    """[64, 64] relu at an m that is no multiple of 64 and gives every workgroup two or three sample tiles (the
    running partial row is read back and added to), with the samples gathered through an index."""
    net = R.extra_net(*DEFAULT)
    m = 2 * 1024 * 64 + 64 + 7
    data, labels = M.features(), R.seeded_targets(net, len(M.features()))
    index = R.ROW0 + np.arange(m) % (len(data) - R.ROW0)
    ref = R.Reference(net, data[index], labels[index])
    loss, grad, _ = gradient(net, data, labels, index=index, want_pred=False)
    hold(ref, loss, grad, f"relu-64x64 m={m}")
    m = 3 * 64 + 5  # four workgroups of one tile each
    ref = R.Reference(net, data[index[:m]], labels[index[:m]])
    loss, grad, _ = gradient(net, data, labels, index=index[:m], want_pred=False)
    hold(ref, loss, grad, f"relu-64x64 m={m}")


# ------------------------------------------------------------------ 2. derivative at zero

@pytest.mark.parametrize("act", ["relu", "leaky_relu"])
def test_derivative_at_a_pre_activation_of_zero(act):
    base = R.extra_net(act, (64, 64), 311)
    sd = dict(base.sd)
    sd["feature_extractor.0.bias"] = torch.zeros(64)
    net = dataclasses.replace(base, name=base.name + "-zero-bias", sd=sd)
    feats, targets = R.sample_features(9), R.seeded_targets(net, 9)
    feats[4] = 0.0  # every first-layer pre-activation of this sample is exactly 0
    loss, grad, _ = gradient(net, feats, targets)
    hold(R.Reference(net, feats, targets), loss, grad, f"{net.name} with a zero row")
    loss, grad, _ = gradient(net, feats[4:5], targets[4:5])
    parts = R.split(grad, net)
    hold(R.Reference(net, feats[4:5], targets[4:5]), loss, grad, f"{net.name}, the zero row alone")
    assert not parts[0].any()  # zero features
    if act == "relu":
        assert not parts[1].any()  # relu'(0) = 0: nothing reaches the first layer's bias
    else:
        assert parts[1].any()


# ------------------------------------------------------------------ 3. / 4. the forward half

def seeded_observations(n, seed):
    """([n, 6, 3] float64 observation rows, their features as _extract_features forms them)."""
    obs = np.random.default_rng(seed).uniform(-2.0, 2.0, (n, 6, 3))
    qp, qv, att, rate, tp, tv = (obs[:, i] for i in range(6))
    return obs, np.concatenate([tp - qp, tv - qv, att, rate, tp, tv], axis=1).astype(np.float32)


def obs_tensors(rows):
    t = dev(rows, torch.float64)
    q = {k: t[:, i] for i, k in enumerate(("position", "velocity", "attitude", "angular_velocity"))}
    return {"quadcopter": q, "target": {"position": t[:, 4], "velocity": t[:, 5]}}


@pytest.mark.parametrize("n", [1, 65, 130])
@pytest.mark.parametrize("name", M.MATRIX_IDS)
def test_pred_is_compute_action_bitwise_and_own_labels_give_exact_zero(name, n):
    net = net_of(name)
    obs, feats = seeded_observations(n, 1000 + n)
    action = device_policy(net).compute_action(obs_tensors(obs)).cpu().numpy()
    _, _, pred = gradient(net, feats, R.seeded_targets(net, n))
    assert pred.dtype == np.float32 and np.array_equal(pred.astype(np.float64), action)
    loss, grad, again = gradient(net, feats, pred)
    assert np.array_equal(again, pred)
    assert loss == 0.0 and not grad.any()  # every element is +0.0 or -0.0


# ------------------------------------------------------------------ 5. gather

def raw_call(pol, feats, targets, index, rows, m, weight, grad, loss, pred, ws, ws_bytes=None, policy_ref=None):
    io = _abi.PolicyGradIO()
    io.features = None if feats is None else feats.data_ptr()
    io.targets = None if targets is None else targets.data_ptr()
    io.index = None if index is None else index.data_ptr()
    io.rows, io.m, io.weight = rows, m, weight
    io.grad = None if grad is None else grad.data_ptr()
    io.loss = None if loss is None else loss.data_ptr()
    io.pred = None if pred is None else pred.data_ptr()
    io.workspace = None if ws is None else ws.data_ptr()
    io.workspace_bytes = (0 if ws is None else ws.numel() * 8) if ws_bytes is None else ws_bytes
    with torch.cuda.device(pol.device):
        return _abi.load().qt_policy_imitation_grad(pol._ref if policy_ref is None else policy_ref, C.byref(io),
                                                    _abi.stream_of(pol.device))


def test_gather_through_the_index():
    net = R.extra_net(*DEFAULT)
    data, labels = R.sample_features(300), R.seeded_targets(net, 300)
    perm = np.random.default_rng(5).permutation(300)[:100]
    by_index = gradient(net, data, labels, index=perm)
    by_copy = gradient(net, data[perm], labels[perm])
    for a, b in zip(by_index, by_copy):
        assert np.array_equal(a, b)
    # index NULL with rows > m: the first m rows
    pol = device_policy(net)
    m = 70
    ws = torch.empty(_abi.load().qt_policy_grad_workspace(pol._ref, m) // 8 + 1, dtype=torch.float64, device=DEV)
    grad = torch.empty(deep.flat_size(net.sizes), dtype=torch.float32, device=DEV)
    loss = torch.empty(1, dtype=torch.float64, device=DEV)
    assert raw_call(pol, dev(data), dev(labels), None, 300, m, 1.0, grad, loss, None, ws) == 0
    first = gradient(net, data[:m], labels[:m])
    assert float(loss.cpu()[0]) == first[0] and np.array_equal(grad.cpu().numpy(), first[1])


# ------------------------------------------------------------------ 6. determinism and isolation

def test_same_bits_whatever_the_buffers_held():
    net = R.extra_net(*DEFAULT)
    pol = device_policy(net)
    m = 200
    data, labels = R.sample_features(300), R.seeded_targets(net, 300)
    a = gradient(net, data[:m], labels[:m])
    b = gradient(net, data[:m], labels[:m])
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    pol._grad_workspace[m].fill_(float("nan"))
    stale = torch.full((deep.flat_size(net.sizes),), float("nan"), dtype=torch.float32, device=DEV)
    loss, grad = pol.imitation_gradient(dev(data[:m]), dev(labels[:m]), grad=stale)
    assert grad is stale and float(loss.cpu()[0]) == a[0] and np.array_equal(grad.cpu().numpy(), a[1])
    # rows beyond m full of NaN are never read
    poisoned, plabels = data.copy(), labels.copy()
    poisoned[m:], plabels[m:] = np.nan, np.nan
    c = gradient(net, poisoned, plabels, index=np.arange(m))
    assert c[0] == a[0] and np.array_equal(c[1], a[1])
    # a NaN feature in one sample: the loss is NaN, as torch's
    poisoned = data[:m].copy()
    poisoned[17, 3] = np.nan
    loss, _, _ = gradient(net, poisoned, labels[:m])
    assert np.isnan(loss) and np.isnan(R.torch_gradient(net, poisoned, labels[:m], 1.0, torch.float32)[0])


# ------------------------------------------------------------------ 7. padding

@pytest.mark.parametrize("width", [1, 31, 33, 65, 97])
def test_padding_has_no_gradient_element(width):
    net = R.extra_net("tanh", (width, width), 320 + width)
    feats, targets = R.sample_features(65), R.seeded_targets(net, 65)
    loss, grad, _ = gradient(net, feats, targets)
    assert grad.size == deep.flat_size(net.sizes) == 18 * width + width * width + 6 * width + 4
    hold(R.Reference(net, feats, targets), loss, grad, f"{net.name}")  # a transposed or shifted tensor fails by orders


# ------------------------------------------------------------------ 8. weight

def test_imitation_weight():
    net = R.extra_net(*DEFAULT)
    feats, targets = R.sample_features(130), R.seeded_targets(net, 130)
    one = gradient(net, feats, targets, weight=1.0)
    quarter = gradient(net, feats, targets, weight=0.25)
    assert abs(quarter[0] - 0.25 * one[0]) <= 2.0 ** -24 * abs(0.25 * one[0])
    assert (np.abs(quarter[1] - 0.25 * one[1]) <= 2.0 ** -24 * np.abs(0.25 * one[1]) + 2.0 ** -149).all()
    assert np.array_equal(quarter[2], one[2])
    hold(R.Reference(net, feats, targets, weight=0.25), quarter[0], quarter[1], "relu-64x64 weight 0.25")


# ------------------------------------------------------------------ 9. refusals

def test_invalid_arguments_are_refused_before_any_launch():
    net = R.extra_net(*DEFAULT)
    pol = device_policy(net)
    lib = _abi.load()
    assert lib.qt_policy_grad_version() == 1 and _abi.has_policy_grad()
    m, rows = 70, 100
    need = lib.qt_policy_grad_workspace(pol._ref, m)
    assert need > 0 and lib.qt_policy_grad_workspace(pol._ref, 0) < 0
    feats, targets = dev(R.sample_features(rows)), dev(R.seeded_targets(net, rows))
    index = dev(np.arange(m))
    grad = torch.full((deep.flat_size(net.sizes),), 7.0, dtype=torch.float32, device=DEV)
    loss = torch.full((1,), 7.0, dtype=torch.float64, device=DEV)
    pred = torch.full((m, 4), 7.0, dtype=torch.float32, device=DEV)
    ws = torch.full((need // 8 + 1,), 7.0, dtype=torch.float64, device=DEV)
    good = dict(feats=feats, targets=targets, index=index, rows=rows, m=m, weight=1.0, grad=grad, loss=loss, pred=pred,
                ws=ws)
    bad_shape = _abi.Policy.from_buffer_copy(pol.c_policy)
    bad_shape.width[0] = 129
    bad_act = _abi.Policy.from_buffer_copy(pol.c_policy)
    bad_act.activation = 4
    no_params = _abi.Policy.from_buffer_copy(pol.c_policy)
    no_params.params = None
    assert lib.qt_policy_grad_workspace(C.byref(bad_shape), m) < 0
    refused = [dict(feats=None), dict(targets=None), dict(grad=None), dict(loss=None), dict(ws=None),
               dict(m=0), dict(m=-1), dict(index=None, rows=m - 1), dict(ws_bytes=need - 1), dict(ws_bytes=0),
               dict(weight=float("nan")), dict(weight=float("inf")), dict(policy_ref=C.byref(bad_shape)),
               dict(policy_ref=C.byref(bad_act)), dict(policy_ref=C.byref(no_params))]
    for change in refused:
        assert raw_call(pol, **{**good, **change}) == -1, change
    with torch.cuda.device(pol.device):
        assert lib.qt_policy_imitation_grad(pol._ref, None, _abi.stream_of(pol.device)) == -1
        assert lib.qt_policy_imitation_grad(None, C.byref(_abi.PolicyGradIO()), _abi.stream_of(pol.device)) == -1
    torch.cuda.synchronize()
    for t in (grad, loss, pred, ws):
        assert (t == 7.0).all()
    assert raw_call(pol, **good) == 0  # and the same arguments unchanged are accepted
    assert not (grad == 7.0).all() and float(loss.cpu()[0]) != 7.0
    # the Python surface says what is wrong
    f, t = dev(R.sample_features(8)), dev(R.seeded_targets(net, 8))
    with pytest.raises(ValueError, match="float32"):
        pol.imitation_gradient(f.double(), t)
    with pytest.raises(ValueError, match="contiguous"):
        pol.imitation_gradient(dev(R.sample_features(16))[::2], t)
    with pytest.raises(ValueError, match="is on"):
        pol.imitation_gradient(f.cpu(), t)
    with pytest.raises(ValueError, match="shape"):
        pol.imitation_gradient(f, t[:, :3].contiguous())
    with pytest.raises(ValueError, match="int64"):
        pol.imitation_gradient(f, t, index=torch.arange(4, device=DEV, dtype=torch.int32))
    with pytest.raises(ValueError, match="finite"):
        pol.imitation_gradient(f, t, weight=float("nan"))


# ------------------------------------------------------------------ 10. the driver

ENV = {"target": {"motion_type": "stationary"}}


def fresh_policy():
    torch.manual_seed(5)
    return quadtrack.DeepTrackingPolicy({"hidden_sizes": [32], "activation": "relu"}, device=DEV)


@functools.lru_cache(maxsize=None)
def trained(backend, run=0):
    """test_train_imitation_driver's set-up: [32] relu, 64 episodes, 100 steps, 3 epochs."""
    pol = fresh_policy()
    out = quadtrack.train_imitation(pol, "riccati_lqr", {"dt": 0.01}, ENV, epochs=3, episodes_per_epoch=64,
                                    max_steps=100, seed=0, keep_datasets=True, backend=backend)
    return pol, out


@functools.lru_cache(maxsize=None)
def one_step(backend):
    pol = fresh_policy()
    out = quadtrack.train_imitation(pol, "riccati_lqr", {"dt": 0.01}, ENV, epochs=1, episodes_per_epoch=64,
                                    max_steps=100, seed=0, keep_datasets=True, backend=backend, batch_size=1 << 20,
                                    optimizer="sgd", grad_clip=0.0, learning_rate=1e-3)
    return pol, out


@functools.lru_cache(maxsize=None)
def epoch0_reference():
    start = fresh_policy().network.state_dict()
    net = M.Net("driver", [32], "relu", {k: v.detach().cpu().clone() for k, v in start.items()})
    feats, targets = (t.cpu().numpy() for t in trained("hip", 0)[1].datasets[0])
    return net, R.Reference(net, feats, targets)


def test_driver_is_reproducible_and_learns():
    (_, a), (_, b) = trained("hip", 0), trained("hip", 1)
    for key in ("mean_reward", "mean_on_target_ratio", "mean_tracking_error", "imitation_loss", "dataset_loss_before",
                "dataset_loss_after", "dataset_size"):
        assert torch.equal(getattr(a, key), getattr(b, key)), key
    for k in a.state_dict:
        assert torch.equal(a.state_dict[k], b.state_dict[k]), k
    before, after = a.dataset_loss_before.numpy(), a.dataset_loss_after.numpy()
    print("hip backend: data-set loss before", before, "after", after)
    assert before.dtype == np.float64 and before.shape == after.shape == (3,) and (after < before).all()


def test_driver_epoch0_is_the_torch_backends():
    (_, h), (_, t) = trained("hip", 0), trained("torch", 0)
    for x, y in zip(h.datasets[0], t.datasets[0]):
        assert torch.equal(x, y)
    assert h.datasets[0][0].shape == (64 * 32, 18)
    _, ref = epoch0_reference()
    lh, lt = float(h.dataset_loss_before[0]), float(t.dataset_loss_before[0])
    print(f"epoch 0 data-set loss: float64 {ref.loss64:.12g}, hip {lh:.12g} at {ref.loss_fraction(lh):.3f} of the "
          f"bound, torch backend {lt:.12g} at {ref.loss_fraction(lt):.3f}")
    assert ref.loss_fraction(lh) <= 1.0
    for key in ("mean_reward", "mean_on_target_ratio", "mean_tracking_error", "imitation_loss"):
        assert getattr(h, key)[0] == getattr(t, key)[0], key  # epoch 0's flight does not depend on the backend


def test_driver_single_sgd_step_against_the_torch_backend():
    (_, h), (_, t) = one_step("hip"), one_step("torch")
    net, ref = epoch0_reference()
    assert torch.equal(h.datasets[0][0], trained("hip", 0)[1].datasets[0][0])
    names = [f"{n}.{k}" for n in deep.layer_names(1) for k in ("weight", "bias")]
    for name, g64 in zip(names, ref.g64):
        wh, wt = h.state_dict[name].numpy().astype(np.float64), t.state_dict[name].numpy().astype(np.float64)
        ulp = np.spacing(np.abs(t.state_dict[name].numpy())).astype(np.float64)
        bound = 1e-3 * 4.0 * ref.gap * np.abs(g64).max() + ulp
        diff = np.abs(wh - wt)
        print(f"{name}: largest weight difference {diff.max():.3e}, at {(diff / bound).max():.3f} of the bound")
        assert (diff <= bound).all(), name
        assert not np.array_equal(wh, net.sd[name].numpy().astype(np.float64))  # the step moved the weights


def test_driver_leaves_the_trained_weights_in_the_policy():
    pol, out = trained("hip", 0)
    for k, v in pol.network.state_dict().items():
        assert v.device.type == "cpu" and torch.equal(v, out.state_dict[k]), k
    flown = run_policy_loop(pol, ENV, n=8, seeds=np.arange(8), max_steps=20, record=True)
    fresh = quadtrack.BatchedDeepPolicy.from_state_dict(out.state_dict, [32], "relu", device=DEV)
    again = run_policy_loop(fresh, ENV, n=8, seeds=np.arange(8), max_steps=20, record=True)
    assert torch.equal(flown.record, again.record)
    assert not torch.equal(fresh_policy().network.output_layer.weight, pol.network.output_layer.weight)
    # the module-level entry takes the DeepTrackingPolicy itself
    f, t = out.datasets[0][0][:64].contiguous(), out.datasets[0][1][:64].contiguous()
    a, b = imitation_gradient(pol, f, t), fresh.imitation_gradient(f, t)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_driver_refuses_an_unknown_backend():
    with pytest.raises(ValueError, match="backend"):
        quadtrack.train_imitation(fresh_policy(), "riccati_lqr", {"dt": 0.01}, ENV, epochs=1, episodes_per_epoch=4,
                                  max_steps=10, backend="cuda")
