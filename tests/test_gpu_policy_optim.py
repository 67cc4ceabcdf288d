"""The clip + optimiser step and the fused imitation fit on the GPU
(qt_policy_optim_step, qt_policy_imitation_fit, csrc/qt_policy_optim.hip)
against torch's optimisers in float64 on the CPU, and
train_imitation(backend="hip_fused") on top of them.

Rule (tests/policy_optim_ref.py): per quantity (dtheta = theta' - theta, m',
v') max|x - x64| / max|x64| <= 4 x gap, gap = torch's own float32 run against
the float64 one; grad_norm within 2^-23 relative of the float64 norm.  Every
test prints the largest fraction of each bound it reached.
"""

import ctypes as C
import functools

import numpy as np
import pytest
import torch

import policy_grad_ref as G
import policy_model as M
import policy_optim_ref as R
import quadtrack
from quadtrack import PolicyOptimizer, _abi
from quadtrack.controllers import deep

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = (64, 64)
NAN = float("nan")


def dev(a, dtype=None):
    return torch.as_tensor(np.array(a), device=DEV, dtype=dtype)


def bits(t):
    """The bit patterns of a float32 tensor or array (so that NaN equals NaN and +0 differs from -0)."""
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.int32) if a.dtype == np.float32 else a


def shape_of(sizes, activation=0):
    p = _abi.Policy()
    p.n_hidden = len(sizes)
    for i, h in enumerate(sizes):
        p.width[i] = h
    p.activation = activation
    return p


class Raw:
    """Device buffers of one raw qt_policy_optim_step call, preloaded with any state."""

    def __init__(self, kind, sizes, theta, m, v, step, *, lr=R.LR, weight_decay=0.0, max_norm=0.0, skip=0,
                 stale=NAN, skipped=0):
        self.sizes, self.kind = list(sizes), kind
        self.shape = shape_of(self.sizes)
        self.theta, self.m = dev(theta, torch.float32), dev(m, torch.float32)
        self.v = None if v is None else dev(v, torch.float32)
        self.step = torch.tensor([step], dtype=torch.int64, device=DEV)
        self.skipped = torch.tensor([skipped], dtype=torch.int64, device=DEV)
        nb = _abi.policy_block_floats(len(self.sizes), deep.policy_tiles(self.sizes))
        self.block = torch.full((nb,), stale, dtype=torch.float32, device=DEV)
        self.norm = torch.full((1,), stale, dtype=torch.float32, device=DEV)
        o = _abi.PolicyOptim()
        o.kind, o.skip_nonfinite = _abi.OPTIMIZERS[kind], skip
        o.lr, o.weight_decay, o.max_norm = lr, weight_decay, max_norm
        o.beta1, o.beta2, o.eps, o.momentum = R.BETAS[0], R.BETAS[1], R.EPS, R.MOMENTUM
        o.theta, o.m, o.v = self.theta.data_ptr(), self.m.data_ptr(), None if self.v is None else self.v.data_ptr()
        o.step, o.skipped = self.step.data_ptr(), self.skipped.data_ptr()
        o.block, o.grad_norm = self.block.data_ptr(), self.norm.data_ptr()
        self.o = o

    def call(self, g, shape=None, opt=None, null_grad=False):
        self.g = g if isinstance(g, torch.Tensor) else dev(g, torch.float32)
        with torch.cuda.device(DEV):
            return _abi.load().qt_policy_optim_step(C.byref(self.shape) if shape is None else shape,
                                                    C.byref(self.o) if opt is None else opt,
                                                    None if null_grad else self.g.data_ptr(), _abi.stream_of(torch.device(DEV)))

    def host(self):
        """(theta, m, v) as numpy."""
        return (self.theta.cpu().numpy(), self.m.cpu().numpy(), None if self.v is None or self.kind == "sgd"
                else self.v.cpu().numpy())

    def all_bits(self):
        return [bits(t) for t in (self.theta, self.m, self.v if self.v is not None else self.m, self.block)] + \
               [self.step.cpu().numpy(), self.skipped.cpu().numpy()]


def hold(ref, raw, label, i=-1):
    th, m, v = raw.host()
    frac, nfrac = ref.fractions(th, m, v), ref.norm_fraction(raw.norm.cpu()[0], i)
    print(f"{label}: gaps {({k: float(f'{x:.3e}') for k, x in ref.gap.items()})}, fractions of the bound "
          f"{({k: round(x, 3) for k, x in frac.items()})}, norm at {nfrac:.3f} of 2^-23")
    assert np.isfinite(th).all() and max(frac.values()) <= 1.0, (label, frac)
    assert nfrac <= 1.0, (label, float(raw.norm.cpu()[0]), ref.norms64[i])
    return frac


def single_step(kind, sizes, family, step, wd, clip):
    theta, m, v, g = R.case_inputs(tuple(sizes), family, step)
    h = dict(weight_decay=wd, max_norm=clip * R.norm64(g))
    ref = R.Reference(kind, sizes, theta, m, v, g, step, **h)
    # SGD at step 0 must not read its buffer: hand it NaN
    raw = Raw(kind, sizes, theta, np.full_like(m, NAN) if kind == "sgd" and step == 0 else m,
              None if kind == "sgd" else v, step, **h)
    assert raw.call(g) == 0
    hold(ref, raw, f"{kind} {list(sizes)} {family} step {step} wd {wd} clip {clip}")
    assert int(raw.step.cpu()[0]) == step + 1 and int(raw.skipped.cpu()[0]) == 0
    assert np.array_equal(raw.g.cpu().numpy(), g)  # grad is const
    return raw


# ------------------------------------------------------------------ 1. single steps

@pytest.mark.parametrize("step", [0, 1, 999])
@pytest.mark.parametrize("family", ["trained", "small"])
@pytest.mark.parametrize("kind", R.KINDS)
def test_single_step_against_float64(kind, family, step):
    for wd in (0.0, 1e-2):
        for clip in (0.0, 2.0, 0.5):  # off, inactive (norm < max_norm), active
            single_step(kind, SIZES, family, step, wd, clip)


@pytest.mark.parametrize("step", [0, 999])
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("sizes", [(1,), (128, 128, 128, 128)], ids=["1", "128x128x128x128"])
def test_single_step_smallest_and_largest_network(sizes, kind, step):
    """27 elements (fewer than a wave) and 52,484 (the largest flat vector)."""
    assert R.flat_size(sizes) in (27, 52484)
    single_step(kind, sizes, "trained", step, 1e-2, 0.5)
    single_step(kind, sizes, "small", step, 0.0, 0.0)


# ------------------------------------------------------------------ 2. sequences

@pytest.mark.parametrize("kind", R.KINDS)
def test_twenty_steps_on_a_prescribed_gradient_sequence(kind):
    grads = [R.seeded_gradient(SIZES, 700 + i) for i in range(20)]
    theta = R.trained_theta(SIZES)
    zero = np.zeros_like(theta)
    h = dict(weight_decay=1e-2, max_norm=0.8 * float(np.median([R.norm64(g) for g in grads])))
    ref = R.Reference(kind, SIZES, theta, zero, zero, grads, 0, **h)
    raw = Raw(kind, SIZES, theta, zero, None if kind == "sgd" else zero, 0, **h)
    for g in grads:
        assert raw.call(g) == 0
    hold(ref, raw, f"{kind} 20 steps")
    assert int(raw.step.cpu()[0]) == 20


# ------------------------------------------------------------------ 3. packing

def seeded_obs(n, seed):
    t = dev(np.random.default_rng(seed).uniform(-2.0, 2.0, (n, 6, 3)), torch.float64)
    q = {k: t[:, i] for i, k in enumerate(("position", "velocity", "attitude", "angular_velocity"))}
    return {"quadcopter": q, "target": {"position": t[:, 4], "velocity": t[:, 5]}}


@pytest.mark.parametrize("name", M.MATRIX_IDS)
def test_block_is_the_packed_new_theta(name):
    net = M.matrix_net(name)
    start = quadtrack.BatchedDeepPolicy.from_state_dict(net.sd, net.sizes, net.activation, net.bounds, device=DEV)
    opt = PolicyOptimizer(start, "adam", learning_rate=1e-2, grad_clip=1.0)
    assert opt.policy.params is opt.block and torch.equal(opt.block, start.params)
    assert np.array_equal(opt.theta.cpu().numpy(), R.trained_theta(net.sizes, M.MATRIX_SEEDS[M.MATRIX_IDS.index(name)]))
    before = opt.theta.clone()
    opt.block.fill_(NAN)  # every element, padding included, has to be written
    opt.step(dev(R.seeded_gradient(net.sizes, 800), torch.float32))
    assert not torch.equal(opt.theta, before)
    sd = {k: v.cpu() for k, v in opt.network_state_dict().items()}
    want = deep.pack_params(sd, net.sizes)
    assert np.array_equal(bits(opt.block), bits(want))  # padding: +0, not -0 and not the stale NaN
    fresh = quadtrack.BatchedDeepPolicy.from_state_dict(sd, net.sizes, net.activation, net.bounds, device=DEV)
    obs = seeded_obs(70, 3)
    assert torch.equal(opt.policy.compute_action(obs), fresh.compute_action(obs))


# ------------------------------------------------------------------ 4. determinism

@pytest.mark.parametrize("kind", R.KINDS)
def test_same_bits_whatever_the_outputs_held_and_wherever_the_inputs_lie(kind):
    theta, m, v, g = R.case_inputs(SIZES, "trained", 999)
    h = dict(weight_decay=1e-2, max_norm=0.5 * R.norm64(g))
    a = Raw(kind, SIZES, theta, m, v, 999, stale=NAN, **h)
    assert a.call(g) == 0
    shift = torch.empty(12345, dtype=torch.float32, device=DEV)  # moves the next allocations
    b = Raw(kind, SIZES, theta, m, v, 999, stale=7.0, **h)
    assert b.call(g) == 0
    assert b.theta.data_ptr() != a.theta.data_ptr() and shift.numel()
    for x, y in zip(a.all_bits(), b.all_bits()):
        assert np.array_equal(x, y)
    assert np.array_equal(bits(a.norm), bits(b.norm))


# ------------------------------------------------------------------ 5. non-finite gradients

@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("bad", [NAN, float("inf")])
def test_skip_nonfinite_leaves_everything_as_it_was(kind, bad):
    theta, m, v, g = R.case_inputs(SIZES, "trained", 999)
    h = dict(weight_decay=1e-2, max_norm=0.5 * R.norm64(g))
    poisoned = g.copy()
    poisoned[1234] = bad
    raw = Raw(kind, SIZES, theta, m, v, 999, skip=1, stale=5.0, skipped=3, **h)
    before = raw.all_bits()
    assert raw.call(poisoned) == 0
    after = raw.all_bits()
    for x, y in zip(before[:5], after[:5]):  # theta, m, v, block, step
        assert np.array_equal(x, y)
    assert int(raw.skipped.cpu()[0]) == 4 and int(raw.step.cpu()[0]) == 999
    assert not np.isfinite(float(raw.norm.cpu()[0]))
    # the next finite step is the step from the untouched state
    assert raw.call(g) == 0
    clean = Raw(kind, SIZES, theta, m, v, 999, skip=1, **h)
    assert clean.call(g) == 0
    for x, y in zip(raw.all_bits()[:5], clean.all_bits()[:5]):
        assert np.array_equal(x, y)
    assert int(raw.skipped.cpu()[0]) == 4 and int(clean.skipped.cpu()[0]) == 0


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("clip", [0.0, 0.5])
def test_without_the_flag_nan_propagates_as_in_torch(kind, clip):
    theta, m, v, g = R.case_inputs(SIZES, "trained", 999)
    h = dict(weight_decay=0.0, max_norm=clip * R.norm64(g))
    poisoned = g.copy()
    poisoned[1234] = NAN
    ref = R.Reference(kind, SIZES, theta, m, v, poisoned, 999, **h)
    raw = Raw(kind, SIZES, theta, m, v, 999, skip=0, **h)
    assert raw.call(poisoned) == 0
    th = raw.theta.cpu().numpy()
    where = np.isnan(ref.theta32)
    assert where.sum() == (1 if clip == 0.0 else th.size)  # the clip coefficient carries the NaN to every element
    assert np.array_equal(np.isnan(th), where)
    assert int(raw.step.cpu()[0]) == 1000 and int(raw.skipped.cpu()[0]) == 0
    assert np.isnan(float(raw.norm.cpu()[0]))


# ------------------------------------------------------------------ 6. refusals

def test_optim_step_refusals_launch_nothing():
    lib = _abi.load()
    assert lib.qt_policy_optim_version() == 1 and _abi.has_policy_optim()
    theta, m, v, g = R.case_inputs(SIZES, "trained", 999)
    raw = Raw("adam", SIZES, theta, m, v, 999, stale=7.0, weight_decay=1e-2, max_norm=1.0)
    before = raw.all_bits()

    def changed(**kw):
        o = _abi.PolicyOptim.from_buffer_copy(raw.o)
        for k, x in kw.items():
            setattr(o, k, x)
        return C.byref(o)

    inf = float("inf")
    refused = [dict(theta=None), dict(m=None), dict(v=None), dict(kind=2, v=None), dict(step=None), dict(skipped=None),
               dict(kind=3), dict(kind=-1), dict(lr=NAN), dict(lr=inf), dict(lr=-1e-3), dict(weight_decay=NAN),
               dict(weight_decay=inf), dict(weight_decay=-1e-2), dict(eps=NAN), dict(eps=inf), dict(eps=-1e-8),
               dict(beta1=1.0), dict(beta1=-0.1), dict(beta1=NAN), dict(beta2=1.0), dict(beta2=-0.1), dict(beta2=NAN),
               dict(max_norm=NAN)]
    for change in refused:
        assert raw.call(g, opt=changed(**change)) == -1, change
    for bad in (shape_of([64, 129]), shape_of([64, 0]), shape_of([]), shape_of([8] * 4, activation=4)):
        assert raw.call(g, shape=C.byref(bad)) == -1
    five = shape_of([8] * 4)
    five.n_hidden = 5
    assert raw.call(g, shape=C.byref(five)) == -1
    assert raw.call(g, shape=C.POINTER(_abi.Policy)()) == -1  # NULL shape, NULL opt
    assert raw.call(g, opt=C.POINTER(_abi.PolicyOptim)()) == -1
    assert raw.call(g, null_grad=True) == -1
    torch.cuda.synchronize()
    for x, y in zip(before, raw.all_bits()):
        assert np.array_equal(x, y)
    assert float(raw.norm.cpu()[0]) == 7.0
    # what is allowed: SGD without v, no block, no grad_norm, an infinite max_norm (never clips), max_norm <= 0
    assert raw.call(g, opt=changed(kind=1, v=None, block=None, grad_norm=None, max_norm=inf)) == 0
    torch.cuda.synchronize()
    assert int(raw.step.cpu()[0]) == 1000 and (raw.block == 7.0).all() and float(raw.norm.cpu()[0]) == 7.0
    assert raw.call(g, opt=changed(max_norm=-1.0)) == 0


def fit_setup(optimizer="adam", m_rows=1000, seed=11):
    """(a factory of equal optimisers on a [64, 64] relu net, 1,000 seeded samples, a seeded permutation)."""
    net = G.extra_net("relu", SIZES, 301)
    start = quadtrack.BatchedDeepPolicy.from_state_dict(net.sd, net.sizes, net.activation, net.bounds, device=DEV)
    feats, targets = dev(G.sample_features(m_rows)), dev(G.seeded_targets(net, m_rows))
    order = dev(np.random.default_rng(seed).permutation(m_rows))

    def make():
        return PolicyOptimizer(start, optimizer, learning_rate=1e-3, weight_decay=1e-2, grad_clip=1.0)

    return make, feats, targets, order


def test_fit_refusals_launch_nothing():
    make, feats, targets, order = fit_setup()
    opt = make()
    lib = _abi.load()
    m_total, batch = 1000, 64
    need = lib.qt_policy_grad_workspace(opt.policy._ref, batch)
    ws = torch.full((need // 8 + 1,), 7.0, dtype=torch.float64, device=DEV)
    grad = torch.full((R.flat_size(SIZES),), 7.0, dtype=torch.float32, device=DEV)
    losses = torch.full((16,), 7.0, dtype=torch.float64, device=DEV)
    norms = torch.full((16,), 7.0, dtype=torch.float32, device=DEV)
    state = [bits(t).copy() for t in (opt.theta, opt.m, opt.v, opt.block)]

    def call(policy=None, optim=None, **kw):
        io = _abi.PolicyFitIO()
        io.features, io.targets, io.rows = feats.data_ptr(), targets.data_ptr(), 1000
        io.order, io.m_total, io.batch, io.weight = order.data_ptr(), m_total, batch, 1.0
        io.grad, io.losses, io.norms = grad.data_ptr(), losses.data_ptr(), norms.data_ptr()
        io.workspace, io.workspace_bytes = ws.data_ptr(), ws.numel() * 8
        for k, x in kw.items():
            setattr(io, k, x)
        with torch.cuda.device(DEV):
            return lib.qt_policy_imitation_fit(opt.policy._ref if policy is None else policy,
                                               opt._ref if optim is None else optim, C.byref(io),
                                               _abi.stream_of(torch.device(DEV)))

    def optim(**kw):
        o = _abi.PolicyOptim.from_buffer_copy(opt.c_optim)
        for k, x in kw.items():
            setattr(o, k, x)
        return C.byref(o)

    def policy(**kw):
        p = _abi.Policy.from_buffer_copy(opt.policy.c_policy)
        for k, x in kw.items():
            setattr(p, k, x)
        return C.byref(p)

    other = torch.zeros_like(opt.block)
    refused = [dict(features=None), dict(targets=None), dict(order=None), dict(grad=None), dict(losses=None),
               dict(workspace=None), dict(workspace_bytes=need - 1), dict(rows=0), dict(m_total=0), dict(m_total=-5),
               dict(batch=0), dict(batch=-1), dict(weight=NAN), dict(weight=float("inf")),
               dict(batch=1 << 41, m_total=1 << 41)]
    for change in refused:
        assert call(**change) == -1, change
    for o in (optim(theta=None), optim(m=None), optim(v=None), optim(step=None), optim(skipped=None), optim(kind=7),
              optim(lr=NAN), optim(lr=-1.0), optim(weight_decay=-1.0), optim(eps=NAN), optim(beta1=1.0),
              optim(beta2=-0.5), optim(max_norm=NAN), optim(block=None), optim(block=other.data_ptr())):
        assert call(optim=o) == -1
    for p in (policy(params=None), policy(params=other.data_ptr()), policy(n_hidden=0), policy(activation=9)):
        assert call(policy=p) == -1
    wide = policy()
    wide._obj.width[0] = 129
    assert call(policy=wide) == -1
    with torch.cuda.device(DEV):
        s = _abi.stream_of(torch.device(DEV))
        assert lib.qt_policy_imitation_fit(opt.policy._ref, opt._ref, None, s) == -1
        assert lib.qt_policy_imitation_fit(None, opt._ref, C.byref(_abi.PolicyFitIO()), s) == -1
        assert lib.qt_policy_imitation_fit(opt.policy._ref, None, C.byref(_abi.PolicyFitIO()), s) == -1
    torch.cuda.synchronize()
    for t in (ws, grad, losses, norms):
        assert (t == 7.0).all()
    for x, t in zip(state, (opt.theta, opt.m, opt.v, opt.block)):
        assert np.array_equal(x, bits(t))
    assert int(opt.step_count.cpu()[0]) == 0
    assert call() == 0  # and the same arguments unchanged are accepted
    torch.cuda.synchronize()
    assert int(opt.step_count.cpu()[0]) == 16 and not (losses == 7.0).any() and not (norms == 7.0).any()
    # the Python surface says what is wrong
    with pytest.raises(ValueError, match="float32"):
        opt.step(grad.double())
    with pytest.raises(ValueError, match="shape"):
        opt.step(grad[:-1])
    with pytest.raises(ValueError, match="is on"):
        opt.step(grad.cpu())
    with pytest.raises(ValueError, match="contiguous"):
        opt.fit(feats[::2], targets[:500].contiguous(), order, 64)
    with pytest.raises(ValueError, match="int64"):
        opt.fit(feats, targets, order.int(), 64)
    with pytest.raises(ValueError, match="batch_size"):
        opt.fit(feats, targets, order, 0)
    with pytest.raises(ValueError, match="Unknown optimizer"):
        PolicyOptimizer(opt.policy, "rmsprop")
    with pytest.raises(ValueError, match="learning_rate"):
        PolicyOptimizer(opt.policy, learning_rate=-1.0)


# ------------------------------------------------------------------ 7. the fused fit

@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
@pytest.mark.parametrize("m_total,batch,steps,last", [(1000, 64, 16, 40), (1000, 130, 8, 90), (1000, 1000, 1, 1000),
                                                      (1000, 4096, 1, 1000), (1, 64, 1, 1)])
def test_fit_is_the_python_loop_bit_for_bit(m_total, batch, steps, last, optimizer):
    make, feats, targets, order = fit_setup(optimizer=optimizer)
    order = order[:m_total].contiguous()
    fused, loop = make(), make()
    assert fused.optimizer == optimizer
    first = fused.policy.imitation_gradient(feats, targets, order[:batch].contiguous(), 0.75)[0].clone()
    losses, norms = fused.fit(feats, targets, order, batch, weight=0.75)
    assert losses.shape == norms.shape == (steps,) and losses.dtype == torch.float64 and norms.dtype == torch.float32
    want_l, want_n, sizes = [], [], []
    for k in range(0, m_total, batch):
        idx = order[k:k + batch]
        sizes.append(idx.numel())
        loss, grad = loop.policy.imitation_gradient(feats, targets, idx, 0.75)
        want_l.append(loss.clone())
        want_n.append(loop.step(grad).clone())
    assert len(sizes) == steps and sizes[-1] == last
    assert torch.equal(losses, torch.cat(want_l)) and np.array_equal(bits(norms), bits(torch.cat(want_n)))
    assert torch.equal(losses[:1], first)  # imitation_gradient's loss on the first minibatch, before any update
    a, b = fused.state_dict(), loop.state_dict()
    for k in ("theta", "m", "v"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert int(a["step"][0]) == int(b["step"][0]) == steps and int(a["skipped"][0]) == 0
    assert np.array_equal(bits(fused.block), bits(loop.block))
    assert torch.isfinite(losses).all() and not torch.equal(a["theta"], make().theta)


def test_fit_first_loss_and_state_round_trip():
    make, feats, targets, order = fit_setup()
    opt = make()
    want = opt.policy.imitation_gradient(feats, targets, order[:64].contiguous())[0].clone()
    losses, _ = opt.fit(feats, targets, order, 64)
    assert torch.equal(losses[:1], want)  # bit for bit imitation_gradient's loss on the first minibatch
    # state_dict / load_state_dict: a second optimiser continues exactly where the first one stands
    other = make()
    other.load_state_dict({k: v.cpu() for k, v in opt.state_dict().items()})
    assert np.array_equal(bits(other.block), bits(opt.block))
    a, b = opt.fit(feats, targets, order, 130), other.fit(feats, targets, order, 130)
    assert torch.equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))
    assert np.array_equal(bits(opt.theta), bits(other.theta)) and int(other.step_count.cpu()[0]) == 16 + 8
    sd = opt.network_state_dict()
    assert [tuple(v.shape) for v in sd.values()] == [(64, 18), (64,), (64, 64), (64,), (4, 64), (4,)]


# ------------------------------------------------------------------ 8. the driver

ENV = {"target": {"motion_type": "stationary"}}


def fresh_policy():
    torch.manual_seed(5)
    return quadtrack.DeepTrackingPolicy({"hidden_sizes": [32], "activation": "relu"}, device=DEV)


@functools.lru_cache(maxsize=None)
def trained(backend, epochs=1):
    pol = fresh_policy()
    out = quadtrack.train_imitation(pol, "riccati_lqr", {"dt": 0.01}, ENV, epochs=epochs, episodes_per_epoch=64,
                                    samples_per_episode=8, batch_size=64, max_steps=100, seed=0, optimizer="adam",
                                    backend=backend)
    return pol, out


def tensor_differences(a, b) -> float:
    """The largest per-tensor max|a - b| / max|b| of two state dicts."""
    return max(float((a[k].double() - b[k].double()).abs().max() / b[k].double().abs().max()) for k in b)


def test_driver_one_epoch_against_the_hip_backend():
    (_, f), (_, h), (_, t) = trained("hip_fused"), trained("hip"), trained("torch")
    for key in ("mean_reward", "imitation_loss", "dataset_size", "dataset_loss_before"):
        assert torch.equal(getattr(f, key), getattr(h, key)), key
    D = tensor_differences(t.state_dict, h.state_dict)
    d = tensor_differences(f.state_dict, h.state_dict)
    print(f"final parameters after one epoch ({int(f.dataset_size[0])} pairs, batch 64): torch vs hip D = {D:.3e}, "
          f"hip_fused vs hip {d:.3e} = {d / (4.0 * D):.3f} of the bound 4 D")
    assert D > 0.0 and d <= 4.0 * D
    start = fresh_policy().network.state_dict()
    assert all(not torch.equal(f.state_dict[k], start[k].cpu()) for k in start)  # every tensor moved
    assert float(f.dataset_loss_after[0]) < float(f.dataset_loss_before[0])


def test_driver_two_epochs_leave_the_new_weights_in_the_policy():
    pol, out = trained("hip_fused", 2)
    assert torch.isfinite(out.dataset_loss_before).all() and torch.isfinite(out.dataset_loss_after).all()
    assert out.dataset_loss_before.shape == (2,)
    for k, v in pol.network.state_dict().items():
        assert v.device.type == "cpu" and torch.equal(v, out.state_dict[k]), k
    obs = seeded_obs(1, 9)
    one = {a: {k: v[0].cpu().numpy() for k, v in d.items()} for a, d in obs.items()}
    act = pol.compute_action(one)
    fresh = quadtrack.BatchedDeepPolicy.from_state_dict(out.state_dict, [32], "relu", device=DEV)
    want = fresh.compute_action(obs)[0].cpu().numpy()
    assert [act[k] for k in ("thrust", "roll_rate", "pitch_rate", "yaw_rate")] == list(want)
    first = trained("hip_fused", 1)[1]
    assert not torch.equal(out.state_dict["output_layer.weight"], first.state_dict["output_layer.weight"])


def test_driver_names_the_new_backend_when_it_refuses_one():
    with pytest.raises(ValueError, match="Unknown backend: cuda. Valid: 'torch', 'hip', 'hip_fused'"):
        quadtrack.train_imitation(fresh_policy(), "riccati_lqr", {"dt": 0.01}, ENV, epochs=1, episodes_per_epoch=4,
                                  max_steps=10, backend="cuda")
