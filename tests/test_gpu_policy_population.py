"""Policy populations on the GPU: a population launch (qt_policy_population_rollout) is bit for bit its
members' single-policy launches (qt_policy_rollout), for every kernel variant, at the member sizes around the
wave edge, in chunks, with broken neighbours, and in any member order; the per-member summaries and fitness;
and the search driver on top of it.  Every comparison is assert_array_equal / torch.equal: the two kernels
run the same device functions in the same order, so there is no tolerance to state."""

import numpy as np
import pytest
import torch

import policy_model as M
import quadtrack
from quadtrack import _abi, core
from quadtrack.policy import (evaluate_policy, evaluate_population, policy_batch, run_policy_loop,
                              run_policy_population)
from quadtrack.train import generation_seeds, search_policy

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MEMBERS, STEPS = 5, 24
ENV_CFG = {"target": {"motion_type": "linear"}}
# every kernel variant (NT 1, 2, 4; weights staged in LDS or not): 1, 2, 3 and 4 hidden layers, all four activations
NETS = [("leaky_relu", [17, 9, 32, 5]), ("relu", [33, 64]), ("tanh", [65]), ("elu", [48, 64, 33, 40]),
        ("relu", [128, 128]), ("relu", [64, 64, 64])]
NET_IDS = [M.net_id(a, s) for a, s in NETS]
# The first three stage their weights in LDS (four waves' blocks fit the CU's 160 KiB), the fourth (NT = 2,
# 4 x 55.8 KB) and the fifth (NT = 4, 4 x 77.8 KB) do not; the sixth is the largest staged shape there is
# (4 x 39.4 KB = 157,696 of 163,840 bytes).  The matrix below runs the first five; the sixth runs in the
# test of the two paths against each other.
MATRIX_IDS = NET_IDS[:5]
SIZES = [1, 63, 64, 65, 130]
_POPS = {}


def population_of(name, members=MEMBERS) -> quadtrack.PolicyPopulation:
    """`members` networks of shape `name` with different seeded weights (policy_model.random_state_dict)."""
    if (name, members) not in _POPS:
        act, sizes = NETS[NET_IDS.index(name)]
        sds = [M.random_state_dict(sizes, 300 + 17 * NET_IDS.index(name) + m) for m in range(members)]
        _POPS[name, members] = quadtrack.PolicyPopulation(sds, activation=act, device=DEV)
    return _POPS[name, members]


def inputs(E, members=MEMBERS):
    """Per-member seeds and plant masses [M, E], motions [E] shared by the members."""
    seeds = 100 + 1000 * np.arange(members)[:, None] + np.arange(E)[None, :]
    mass = np.linspace(0.8, 1.3, members * E).reshape(members, E)
    motion = [_abi.MOTIONS[i % 5] for i in range(E)]
    return seeds, motion, mass


def assert_member_equals(res, m, single, steps=STEPS):
    """Columns [m E, (m + 1) E) of a population result against a single-policy result, bit for bit."""
    E = res.episodes_per_member
    cols = slice(m * E, (m + 1) * E)
    eq = lambda a, b, what: np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy(), err_msg=f"member {m} {what}")  # noqa: E731
    eq(res.state.x[:, cols], single.state.x, "state")
    eq(res.state.target[:, cols], single.state.target, "target rows")
    eq(res.state.t[cols], single.state.t, "time")
    eq(res.state.acc[:, cols], single.state.acc, "accumulator rows")
    eq(res.metrics[:, cols], single.metrics, "metrics")
    if single.record is not None:
        assert res.record.shape == (steps, 16, res.n) and single.record.shape == (steps, 16, E)
        eq(res.record[:, :, cols], single.record, "record")


def single_run(pop, m, E, seeds, motion, mass, record=True, steps=STEPS):
    return run_policy_loop(pop.member(m), ENV_CFG, n=E, seeds=seeds[m], motion=motion, plant_mass=mass[m],
                           max_steps=steps, record=record)


# ------------------------------------------------------------------ 1. population == members

@pytest.mark.parametrize("E", SIZES)
@pytest.mark.parametrize("name", MATRIX_IDS)
def test_population_run_is_its_members_single_runs(name, E):
    pop = population_of(name)
    seeds, motion, mass = inputs(E)
    res = run_policy_population(pop, ENV_CFG, episodes_per_member=E, seeds=seeds, motion=motion, plant_mass=mass,
                                max_steps=STEPS, record=True)
    assert res.n == MEMBERS * E and res.members == MEMBERS and res.metrics.shape == (_abi.MET_ROWS, MEMBERS * E)
    assert (res.metric("steps") == STEPS).all()
    assert not torch.isnan(res.record).any()
    for m in range(MEMBERS):
        assert_member_equals(res, m, single_run(pop, m, E, seeds, motion, mass))
    # different members do compute different things
    if E > 1:
        assert not torch.equal(res.record[:, 12:, :E], res.record[:, 12:, E:2 * E])


@pytest.mark.parametrize("name", MATRIX_IDS)
def test_member_round_trip(name):
    """member(m) holds the block the population holds; flat() and from_flat() invert each other on the device."""
    pop = population_of(name)
    act, sizes = NETS[NET_IDS.index(name)]
    theta = pop.flat()
    assert theta.shape == (MEMBERS, quadtrack.controllers.deep.flat_size(sizes)) and theta.dtype == torch.float32
    again = quadtrack.PolicyPopulation.from_flat(pop.member(0), theta)
    assert torch.equal(again.params, pop.params) and again.params.shape[1] % 64 == 0
    for m in range(MEMBERS):
        sd = M.random_state_dict(sizes, 300 + 17 * NET_IDS.index(name) + m)
        want = quadtrack.BatchedDeepPolicy(sd, sizes, act, device=DEV)
        assert torch.equal(pop.member(m).params, want.params)
        flat = torch.cat([sd[f"{n}.{k}"].reshape(-1) for n in quadtrack.controllers.deep.layer_names(len(sizes))
                          for k in ("weight", "bias")])
        assert torch.equal(theta[m].cpu(), flat)
    # mixed member kinds: a BatchedDeepPolicy, a DeepTrackingPolicy's network, a state dict
    pol = quadtrack.DeepTrackingPolicy({"hidden_sizes": sizes, "activation": act}, device="cpu")
    pol.network.load_state_dict(M.random_state_dict(sizes, 301 + 17 * NET_IDS.index(name)))
    mixed = quadtrack.PolicyPopulation([pop.member(0), pol, M.random_state_dict(sizes, 302 + 17 * NET_IDS.index(name))],
                                       activation=act, device=DEV)
    assert torch.equal(mixed.params, pop.params[:3])


def test_one_member_is_the_single_policy_entry_point():
    E = 65
    pop = population_of("relu-33x64", members=1)
    seeds, motion, mass = inputs(E, members=1)
    res = run_policy_population(pop, ENV_CFG, episodes_per_member=E, seeds=seeds[0], motion=motion, plant_mass=mass[0],
                                max_steps=STEPS, record=True)
    assert_member_equals(res, 0, single_run(pop, 0, E, seeds, motion, mass))


@pytest.mark.parametrize("name", NET_IDS)
def test_staged_and_unstaged_kernels_agree(name, monkeypatch):
    """QT_POPULATION_STAGE=0 (read at every launch) runs the kernel that reads its weights from global memory;
    by default a shape whose four blocks fit the LDS runs from there.  Same bits either way, and for the
    largest staged shape, relu-64x64x64, the bits of its members' single runs."""
    E = 65
    pop = population_of(name)
    seeds, motion, mass = inputs(E)
    run = lambda: run_policy_population(pop, ENV_CFG, episodes_per_member=E, seeds=seeds, motion=motion,  # noqa: E731
                                        plant_mass=mass, max_steps=STEPS, record=True)
    monkeypatch.delenv("QT_POPULATION_STAGE", raising=False)
    default = run()
    monkeypatch.setenv("QT_POPULATION_STAGE", "0")
    unstaged = run()
    for k in ("x", "t", "acc", "target"):
        assert torch.equal(getattr(default.state, k), getattr(unstaged.state, k)), k
    assert torch.equal(default.metrics, unstaged.metrics) and torch.equal(default.record, unstaged.record)
    if name == "relu-64x64x64":
        for m in range(MEMBERS):
            assert_member_equals(default, m, single_run(pop, m, E, seeds, motion, mass))


# ------------------------------------------------------------------ 2. chunking

@pytest.mark.parametrize("name", ["relu-33x64", "tanh-65", "elu-48x64x33x40"])
def test_uneven_chunks_equal_one_launch(name):
    E, total = 65, 40
    pop = population_of(name)
    seeds, motion, mass = inputs(E)
    one = run_policy_population(pop, ENV_CFG, episodes_per_member=E, seeds=seeds, motion=motion, plant_mass=mass,
                                max_steps=total, record=True)
    cfg = quadtrack.env.config.as_env_config(ENV_CFG)
    env, crit = cfg.to_params(), core.criteria()
    n = MEMBERS * E
    batch = policy_batch(cfg, n, DEV, seeds=seeds.reshape(-1), motion=motion * MEMBERS, plant_mass=mass.reshape(-1))
    st = core.RolloutState.empty(n, batch.device)
    core.reset(env, batch, st)
    rec = torch.full((total, 16, n), float("nan"), dtype=torch.float64, device=DEV)
    done = 0
    for k in (7, 1, 32):
        pop.rollout(env, crit, batch, st, k, E, rec[done:done + k])
        done += k
    assert done == total
    for k in ("x", "t", "acc", "target"):
        assert torch.equal(getattr(st, k), getattr(one.state, k)), k
    assert torch.equal(core.episode_metrics(crit, st), one.metrics)
    assert torch.equal(rec, one.record) and not torch.isnan(rec).any()
    fixed = run_policy_population(pop, ENV_CFG, episodes_per_member=E, seeds=seeds, motion=motion, plant_mass=mass,
                                  max_steps=total, chunk=7, record=True)
    assert torch.equal(fixed.record, one.record) and torch.equal(fixed.metrics, one.metrics)


# ------------------------------------------------------------------ 3. isolation

@pytest.mark.parametrize("name", ["relu-33x64", "tanh-65", "relu-128x128"])
def test_broken_members_do_not_touch_their_neighbours(name):
    """Member 1's weights are NaN; member 3's command is full thrust whatever it observes, which carries its
    episodes through the position bound before the run ends.  Members 0, 2 and 4 (the waves before and after
    each of them, E = 65: two waves per member, the second with one live lane) are bit for bit what they are
    with members 1 and 3 intact.  The bound is read from a probe run without a bound: halfway between the
    largest |position| any episode of the other members reaches and the largest member 3 reaches."""
    E, total = 65, 40
    clean_pop = population_of(name)
    theta = clean_pop.flat().clone()
    theta[1] = float("nan")
    theta[3] = 0.0
    theta[3, -4] = 50.0  # output bias of the thrust: sigmoid -> 1, 20 N
    dirty_pop = quadtrack.PolicyPopulation.from_flat(clean_pop.member(0), theta)
    seeds = 500 + np.arange(E)
    cfg = {"target": {"motion_type": "stationary"}}
    probe = run_policy_population(dirty_pop, cfg, episodes_per_member=E, seeds=seeds, max_steps=total, record=True)
    # [M, E] largest |p|_inf of each episode (rows an ended episode never wrote are NaN: no position)
    reach = torch.nan_to_num(probe.record[:, :3], nan=0.0).abs().amax(dim=(0, 1)).view(MEMBERS, E)
    others = float(reach[[0, 1, 2, 4]].max())
    far = float(reach[3].max())
    assert far > others + 0.05, (far, others)
    bounded = {"target": {"motion_type": "stationary"}, "simulation": {"max_position": 0.5 * (far + others)}}
    clean = run_policy_population(clean_pop, bounded, episodes_per_member=E, seeds=seeds, max_steps=total, record=True)
    dirty = run_policy_population(dirty_pop, bounded, episodes_per_member=E, seeds=seeds, max_steps=total, record=True)
    for m in (0, 2, 4):
        cols = slice(m * E, (m + 1) * E)
        for k in ("x", "acc", "target"):
            assert torch.equal(getattr(clean.state, k)[:, cols], getattr(dirty.state, k)[:, cols]), (m, k)
        assert torch.equal(clean.state.t[cols], dirty.state.t[cols]), m
        assert torch.equal(clean.metrics[:, cols], dirty.metrics[:, cols]), m
        assert torch.equal(clean.record[:, :, cols], dirty.record[:, :, cols]), m
        assert (dirty.metric("steps")[cols] == total).all()
    # the broken members did break: NaN commands in every step of member 1, position_bounds ends in member 3
    assert torch.isnan(dirty.record[:, 12:, E:2 * E]).all()
    code3, steps3 = dirty.metric("termination_code")[3 * E:4 * E], dirty.metric("steps")[3 * E:4 * E]
    ended = code3 == _abi.TERM_REASONS.index("position_bounds")
    assert (steps3[ended] < total).any() and (steps3[~ended] == total).all()  # (an end on the last step has 40 too)
    assert torch.isnan(dirty.record[:, :, 3 * E:4 * E][int(steps3[ended].min()):, :, ended]).any()  # frozen: no rows


# ------------------------------------------------------------------ 4. order invariance

@pytest.mark.parametrize("name", ["leaky_relu-17x9x32x5", "elu-48x64x33x40"])
def test_permuting_members_permutes_results(name):
    E = 65
    pop = population_of(name)
    perm = [3, 0, 4, 2, 1]
    shuffled = quadtrack.PolicyPopulation([pop.member(j) for j in perm], device=DEV)
    seeds, motion, mass = inputs(E)
    run = lambda p: run_policy_population(p, ENV_CFG, episodes_per_member=E, seeds=seeds[0], motion=motion,  # noqa: E731
                                          plant_mass=mass[0], max_steps=STEPS, record=True)
    a, b = run(pop), run(shuffled)
    idx = torch.as_tensor(perm, device=DEV)
    assert torch.equal(b.member_metrics(), a.member_metrics().index_select(1, idx))
    for k in ("x", "acc", "target"):
        va, vb = getattr(a.state, k).view(-1, MEMBERS, E), getattr(b.state, k).view(-1, MEMBERS, E)
        assert torch.equal(vb, va.index_select(1, idx)), k
    assert torch.equal(b.record.view(STEPS, 16, MEMBERS, E), a.record.view(STEPS, 16, MEMBERS, E).index_select(2, idx))
    assert torch.equal(b.fitness("tracking_error"), a.fitness("tracking_error").index_select(0, idx))


# ------------------------------------------------------------------ 5. summaries and fitness

def test_member_summaries_and_fitness():
    E, name = 65, "relu-33x64"
    pop = population_of(name)
    kw = dict(num_episodes=E, base_seed=7, motion=[_abi.MOTIONS[i % 5] for i in range(E)], max_steps_per_episode=STEPS)
    summaries = evaluate_population(pop, ENV_CFG, **kw)
    res = run_policy_population(pop, ENV_CFG, episodes_per_member=E, seeds=7 + np.arange(E), motion=kw["motion"],
                                max_steps=STEPS)
    assert res.member_metrics().shape == (_abi.MET_ROWS, MEMBERS, E)
    assert res.member_metrics().data_ptr() == res.metrics.data_ptr()  # a view
    rows = []
    for m in range(MEMBERS):
        alone = evaluate_policy(pop.member(m), ENV_CFG, **kw)
        np.testing.assert_equal(summaries[m].to_dict(), alone.to_dict())
        lean = res.member_summary(m).to_dict()
        want = dict(alone.to_dict(), episode_metrics=[])
        np.testing.assert_equal(lean, want)
        assert alone.total_episodes == E and len(alone.episode_metrics) == E
        single = run_policy_loop(pop.member(m), ENV_CFG, n=E, seeds=7 + np.arange(E), motion=kw["motion"],
                                 max_steps=STEPS)
        rows.append(single.metrics)
    stacked = torch.stack(rows, dim=1)  # [rows, M, E] from the single runs
    assert torch.equal(stacked, res.member_metrics())
    fit = res.fitness("tracking_error")
    assert fit.shape == (MEMBERS,) and fit.device == res.metrics.device and fit.dtype == torch.float64
    assert torch.equal(fit, -stacked[_abi.MET["mean_tracking_error"]].mean(dim=1))
    assert torch.equal(res.fitness("on_target"), stacked[_abi.MET["on_target_ratio"]].mean(dim=1))
    assert torch.equal(res.fitness(lambda mm: mm[_abi.MET["max_tracking_error"]].amax(dim=1)),
                       stacked[_abi.MET["max_tracking_error"]].amax(dim=1))
    assert len(set(fit.tolist())) == MEMBERS  # the members differ
    with pytest.raises(ValueError, match="Unknown fitness"):
        res.fitness("reward")
    with pytest.raises(IndexError):
        res.member_summary(MEMBERS)


def test_shared_and_per_member_inputs():
    """[E] inputs are shared by every member; [M, E] inputs are per member; other shapes are refused."""
    E = 3
    pop = population_of("relu-33x64")
    seeds = 11 + np.arange(E)
    a = run_policy_population(pop, ENV_CFG, episodes_per_member=E, seeds=seeds, plant_mass=[0.9, 1.0, 1.1], max_steps=4)
    b = run_policy_population(pop, ENV_CFG, episodes_per_member=E, seeds=np.tile(seeds, (MEMBERS, 1)),
                              plant_mass=np.tile([0.9, 1.0, 1.1], (MEMBERS, 1)), motion=["linear"] * E, max_steps=4)
    assert torch.equal(a.metrics, b.metrics) and torch.equal(a.state.x, b.state.x)
    default = run_policy_population(pop, ENV_CFG, episodes_per_member=E, max_steps=4)
    zero = run_policy_population(pop, ENV_CFG, episodes_per_member=E, seeds=np.arange(E), max_steps=4)
    assert torch.equal(default.state.x, zero.state.x)
    with pytest.raises(ValueError, match="seeds must have shape"):
        run_policy_population(pop, ENV_CFG, episodes_per_member=E, seeds=np.arange(E * MEMBERS))
    with pytest.raises(ValueError, match="plant_mass must have shape"):
        run_policy_population(pop, ENV_CFG, episodes_per_member=E, plant_mass=[1.0, 1.0])
    with pytest.raises(ValueError, match="episodes_per_member"):
        run_policy_population(pop, ENV_CFG, episodes_per_member=0)
    with pytest.raises(ValueError, match="re-run"):
        a.trajectories()


# ------------------------------------------------------------------ 6. the search driver

def fitness_alone(single, m, members, E):
    """PopulationResult.fitness("tracking_error") of member m, from a single-policy run of its E episodes:
    the same torch reduction on a metrics tensor of the population's shape with that member's columns filled."""
    met = torch.zeros(_abi.MET_ROWS, members * E, dtype=torch.float64, device=DEV)
    met[:, m * E:(m + 1) * E] = single.metrics
    return (-met.view(_abi.MET_ROWS, members, E)[_abi.MET["mean_tracking_error"]].mean(dim=1))[m]

def test_search_policy_is_reproducible_and_consistent():
    kw = dict(population=8, sigma=0.1, learning_rate=0.1, generations=3, episodes_per_member=4, max_steps=40,
              env_seed=42, seed=5)
    torch.manual_seed(3)
    template = quadtrack.DeepTrackingPolicy({"hidden_sizes": [8]}, device="cpu")
    start = torch.nn.utils.parameters_to_vector(template.network.parameters()).detach().clone()
    a = search_policy(template, ENV_CFG, **kw)
    b = search_policy(template, ENV_CFG, **kw)
    G, P = 3, start.numel()
    for k in ("centre_fitness", "best_fitness", "mean_fitness", "incumbent_fitness", "best_index", "generation_best",
              "best_theta", "centre"):
        va, vb = getattr(a, k), getattr(b, k)
        assert va.device.type == "cpu" and torch.equal(va, vb), k
    assert a.centre_fitness.shape == a.best_fitness.shape == a.mean_fitness.shape == (G,)
    assert a.generation_best.shape == (G, P) and a.best_theta.shape == (P,) and a.best_theta.dtype == torch.float32
    assert torch.equal(torch.nn.utils.parameters_to_vector(template.network.parameters()).detach(), start)  # untouched
    assert not torch.equal(a.centre, start)  # the centre moved
    assert torch.equal(a.generation_best[-1], a.best_theta)
    # another noise seed gives another search
    c = search_policy(template, ENV_CFG, **dict(kw, seed=6))
    assert not torch.equal(c.generation_best, a.generation_best)
    # generation 0: the incumbent is the starting centre, so both of its copies score the same
    assert a.incumbent_fitness[0] == a.centre_fitness[0]
    M_ = kw["population"] + 2
    E = kw["episodes_per_member"]
    for g in range(G):
        # like for like: the generation's best is at least the re-run incumbent, and is the next incumbent
        assert a.best_fitness[g] >= a.incumbent_fitness[g]
        assert a.best_fitness[g] >= a.centre_fitness[g]
        assert 0 <= int(a.best_index[g]) < M_
        # the recorded fitness is that member's, run alone on the generation's seeds, under the same reduction
        alone = quadtrack.PolicyPopulation.from_flat(template, a.generation_best[g][None]).member(0)
        single = run_policy_loop(alone, ENV_CFG, n=E, seeds=generation_seeds(42, g, E), max_steps=40)
        assert float(fitness_alone(single, int(a.best_index[g]), M_, E)) == float(a.best_fitness[g]), g
        if g + 1 < G:  # the next generation's incumbent is this generation's best
            nxt = run_policy_loop(alone, ENV_CFG, n=E, seeds=generation_seeds(42, g + 1, E), max_steps=40)
            assert float(fitness_alone(nxt, M_ - 1, M_, E)) == float(a.incumbent_fitness[g + 1]), g
    assert list(generation_seeds(42, 2, 3)) == [2042, 2043, 2044]


def test_search_result_policy_saves_a_reference_checkpoint(tmp_path):
    res = search_policy({"hidden_sizes": [8], "activation": "tanh"}, ENV_CFG, population=2, sigma=0.05, generations=1,
                        episodes_per_member=2, max_steps=5)
    pol = res.best_policy
    assert isinstance(pol, quadtrack.DeepTrackingPolicy)
    assert torch.equal(torch.nn.utils.parameters_to_vector(pol.network.parameters()).detach(), res.best_theta)
    pol.save_checkpoint(tmp_path / "best.pt", metadata={"generations": 1})
    ck = torch.load(tmp_path / "best.pt", map_location="cpu", weights_only=False)
    assert set(ck) == {"model_state_dict", "config", "input_dim", "hidden_sizes", "activation", "output_bounds", "metadata"}
    assert ck["hidden_sizes"] == [8] and ck["activation"] == "tanh" and ck["input_dim"] == 18
    back = quadtrack.DeepTrackingPolicy({"hidden_sizes": [8], "activation": "tanh", "checkpoint_path": str(tmp_path / "best.pt")},
                                        device="cpu")
    assert torch.equal(torch.nn.utils.parameters_to_vector(back.network.parameters()).detach(), res.best_theta)
