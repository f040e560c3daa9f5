"""GPU: the tanh-Gaussian actor's rollout sampling on the fused split-fp16 kernel (csrc/actor_fused.hip: k_actor_pack_planes +
k_actor_fused_sample behind orl_actor_sample) against a float64 numpy restatement of
    h = relu(W h + b) ...;  mu = W_mu h + b_mu;  ls = clamp(W_sigma h + b_sigma, -5, 2);  act = tanh(mu + e^ls eps).

Bar: scale_err(actions, float64) <= 16 x D32 per run, D32 = scale_err of the same restatement in float32 -- the project's bar for every
split forward path (BAR of tests/test_gpu_autoreg_fused.py).  A numpy emulation of the three-product split (fp16 hi / lo planes of the
activations and of w * 64, fp32 accumulation) run before any GPU visit gave 1.1 x D32 on the widest case (h512) and 1.0 x on the deepest
(deep4).  Every case prints its err / D32 (MI355X: profiles/actor_sample_split_accuracy.json)."""
import functools

import numpy as np
import pytest
import torch

from helpers import scale_err

pytestmark = pytest.mark.gpu
NET = 0      # ORL_NET_ACTOR
BAR = 16.0
DEV = "cuda:0"
BASE = dict(obs_dim=5, act_dim=2, hidden=[32, 32], rows=17, runs=1, sigma_gain=1.0, det=False)
# one edge each on the small base: tile tails and several tiles; 88 x 3 / 87 x 3 workgroups make the 32- / 64-row tile (dyf_pick_tile's
# rule: the largest tile that still gives 256 workgroups); the act_dim floor and ceiling; uneven widths; K tail and partial fragment; one
# hidden layer; the deepest net; a second k-step of layer 0; run_mopo.py's halfcheetah shape; 8 fragments per wave; two runs with their
# own nets; both clamp bounds; the deterministic form
CASES = dict({f"n{n}": dict(BASE, rows=n) for n in (1, 15, 16, 17, 65, 257)},
             n2801=dict(BASE, rows=2801, runs=3), n5505=dict(BASE, rows=5505, runs=3),
             act1=dict(BASE, act_dim=1), act32=dict(BASE, act_dim=32), act3=dict(BASE, act_dim=3, hidden=[48, 32, 40]),
             h20_36=dict(BASE, hidden=[20, 36]), h16=dict(BASE, hidden=[16]), deep4=dict(BASE, hidden=[32, 48, 32, 64]),
             od33=dict(BASE, obs_dim=33), work=dict(BASE, obs_dim=17, act_dim=6, hidden=[256, 256], rows=65), h512=dict(BASE, hidden=[512]),
             R2=dict(BASE, runs=2), clamp=dict(BASE, sigma_gain=40.0), det=dict(BASE, det=True))


def make_net(c, rng):
    """nn.Linear's default init under the engine's tensor names; the sigma head's weights scaled by ``sigma_gain``"""
    net, d = {}, c["obs_dim"]
    lin = lambda g, *shape: (np.float32(g) * rng.uniform(-1, 1, shape) / np.sqrt(d)).astype(np.float32)
    for i, h in enumerate(c["hidden"]):
        net[f"backbone.model.{2 * i}.weight"], net[f"backbone.model.{2 * i}.bias"] = lin(1, h, d), lin(1, h)
        d = h
    for name, g in (("mu", 1.0), ("sigma", c["sigma_gain"])):
        net[f"dist_net.{name}.weight"], net[f"dist_net.{name}.bias"] = lin(g, c["act_dim"], d), lin(1, c["act_dim"])
    return net


def head_np(net, obs, dt):
    """(mu, raw log-sigma) in ``dt``"""
    h = obs.astype(dt)
    for i in range(sum(k.startswith("backbone") for k in net) // 2):
        h = np.maximum((h @ net[f"backbone.model.{2 * i}.weight"].astype(dt).T + net[f"backbone.model.{2 * i}.bias"].astype(dt)).astype(dt), 0)
    return [(h @ net[f"dist_net.{n}.weight"].astype(dt).T + net[f"dist_net.{n}.bias"].astype(dt)).astype(dt) for n in ("mu", "sigma")]


def sample_np(net, obs, eps, dt, det=False):
    mu, ls = head_np(net, obs, dt)
    return np.tanh(mu if det else (mu + np.exp(np.clip(ls, dt(-5), dt(2))).astype(dt) * eps.astype(dt)).astype(dt)).astype(dt)


@functools.lru_cache(maxsize=None)
def reference(name):
    """per case, computed once and read-only: the nets of every run, obs, eps, the float64 actions and D32"""
    c = CASES[name]
    rng = np.random.RandomState(9300 + sorted(CASES).index(name))
    nets = [make_net(c, rng) for _ in range(c["runs"])]
    obs = rng.standard_normal((c["runs"], c["rows"], c["obs_dim"])).astype(np.float32)
    eps = rng.standard_normal((c["runs"], c["rows"], c["act_dim"])).astype(np.float32)
    a64 = [sample_np(nets[r], obs[r], eps[r], np.float64, c["det"]) for r in range(c["runs"])]
    D32 = [scale_err(sample_np(nets[r], obs[r], eps[r], np.float32, c["det"]), a64[r]) for r in range(c["runs"])]
    return dict(c=c, nets=nets, obs=obs, eps=eps, a64=a64, D32=D32)


def make_engine(c, nets, algo="sac", runs=None):
    from offlinerlkit import _engine
    eng = _engine.Engine(_engine.default_config(algo, obs_dim=c["obs_dim"], act_dim=c["act_dim"], hidden=c["hidden"], batch_size=8,
                                                n_runs=runs or max(len(nets), 1)))
    for r, net in enumerate(nets):
        eng.set_net(r, NET, net)
    return eng


@pytest.mark.parametrize("name", list(CASES))
def test_actions_against_float64(name):
    ref = reference(name)
    c = ref["c"]
    if name == "clamp":
        ls = head_np(ref["nets"][0], ref["obs"][0], np.float64)[1]
        assert (ls < -5).any() and (ls > 2).any()
    eng = make_engine(c, ref["nets"])
    try:
        got = eng.actor_sample(ref["obs"], None if c["det"] else ref["eps"], deterministic=c["det"])
    finally:
        eng.close()
    ratios = []
    for r in range(c["runs"]):
        assert ref["D32"][r] > 0.0, (name, r)
        ratios.append(scale_err(got[r], ref["a64"][r]) / ref["D32"][r])
    print(f"{name}: err / D32 per run {', '.join(f'{x:.2f}' for x in ratios)} (bar {BAR:.0f}; D32 {max(ref['D32']):.2e})")
    assert all(x <= BAR for x in ratios), (name, ratios)


def test_ragged_selected_runs_and_device_noise():
    c = dict(BASE, rows=65, runs=3)
    rng = np.random.RandomState(5)
    nets = [make_net(c, rng) for _ in range(3)]
    obs, eps = rng.standard_normal((3, 65, 5)).astype(np.float32), rng.standard_normal((3, 65, 2)).astype(np.float32)
    eng = make_engine(c, nets)
    try:
        full = eng.actor_sample(obs, eps)
        rag = eng.actor_sample(obs, eps, live=[65, 0, 17])
        for r, n in enumerate((65, 0, 17)):
            assert np.array_equal(rag[r, :n].view(np.uint32), full[r, :n].view(np.uint32)) and not rag[r, n:].any(), r
        assert np.array_equal(eng.actor_sample(obs[1], eps[1], run=1).view(np.uint32), full[1].view(np.uint32))
        assert not np.array_equal(full[0], full[1])
        one = eng.actor_sample(obs[2], eps[2], run=2, live=[17])
        assert np.array_equal(one[:17].view(np.uint32), full[2, :17].view(np.uint32)) and not one[17:].any()
        d1, d2 = eng.actor_sample(obs), eng.actor_sample(obs)             # device-drawn normals
        assert not np.array_equal(d1, d2)
        for d in (d1, d2):
            assert np.isfinite(d).all() and (np.abs(d) < 1).all()
    finally:
        eng.close()


def test_refusals_and_range_flags():
    ref = reference("n17")
    c, obs, eps = ref["c"], ref["obs"], ref["eps"]
    eng, wide, iql = make_engine(c, ref["nets"]), make_engine(dict(c, hidden=[513]), []), make_engine(c, [], algo="iql")
    try:
        with pytest.raises(RuntimeError, match="513 units is wider than the 512"):
            wide.actor_sample(obs, eps)
        with pytest.raises(RuntimeError, match="act_dim"):
            make_engine(dict(c, act_dim=33), []).close()
        with pytest.raises(RuntimeError, match="IQL actor.*state-independent"):
            iql.actor_sample(obs, eps)
        good = eng.actor_sample(obs, eps)
        hot = obs.copy()
        hot[0, 3, 1] = 1e5
        with pytest.raises(RuntimeError, match="range flag.*activation"):
            eng.actor_sample(hot, eps)
        assert np.array_equal(eng.actor_sample(obs, eps), good)
        net = {k: v.copy() for k, v in ref["nets"][0].items()}
        net["dist_net.sigma.weight"][1, 2] = 2000.0
        eng.set_net(0, NET, net)
        for _ in range(2):
            with pytest.raises(RuntimeError, match="range flag.*weight"):
                eng.actor_sample(obs, eps)
        eng.set_net(0, NET, ref["nets"][0])
        assert np.array_equal(eng.actor_sample(obs, eps), good)
    finally:
        for e in (eng, wide, iql):
            e.close()


@pytest.mark.parametrize("before", [True, False])
def test_policy_switch(before):
    import test_gpu_mb_trainer as tt
    torch.manual_seed(11)
    pol = tt._policy("mopo", None)
    obs = torch.randn((65, tt.OD), device=DEV)
    if before:
        pol.set_rollout_precision(1)
    pol._bind(256)
    torch.manual_seed(12)
    a0, _ = pol.actforward(obs)
    torch.manual_seed(12)
    assert pol._rollout_precision == int(before) and (before or torch.equal(pol.actforward_device(obs), a0))
    pol.set_rollout_precision(1)
    torch.manual_seed(12)
    got = pol.actforward_device(obs).cpu().numpy()
    torch.manual_seed(12)
    eps = torch.randn((65, tt.AD), device=DEV).cpu().numpy()
    want = pol._eng.actor_sample(obs.cpu().numpy(), eps, run=0)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the bar's distance from the torch path: D32 from the float32 restatement on the live weights
    net = pol._eng.get_net(0, NET)
    a64 = sample_np(net, obs.cpu().numpy(), eps, np.float64)
    D32 = scale_err(sample_np(net, obs.cpu().numpy(), eps, np.float32), a64)
    assert D32 > 0 and scale_err(got, a0.detach().cpu().numpy()) <= BAR * D32
    pol.set_rollout_precision(0)
    torch.manual_seed(12)
    assert torch.equal(pol.actforward_device(obs), a0)


@pytest.mark.parametrize("per_run", [False, True])
def test_rollout_device_samples_on_the_fused_kernel(tmp_path, per_run):
    """every action rollout_device stores at rollout precision 1 == orl_actor_sample on that step's stored observations and that
    step's rows of the same torch.randn sequence"""
    import test_gpu_mb_trainer as tt
    from offlinerlkit.buffer import ReplayBuffer
    from offlinerlkit.dynamics import EnsembleDynamics
    from offlinerlkit.modules import EnsembleDynamicsModel
    from offlinerlkit.utils.logger import Logger
    from offlinerlkit.utils.scaler import StandardScaler
    from offlinerlkit.utils.termination_fns import termination_fn_ant
    torch.manual_seed(5)
    np.random.seed(5)
    ds = tt.make_dataset(n_episodes=300)
    logger = Logger(str(tmp_path), {"consoleout_backup": "stdout", "dynamics_training_progress": "csv"})
    data = ReplayBuffer(len(ds["rewards"]), (tt.OD,), np.float32, tt.AD, np.float32, device=DEV)
    data.load_dataset(ds)
    model = EnsembleDynamicsModel(tt.OD, tt.AD, [64, 64], num_ensemble=5, num_elites=3, weight_decays=[2.5e-5, 5e-5, 1e-4], device=DEV)
    dyn = EnsembleDynamics(model, torch.optim.Adam(model.parameters(), lr=1e-3), StandardScaler(), termination_fn_ant, penalty_coef=0.5,
                           uncertainty_mode="aleatoric")
    dyn.train(data.sample_all(), logger, max_epochs=10, max_epochs_since_update=5)
    pol = tt._policy("mopo", dyn)
    R, N, L = (2, 300, 3) if per_run else (1, 300, 3)
    pol.set_engine_options(n_runs=R, seed=11)
    pol.set_rollout_precision(1)
    pol._bind(256)
    rng = np.random.RandomState(1)      # x0 around TERM_ANT's 0.2 / 1.0 bounds: some rows end in every step
    init = np.stack([rng.uniform(0.25, 0.95, R * N), rng.uniform(-1.5, 1.5, R * N)], 1).astype(np.float32)
    fakes = [ReplayBuffer(N * L, (tt.OD,), np.float32, tt.AD, np.float32, device=DEV) for _ in range(R)]
    torch.manual_seed(123)
    info = pol.rollout_device(data, fakes if per_run else fakes[0], N, L, init_obss=init.reshape(R, N, -1) if per_run else init)
    got = [f.sample_all() for f in fakes]
    term = [g["terminals"].ravel() for g in got]
    torch.manual_seed(123)
    live, off, shrunk = np.full(R, N), np.zeros(R, int), False
    while live.max() > 0 and off.max() < np.atleast_1d(info["num_transitions"]).max():
        nmax = int(live.max())
        eps = torch.randn((R, nmax, tt.AD) if per_run else (nmax, tt.AD), device=DEV).cpu().numpy().reshape(R, nmax, tt.AD)
        nxt = live.copy()
        for r in range(R):
            n, sl = int(live[r]), slice(off[r], off[r] + int(live[r]))
            if n:
                want = pol._eng.actor_sample(got[r]["observations"][sl], eps[r, :n], run=r)
                assert np.array_equal(want.view(np.uint32), got[r]["actions"][sl].view(np.uint32)), (r, off[r])
            nxt[r] = n - int(term[r][sl].sum())
            off[r] += n
        shrunk |= bool((nxt < live).any() and nxt.max() > 0)
        live = nxt
    assert shrunk and all(off[r] == len(term[r]) for r in range(R))
