"""GPU: the autoregressive policy's sampling at sample precision 1 (csrc/autoreg_fused.hip: k_autoreg_pack_planes +
k_autoreg_fused_sample) against a float64 numpy restatement of tests/autoreg_oracle.py's ``sample``.

Bar: scale_err(actions, float64) <= 16 x D32 per run, D32 = scale_err of the same restatement in float32 -- SPLIT x BAR of
tests/diffusion_split_cases.py, the project's bar for every split forward path.  A numpy emulation of the three-product split with the
fp32 layer-0 updates stays at 1.8 x D32 at act_dim 32 (32 compounding passes).  Every case prints its err / D32 (MI355X:
profiles/autoreg_sample_split_accuracy.json)."""
import functools

import numpy as np
import pytest
import torch

import autoreg_cases as ac
from helpers import scale_err
from test_gpu_rcsl_rollout_fused import N_TRAJ, _step_sizes, world      # noqa: F401  (the tiny world fixture, the step sizes of a store)

pytestmark = pytest.mark.gpu
NET = 0      # ORL_NET_ACTOR
BAR = 16.0                                  # SPLIT (4) x BAR (4) of tests/diffusion_split_cases.py
BASE = dict(obs_dim=5, act_dim=2, hidden=[32, 32], rows=17, runs=1)
# one edge each on the small base: tile tails and several tiles; 88 x 3 / 87 x 3 workgroups make the 32- / 64-row tile; one pass; several
# rank-1 updates; the act_dim ceiling; K tail and partial fragment; nl = 2; a second k-step of the obs product; run_regress.py's hopper
# shape; 8 fragments per wave; two runs with their own nets
CASES = dict({f"n{n}": dict(BASE, rows=n) for n in (1, 15, 16, 17, 65, 257)},
             n2801=dict(BASE, rows=2801, runs=3), n5505=dict(BASE, rows=5505, runs=3),
             act1=dict(BASE, act_dim=1), act3=dict(BASE, act_dim=3, hidden=[48, 32, 40]), act32=dict(BASE, act_dim=32, hidden=[32]),
             h20_36=dict(BASE, hidden=[20, 36]), h16=dict(BASE, hidden=[16]), od33=dict(BASE, obs_dim=33),
             work=dict(BASE, obs_dim=11, act_dim=3, hidden=[200] * 4, rows=65), h256=dict(BASE, hidden=[256]), h512=dict(BASE, hidden=[512]),
             R2=dict(BASE, runs=2))


def sample_np(net, obs, eps, dt):
    """autoreg_oracle.sample in ``dt``"""
    lin = [(net[f"model.{i}.weight"].astype(dt), net[f"model.{i}.bias"].astype(dt)) for i in sorted({int(k.split(".")[1]) for k in net})]
    (n, A), act = eps.shape, np.zeros(eps.shape, dt)
    for j in range(A):
        h = np.concatenate([obs.astype(dt), act, np.tile(np.eye(A, dtype=dt)[j], (n, 1))], axis=1)
        for W, b in lin:
            z = (h @ W.T + b).astype(dt)
            h = np.where(z > 0, z, dt(0.01) * z).astype(dt)
        act[:, j] = (h[:, 0] + np.exp(h[:, 1]).astype(dt) * eps[:, j].astype(dt)).astype(dt)
    return act


@functools.lru_cache(maxsize=None)
def reference(name):
    """per case, computed once and read-only: the nets of every run, obs, eps, the float64 actions and D32"""
    c = dict(CASES[name], seed=9100 + sorted(CASES).index(name))
    nets = [ac.make_net(c, run=r)[0] for r in range(c["runs"])]
    rng = np.random.RandomState(c["seed"] + 7)
    obs = rng.standard_normal((c["runs"], c["rows"], c["obs_dim"])).astype(np.float32)
    eps = rng.standard_normal((c["runs"], c["rows"], c["act_dim"])).astype(np.float32)
    a64 = [sample_np(nets[r], obs[r], eps[r], np.float64) for r in range(c["runs"])]
    D32 = [scale_err(sample_np(nets[r], obs[r], eps[r], np.float32), a64[r]) for r in range(c["runs"])]
    return dict(c=c, nets=nets, obs=obs, eps=eps, a64=a64, D32=D32)


def make_engine(c, nets, sample_precision=None, algo="autoreg"):
    from offlinerlkit import _engine
    eng = _engine.Engine(_engine.default_config(algo, obs_dim=c["obs_dim"], act_dim=c["act_dim"], hidden=c["hidden"], batch_size=8,
                                                n_runs=max(len(nets), 1), actor_lr=3e-4))
    for r, net in enumerate(nets):
        eng.set_net(r, NET, net)
    if sample_precision is not None:
        eng.autoreg_set_sample_precision(sample_precision)
    return eng


@pytest.mark.parametrize("name", list(CASES))
def test_actions_against_float64(name):
    ref = reference(name)
    eng = make_engine(ref["c"], ref["nets"], 1)
    try:
        assert eng.autoreg_sample_precision == 1
        got = eng.autoreg_sample(ref["obs"], ref["eps"])
    finally:
        eng.close()
    ratios = []
    for r in range(ref["c"]["runs"]):
        assert ref["D32"][r] > 0.0, (name, r)
        ratios.append(scale_err(got[r], ref["a64"][r]) / ref["D32"][r])
    print(f"{name}: err / D32 per run {', '.join(f'{x:.2f}' for x in ratios)} (bar {BAR:.0f}; D32 {max(ref['D32']):.2e})")
    assert all(x <= BAR for x in ratios), (name, ratios)


def test_the_option_does_not_leak():
    ref = reference("act3")
    c, obs, eps = ref["c"], ref["obs"], ref["eps"]
    eng, twin = make_engine(c, ref["nets"]), make_engine(c, ref["nets"])
    rng = np.random.RandomState(3)
    batch = dict(observations=rng.standard_normal((1, 8, c["obs_dim"])).astype(np.float32),
                 actions=np.tanh(rng.standard_normal((1, 8, c["act_dim"]))).astype(np.float32))
    try:
        eng.autoreg_set_sample_precision(1)
        a1 = eng.autoreg_sample(obs, eps)
        assert not np.array_equal(a1.view(np.uint32), twin.autoreg_sample(obs, eps).view(np.uint32))      # the new path ran
        drawn = eng.autoreg_sample(obs)                                     # device-drawn at 1 == teacher-forced at 1 on the drawn noise
        seps = eng.debug_read(0, "ar_seps").reshape(1, c["rows"], c["act_dim"])
        assert np.array_equal(drawn, eng.autoreg_sample(obs, seps)) and not np.array_equal(drawn, a1)
        with pytest.raises(RuntimeError, match="unknown tap ar_sx"):        # not produced by a fused call
            eng.debug_read(0, "ar_sx")
        eng.step(batch, [])
        twin.step(batch, [])
        p, q = eng.get_net(0, NET), twin.get_net(0, NET)
        assert all(np.array_equal(p[k], q[k]) for k in p)
        eng.autoreg_set_sample_precision(0)
        assert eng.autoreg_sample_precision == 0 and np.array_equal(eng.autoreg_sample(obs, eps), twin.autoreg_sample(obs, eps))
    finally:
        eng.close()
        twin.close()


def test_refusals_and_range_flags():
    ref = reference("n17")
    c, obs, eps = ref["c"], ref["obs"], ref["eps"]
    eng = make_engine(c, ref["nets"])
    other = make_engine(c, [], algo="rcsl")
    wide = make_engine(dict(c, hidden=[513]), [])
    try:
        with pytest.raises(RuntimeError, match="0 .* or 1"):
            eng.autoreg_set_sample_precision(2)
        with pytest.raises(RuntimeError, match="not an AUTOREG engine"):
            other.autoreg_set_sample_precision(1)
        with pytest.raises(RuntimeError, match="513 units is wider than the 512"):
            wide.autoreg_set_sample_precision(1)
        assert eng.autoreg_sample_precision == 0 and wide.autoreg_sample_precision == 0 and other.autoreg_sample_precision == -1
        eng.autoreg_set_sample_precision(1)
        good = eng.autoreg_sample(obs, eps)
        hot = obs.copy()
        hot[0, 3, 1] = 1e5
        with pytest.raises(RuntimeError, match="range flag.*activation"):
            eng.autoreg_sample(hot, eps)
        assert np.array_equal(eng.autoreg_sample(obs, eps), good)
        net = {k: v.copy() for k, v in ref["nets"][0].items()}
        net["model.2.weight"][1, 2] = 2000.0
        eng.set_net(0, NET, net)
        for _ in range(2):
            with pytest.raises(RuntimeError, match="range flag.*weight"):
                eng.autoreg_sample(obs, eps)
        eng.set_net(0, NET, ref["nets"][0])
        assert np.array_equal(eng.autoreg_sample(obs, eps), good)
    finally:
        for e in (eng, other, wide):
            e.close()


@pytest.mark.parametrize("before", [True, False])
def test_policy_option_reaches_every_engine_it_binds(before):
    from offlinerlkit.policy import AutoregressivePolicy
    torch.manual_seed(11)
    pol = AutoregressivePolicy(5, 3, [32, 32], 1e-3, "cuda:0")
    obs = torch.randn((65, 5), device="cuda:0")
    if before:
        pol.set_sample_precision(1)
        pol.loop_engine()
    else:
        pol.select_action_device(obs)                                       # binds at 0
        pol.set_sample_precision(1)
    torch.manual_seed(12)
    got = pol.select_action_device(obs)
    eng = pol.loop_engine()
    assert eng.autoreg_sample_precision == 1
    torch.manual_seed(12)
    eps = torch.randn((65, 3), device="cuda:0")
    want = eng.autoreg_sample(obs.cpu().numpy()[None], eps.cpu().numpy()[None])[0]
    assert np.array_equal(got.cpu().numpy(), want)
    pol.set_sample_precision(0)
    assert eng.autoreg_sample_precision == 0 and not np.array_equal(eng.autoreg_sample(obs.cpu().numpy()[None], eps.cpu().numpy()[None])[0], want)


@pytest.mark.parametrize("lag", [0, 2])
def test_fused_rollout_samples_on_the_fused_kernel(world, lag):
    """every stored action of rollout_device(fused=True) at policy sample precision 1 == orl_autoreg_sample at 1 on that step's stored
    observations and its rows of the rollout's one randn draw"""
    from test_gpu_rcsl_rollout import _rcsl_policy
    from offlinerlkit.policy import AutoregressivePolicy
    od, ad, length = world["od"], world["ad"], 4
    torch.manual_seed(21)
    ar = AutoregressivePolicy(od, ad, [32, 32], 1e-3, "cuda:0")
    ar.set_sample_precision(1)
    pol = _rcsl_policy(world["twin"](), ar, od, ad)
    ar.loop_engine()                                                        # (bound before the seed: binding draws an engine seed)
    torch.manual_seed(31)
    roll, info = pol.rollout_device(world["init"], length, fused=True, lag=lag)
    torch.manual_seed(31)
    eps = torch.randn((length, N_TRAJ, ad), device="cuda:0").cpu().numpy()
    h = roll.to_host()
    sizes, off = _step_sizes(h["terminals"].ravel(), N_TRAJ), 0
    assert len(sizes) >= 2 and sizes[1] < N_TRAJ
    eng = ar.loop_engine()
    assert eng.autoreg_sample_precision == 1
    for k, n in enumerate(sizes):
        want = eng.autoreg_sample(h["obss"][off:off + n][None], eps[k, :n][None])[0]
        assert np.array_equal(want.view(np.uint32), h["actions"][off:off + n].view(np.uint32)), (lag, k)
        off += n
