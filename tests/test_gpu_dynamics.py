"""GPU: the dynamics ensemble on the HIP engine (orl_dyn_*, csrc/dynamics.hip, the Swish GEMM flavours) against fixtures from the
reference (tests/golden/dyn_*.npz) and float64 restatements."""
import os
import tempfile

import numpy as np
import pytest
import torch

import dyn_oracle as orc
import make_dyn_golden as mk
import synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = ("aleatoric", "pairwise-diff", "ensemble_std")


def _g(name):
    return np.load(os.path.join(GOLD, name))


def _state(g, tag):
    keys = sorted({k.split("/")[1] for k in g.files if k.startswith(tag + "/") and k.endswith("/full")})
    return {k: g[f"{tag}/{k}/full"].copy() for k in keys}


def _model(c):
    from offlinerlkit.modules import EnsembleDynamicsModel
    torch.manual_seed(c["seed"])
    return EnsembleDynamicsModel(c["obs_dim"], c["act_dim"], c["hidden"], c["K"], c["elites"], weight_decays=c["decays"])


def _eng(c, n_runs=1, **over):
    from offlinerlkit import _engine
    cfg = _engine.default_dyn_config(obs_dim=c["obs_dim"], act_dim=c["act_dim"], hidden=c["hidden"], num_ensemble=c["K"],
                                     num_elites=c["elites"], weight_decay=c["decays"], lr=c["lr"], batch_size=c["B"],
                                     logvar_loss_coef=c.get("coef", 0.01), n_runs=n_runs, **over)
    return _engine.Dynamics(cfg)


def _params(model):
    return {k: v.detach().cpu().numpy() for k, v in model.state_dict().items() if k != "elites"}


def _learn_setup(eng, x, t):
    K, T = x.shape[0], x.shape[1]
    eng.load_data(x.reshape(K * T, -1), t.reshape(K * T, -1))
    for r in range(eng.n_runs):
        eng.set_scaler(r, np.zeros(x.shape[-1], np.float32), np.ones(x.shape[-1], np.float32))
    return np.broadcast_to((np.arange(K)[:, None] * T + np.arange(T)[None])[None], (eng.n_runs, K, T))


def _sd_without_elites(st):
    return {k: v for k, v in st.items() if k != "elites"}


def test_swish_gemm_flavours_vs_float64():
    """forward (E_BIAS_SWISH) at width 200 on 37 rows (a partial row tile) through validate, and the dgrad (E_SWISH_GRAD) through
    the gradients of one minibatch of 37 rows, against float64"""
    c = dict(mk.MOPO, T=37, B=64)
    m = _model(c)
    eng = _eng(c)
    st = _params(m)
    eng.set_params(0, st)
    rng = np.random.default_rng(5)
    x = rng.normal(size=(c["K"], 37, 23)).astype(np.float32)
    t = (0.5 * rng.normal(size=(c["K"], 37, 18))).astype(np.float32)
    st64 = {k: v.astype(np.float64) for k, v in st.items()}
    eng.load_data(x[0], t[0])
    eng.set_scaler(0, np.zeros(23, np.float32), np.ones(23, np.float32))
    v = eng.validate(np.arange(37)[None])[0]
    ref = orc.validate(st64, x[0].astype(np.float64), t[0].astype(np.float64))
    assert np.abs(v - ref).max() <= 1e-5 * np.abs(ref).max(), (v, ref)
    rows = _learn_setup(eng, x, t)
    eng.learn_epoch(rows)
    gr = eng.debug_grads(0)
    _, g64 = orc.loss_and_grads(st64, x.astype(np.float64), t.astype(np.float64), [0.0] * 5, 0.01)
    for k in ("backbones.0.weight", "backbones.1.weight", "backbones.3.bias", "output_layer.weight", "max_logvar", "min_logvar"):
        err = np.abs(gr[k] - g64[k]).max() / np.abs(g64[k]).max()
        assert err < 1e-4, (k, err)
    eng.close()


@pytest.mark.parametrize("name,c,full", [("dyn_tiny.npz", mk.TINY, True), ("dyn_mopo.npz", mk.MOPO, False)])
def test_learn_epoch_vs_fixture(name, c, full):
    g = _g(name)
    m = _model(c)
    eng = _eng(c)
    eng.set_params(0, _params(m))
    x, t = mk.learn_inputs(c)
    rows = _learn_setup(eng, x, t)
    for e in range(c["epochs"]):
        loss = eng.learn_epoch(rows)[0]
        ref = float(g[f"epoch{e}/loss"])
        assert abs(loss - ref) <= 1e-4 * abs(ref), (e, loss, ref)
        p = eng.get_params(0)
        for k, v in p.items():
            d, r = synth.digest(v), g[f"epoch{e}/{k}/digest"]
            assert np.abs(d[2:] - r[2:]).max() <= 2e-5 + 1e-4 * np.abs(r[2:]).max(), (e, k)
        gr = eng.debug_grads(0)
        for k in ("max_logvar", "min_logvar"):
            ref = g[f"epoch{e}/grad_{k}"]
            assert np.abs(gr[k] - ref).max() <= 1e-4 * np.abs(ref).max() + 1e-7, (e, k)
    eng.close()


def test_validate_vs_fixture():
    g, c = _g("dyn_tiny.npz"), mk.TINY
    eng = _eng(c)
    eng.set_params(0, _sd_without_elites(_state(g, f"epoch{c['epochs'] - 1}")))
    eng.load_data(g["val_inputs"], g["val_targets"])
    eng.set_scaler(0, np.zeros(5, np.float32), np.ones(5, np.float32))
    v = eng.validate(np.arange(c["H"])[None])[0]
    assert np.abs(v - g["val_loss"]).max() <= 1e-4 * np.abs(g["val_loss"]).max()
    eng.close()


def _step_engine(g, c, n_runs=1):
    eng = _eng(c, n_runs=n_runs)
    st = _state(g, "step_state")
    for r in range(n_runs):
        eng.set_params(r, _sd_without_elites(st))
        eng.set_scaler(r, g["scaler_mu"], g["scaler_std"])
        eng.set_elites(r, st["elites"])
    return eng


@pytest.mark.parametrize("mode", MODES)
def test_step_vs_fixture(mode):
    g, c = _g("dyn_tiny.npz"), mk.TINY
    eng = _step_engine(g, c)
    nxt, rew, raw, pen, _ = eng.step(g["step_obs"][None], g["step_act"][None], g[f"step/{mode}/noise"][None],
                                     g[f"step/{mode}/model_idx"][None], mode, 2.5)
    for a, b in ((nxt[0], g[f"step/{mode}/next_obs"]), (rew[0], g[f"step/{mode}/reward"][:, 0]),
                 (raw[0], g[f"step/{mode}/raw_reward"][:, 0]), (pen[0], g[f"step/{mode}/penalty"][:, 0])):
        assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max() + 1e-6, mode
    eng.close()


def test_run_independence_8_runs():
    c = mk.TINY
    x, t = mk.learn_inputs(c)
    single = []
    states = []
    for r in range(8):
        torch.manual_seed(100 + r)
        m = _model(dict(c, seed=100 + r))
        states.append(_params(m))
        e1 = _eng(c)
        e1.set_params(0, states[r])
        rows = _learn_setup(e1, x, t)
        l1 = e1.learn_epoch(rows)[0]
        single.append((l1, e1.get_params(0)))
        e1.close()
    e8 = _eng(c, n_runs=8)
    for r in range(8):
        e8.set_params(r, states[r])
    rows = _learn_setup(e8, x, t)
    l8 = e8.learn_epoch(rows)
    for r in range(8):
        assert abs(l8[r] - single[r][0]) <= 1e-5 * abs(single[r][0])
        p = e8.get_params(r)
        for k, v in p.items():
            assert np.abs(v - single[r][1][k]).max() <= 1e-5 * max(np.abs(v).max(), 1e-3), (r, k)
    e8.close()


def test_inactive_runs_unchanged_bit_for_bit():
    c = mk.TINY
    x, t = mk.learn_inputs(c)
    eng = _eng(c, n_runs=3)
    for r in range(3):
        eng.set_params(r, _params(_model(dict(c, seed=200 + r))))
    rows = _learn_setup(eng, x, t)
    eng.learn_epoch(rows)
    before = [(eng.get_params(r), eng.adam_state(r)) for r in range(3)]
    loss = eng.learn_epoch(rows, active=np.array([1, 0, 1], np.int32))
    assert loss[1] == 0.0 and loss[0] > 0
    p1, (m1, v1, t1) = eng.get_params(1), eng.adam_state(1)
    for k in p1:
        assert np.array_equal(p1[k].view(np.uint32), before[1][0][k].view(np.uint32)), k
        assert np.array_equal(m1[k].view(np.uint32), before[1][1][0][k].view(np.uint32)), k
        assert np.array_equal(v1[k].view(np.uint32), before[1][1][1][k].view(np.uint32)), k
    assert t1 == before[1][1][2]
    assert not np.array_equal(eng.get_params(0)["backbones.0.weight"], before[0][0]["backbones.0.weight"])
    eng.close()


def _dynamics(c, coef=0.0, mode="aleatoric"):
    from offlinerlkit.dynamics import EnsembleDynamics
    from offlinerlkit.utils.scaler import StandardScaler
    m = _model(c)
    optim = torch.optim.Adam(m.parameters(), lr=c["lr"])
    return EnsembleDynamics(m, optim, StandardScaler(), lambda o, a, n: np.zeros((len(o), 1), bool), penalty_coef=coef,
                            uncertainty_mode=mode)


def test_train_vs_reference_trace():
    g, c = _g("dyn_trace.npz"), mk.TRACE
    dyn = _dynamics(c)
    data = {k: g[k] for k in ("observations", "actions", "next_observations", "rewards")}
    torch.manual_seed(int(g["seeds"][0]))
    np.random.seed(int(g["seeds"][1]))
    with tempfile.TemporaryDirectory() as d:
        log = mk.StubLogger(d)
        dyn.train(data, log, max_epochs=c["max_epochs"], batch_size=c["B"])
        assert os.path.exists(os.path.join(d, "dynamics.pth")) and os.path.exists(os.path.join(d, "mu.npy"))
    tr = dyn.train_trace
    assert tr["stop_epoch"][0] == int(g["stop_epoch"])
    assert list(tr["elites"][0]) == list(g["elites"])
    assert list(dyn.model.elites.cpu().numpy()) == list(g["elites"])
    tl = np.array([r["loss/dynamics_train_loss"] for r in log.rows])
    hl = np.array([r["loss/dynamics_holdout_loss"] for r in log.rows])
    assert np.abs(tl - g["train_loss"]).max() <= 1e-3 * np.abs(g["train_loss"]).max()
    assert np.all(np.abs(hl - g["holdout_loss"]) <= 1e-3 * np.abs(g["holdout_loss"]))


def test_reference_checkpoint_loads_and_steps():
    g, c = _g("dyn_tiny.npz"), mk.TINY
    dyn = _dynamics(c, coef=2.5, mode="pairwise-diff")
    st = _state(g, "step_state")
    with tempfile.TemporaryDirectory() as d:
        torch.save({k: torch.as_tensor(v) for k, v in st.items()}, os.path.join(d, "dynamics.pth"))
        np.save(os.path.join(d, "mu.npy"), g["scaler_mu"]); np.save(os.path.join(d, "std.npy"), g["scaler_std"])
        dyn.load(d)
        mode = "pairwise-diff"
        nxt, rew, term, info = dyn.step(g["step_obs"], g["step_act"], noise=g[f"step/{mode}/noise"], model_idxs=g[f"step/{mode}/model_idx"])
        assert np.abs(nxt - g[f"step/{mode}/next_obs"]).max() <= 1e-5 * np.abs(g[f"step/{mode}/next_obs"]).max()
        assert np.abs(rew - g[f"step/{mode}/reward"]).max() <= 1e-5 * np.abs(g[f"step/{mode}/reward"]).max() + 1e-6
        dyn.save(d)                                             # and the reverse: what this package writes loads into the same keys
        sd = torch.load(os.path.join(d, "dynamics.pth"))
        assert set(sd.keys()) == set(st.keys())
        for k in st:
            assert np.array_equal(sd[k].cpu().numpy(), st[k]), k


def test_mopo_rollout_end_to_end():
    """MOPOPolicy(dynamics=EnsembleDynamics(...)).rollout: the reference's keys and shapes (mopo.py:43-79)"""
    from offlinerlkit.policy import MOPOPolicy
    from helpers import mopo_oracle_setup
    from test_gpu_mb import _modules
    cfg, st, batches, _ = mopo_oracle_setup("mopo_tiny")
    c = synth.MOPO_CASES["mopo_tiny"]
    od, ad = c["obs_dim"], c["act_dim"]
    dyn = _dynamics(dict(mk.TINY, obs_dim=od, act_dim=ad), coef=2.5)
    obs0 = np.asarray(batches[0]["real"]["observations"], np.float32)
    dyn.scaler.fit(np.concatenate([obs0, np.zeros((len(obs0), ad), np.float32)], 1))
    dyn.scalers[0] = dyn.scaler
    actor, c1, c2 = _modules(c, st)
    log_alpha = torch.tensor(st["log_alpha"].copy(), requires_grad=True, device=torch.device("cuda", 0))
    pol = MOPOPolicy(dyn, actor, c1, c2, torch.optim.Adam(actor.parameters(), lr=cfg["actor_lr"]),
                     torch.optim.Adam(c1.parameters(), lr=cfg["critic_lr"]), torch.optim.Adam(c2.parameters(), lr=cfg["critic_lr"]),
                     tau=cfg["tau"], gamma=cfg["gamma"], alpha=(cfg["target_entropy"], log_alpha, torch.optim.Adam([log_alpha], lr=cfg["alpha_lr"])))
    pol.eval()
    roll, info = pol.rollout(obs0, 3)
    n = len(obs0)
    assert set(roll.keys()) == {"obss", "next_obss", "actions", "rewards", "terminals"}
    assert roll["obss"].shape == (3 * n, od) and roll["next_obss"].shape == (3 * n, od) and roll["actions"].shape == (3 * n, ad)
    assert roll["rewards"].shape == (3 * n, 1) and roll["terminals"].shape == (3 * n, 1)
    assert info["num_transitions"] == 3 * n and np.isfinite(info["reward_mean"])
    assert np.all(np.isfinite(roll["next_obss"]))


def test_device_philox_step_statistics():
    g, c = _g("dyn_tiny.npz"), mk.TINY
    eng = _step_engine(g, c)
    n = 20000
    rng = np.random.default_rng(3)
    obs = rng.normal(size=(1, n, 3)).astype(np.float32)
    act = rng.uniform(-1, 1, size=(1, n, 2)).astype(np.float32)
    zero = np.zeros((1, c["K"], n, 4), np.float32)
    mi = np.zeros((1, n), np.int64)
    base = []
    for k in range(c["K"]):                                   # the member means (zero noise) and stds (unit noise)
        m0 = eng.step(obs, act, zero, mi + k)[0][0]
        m1 = eng.step(obs, act, zero + 1, mi + k)[0][0]
        base.append((m0, m1 - m0))
    nxt, _, _, _, idx = eng.step(obs, act)
    idx = idx[0]
    assert set(np.unique(idx)) == {2, 0}                       # elites [2, 0] only
    assert abs((idx == 2).mean() - 0.5) < 0.02
    eps = np.stack([(nxt[0][i] - base[idx[i]][0][i]) / base[idx[i]][1][i] for i in range(n)])
    assert abs(eps.mean()) < 0.02 and abs(eps.var() - 1.0) < 0.05, (eps.mean(), eps.var())
    eng.close()
