"""GPU: RAMBO's adversarial model update on the dynamics engine (orl_dynadv_*, csrc/dynamics.hip) against fixtures from the reference
(tests/golden/rambo_*.npz, make_rambo_golden.py) and the float64 restatement (tests/rambo_oracle.py), and RAMBOPolicy end to end on
the point-mass task of tests/test_gpu_training.py."""
import os

import numpy as np
import pytest
import torch

import make_rambo_golden as mr
import rambo_oracle as ro
import synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROWS = ("obs", "act", "sl_obs", "sl_act", "sl_next_obs", "sl_rew")
F64 = np.float64


def _g(name):
    return np.load(os.path.join(GOLD, name))


def _state(g, tag):
    keys = sorted({k[len(tag) + 1:-len("/full")] for k in g.files if k.startswith(tag + "/") and k.endswith("/full")})
    return {k: g[f"{tag}/{k}/full"].copy() for k in keys if k != "elites"}


def _eng(c, n_runs=1, **over):
    from offlinerlkit import _engine
    cfg = _engine.default_dyn_config(obs_dim=c["obs_dim"], act_dim=c["act_dim"], hidden=c["hidden"], num_ensemble=c["K"],
                                     num_elites=c["elites"], weight_decay=c["decays"], lr=c["lr"], batch_size=64, n_runs=n_runs, **over)
    return _engine.Dynamics(cfg)


def _model_params(c, seed=None):
    from offlinerlkit.modules import EnsembleDynamicsModel
    torch.manual_seed(c["seed"] if seed is None else seed)
    m = EnsembleDynamicsModel(c["obs_dim"], c["act_dim"], c["hidden"], c["K"], c["elites"], weight_decays=c["decays"])
    return {k: v.detach().cpu().numpy() for k, v in m.state_dict().items() if k != "elites"}


def _tiny_engine(g, c, w):
    eng = _eng(c)
    eng.set_params(0, _state(g, "init"))
    eng.set_scaler(0, g["scaler_mu"], g["scaler_std"])
    eng.set_elites(0, c["elite_idx"])
    eng.adv_configure(c["adv_lr"], adv_weight=w, rollout_rows=c["Ba"], sl_rows=c["Bs"])
    return eng


def _fwd(eng, rows, eps=None, midx=None):
    return eng.adv_forward(*[rows[k][None] for k in ROWS], None if eps is None else eps[None], None if midx is None else midx[None])


def _rel(a, b):
    return float(np.abs(np.asarray(a, F64) - np.asarray(b, F64)).max() / max(np.abs(np.asarray(b, F64)).max(), 1e-300))


def test_forward_vs_fixture():
    g, c = _g("rambo_tiny.npz"), mr.TINY
    eng = _tiny_engine(g, c, 1.0)
    tag = "w1/step0"
    nxt, rew, mi = _fwd(eng, {k: g[f"{tag}/{k}"] for k in ROWS}, g[f"{tag}/eps"], g[f"{tag}/model_idx"])
    assert np.array_equal(mi[0], g[f"{tag}/model_idx"])
    for a, b in ((nxt[0], g[f"{tag}/next_obs"]), (rew[0], g[f"{tag}/reward"])):
        print("forward err", np.abs(a - b).max(), "bound", 1e-5 * np.abs(b).max() + 1e-6)
        assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max() + 1e-6
    eng.close()


@pytest.mark.parametrize("traj,w", [("w1", 1.0), ("w0", 0.0)])
def test_update_vs_fixture(traj, w):
    """three consecutive updates; a step() and a validate() between the two calls must not disturb the pending forward; learn_epoch's
    Adam state (given nonzero values here) stays bit for bit.  exp_avg is linear in the gradient (held to the gradient's bar, 1e-4 of
    its max), exp_avg_sq quadratic (2e-4 of its max)."""
    g, c = _g("rambo_tiny.npz"), mr.TINY
    eng = _tiny_engine(g, c, w)
    rng = np.random.default_rng(1)
    lm = {k: rng.normal(size=v.shape).astype(np.float32) for k, v in _state(g, "init").items()}
    lv = {k: (v * v).astype(np.float32) for k, v in lm.items()}
    eng.set_adam_state(0, lm, lv, 5)
    before = eng.adam_state(0)
    vx = rng.normal(size=(8, 5)).astype(np.float32)
    eng.load_data(vx, rng.normal(size=(8, 4)).astype(np.float32))
    for t in range(c["steps"]):
        tag = f"{traj}/step{t}"
        _fwd(eng, {k: g[f"{tag}/{k}"] for k in ROWS}, g[f"{tag}/eps"], g[f"{tag}/model_idx"])
        eng.step(vx[None, :, :3], vx[None, :, 3:])
        eng.validate(np.arange(8)[None])
        m = eng.adv_update(g[f"{tag}/advantage"][None])[0]
        ref = dict(zip(mr.LOSS_KEYS, g[f"{tag}/losses"]))
        for k, v in zip(("all_loss", "sl_loss", "adv_loss", "adv_log_prob"), m):
            print(traj, t, k, float(v), ref[k], abs(v - ref[k]) / abs(ref[k]))
        for k, v in zip(("all_loss", "sl_loss", "adv_loss", "adv_log_prob"), m):
            assert abs(v - ref[k]) <= 1e-4 * abs(ref[k]), (t, k, v, ref[k])
        p, refst = eng.get_params(0), _state(g, tag)
        for k in refst:
            assert np.abs(p[k] - refst[k]).max() <= 2e-5 + 1e-4 * np.abs(refst[k]).max(), (t, k)
        gr = eng.debug_grads(0)
        for k in ("max_logvar", "min_logvar"):
            r = g[f"{tag}/grad_{k}"]
            assert np.abs(gr[k] - r).max() <= 1e-4 * np.abs(r).max() + 1e-7, (t, k)
        am, av, at = eng.adv_adam_state(0)
        assert at == t + 1
        for k in [x[len(tag) + 9:] for x in g.files if x.startswith(tag + "/exp_avg/")]:
            r1, r2 = g[f"{tag}/exp_avg/{k}"], g[f"{tag}/exp_avg_sq/{k}"]
            assert np.abs(am[k] - r1).max() <= 1e-4 * np.abs(r1).max() + 1e-9, (t, k)
            assert np.abs(av[k] - r2).max() <= 2e-4 * np.abs(r2).max() + 1e-12, (t, k)
    after = eng.adam_state(0)
    assert after[2] == before[2] == 5
    for k in before[0]:
        assert np.array_equal(after[0][k].view(np.uint32), before[0][k].view(np.uint32)), k
        assert np.array_equal(after[1][k].view(np.uint32), before[1][k].view(np.uint32)), k
    eng.close()


def _random_rows(rng, c, Ba, Bs):
    od, ad = c["obs_dim"], c["act_dim"]
    rows = {"obs": rng.normal(size=(Ba, od)), "act": rng.uniform(-1, 1, size=(Ba, ad)), "sl_obs": rng.normal(size=(Bs, od)),
            "sl_act": rng.uniform(-1, 1, size=(Bs, ad))}
    rows["sl_next_obs"] = rows["sl_obs"] + 0.3 * rng.normal(size=(Bs, od))
    rows["sl_rew"] = rng.normal(size=(Bs, 1))
    return {k: v.astype(np.float32) for k, v in rows.items()}


def _normalised(rng, n):
    a = rng.normal(size=n)
    return ((a - a.mean()) / (a.std(ddof=1) + 1e-6)).astype(np.float32)


def test_gradient_vs_float64_width_200():
    """one update at [200] x 4, 7 members, 37 + 29 rows (partial row tiles, the block boundary inside a tile) against float64: every
    tensor's gradient within 1e-4 of its max, layer 0's (the wgrad on the input shared by the members) included.  The dataset targets
    are the (float64) predictions of member 2, which is no elite: its mean gradient is then zero up to the fp32 rounding of the targets
    and its whole gradient is the supervised one, which the oracle gives with adv_weight 0."""
    c = dict(mr.MOPO, Ba=37, Bs=29)
    Ba, Bs, K, od = 37, 29, c["K"], c["obs_dim"]
    rng = np.random.default_rng(11)
    st = _model_params(c)
    rows = _random_rows(rng, c, Ba, Bs)
    mu, std = np.zeros(23, np.float32), np.ones(23, np.float32)
    eps = rng.normal(size=(K, Ba, od + 1)).astype(np.float32)
    midx = rng.choice(c["elite_idx"], size=Ba)
    adv = _normalised(rng, Ba)
    ne = 2
    f0 = ro.step_forward(st, mu, std, rows, eps, midx, F64)
    pred = f0["mean"][ne, Ba:]
    rows["sl_next_obs"] = (rows["sl_obs"] + pred[:, :od]).astype(np.float32)
    rows["sl_rew"] = pred[:, od:].astype(np.float32)
    f = ro.step_forward(st, mu, std, rows, eps, midx, F64)
    m64, g64 = ro.step_grads(f, c["elite_idx"], adv, 1.0, c["decays"], F64)
    _, g64_sl = ro.step_grads(f, c["elite_idx"], adv, 0.0, c["decays"], F64)
    eng = _eng(c)
    eng.set_params(0, st)
    eng.set_scaler(0, mu, std)
    eng.set_elites(0, c["elite_idx"])
    eng.adv_configure(1e-3, adv_weight=1.0, rollout_rows=Ba, sl_rows=Bs)
    nxt, rew, _ = _fwd(eng, rows, eps, midx)
    assert np.abs(nxt[0] - f["sample"][:, :-1]).max() <= 1e-5 * np.abs(f["sample"]).max() + 1e-6
    m = eng.adv_update(adv[None])[0]
    assert abs(m[3] - m64["adv_log_prob"]) <= 1e-4 * abs(m64["adv_log_prob"])
    gr = eng.debug_grads(0)
    for k in g64:
        err = _rel(gr[k], g64[k])
        print(k, "grad err / max", err)
        assert err < 1e-4, (k, err)
    for k in ("backbones.0.weight", "backbones.3.weight", "output_layer.weight", "output_layer.bias"):
        big = np.abs(g64[k]).max()
        assert np.abs(gr[k][ne] - g64_sl[k][ne]).max() <= 1e-4 * big, k
        assert np.abs(g64[k][ne] - g64_sl[k][ne]).max() == 0                      # the oracle's own weights are exactly zero there
    ob = gr["output_layer.bias"][ne, 0]
    assert np.abs(ob[:od + 1]).max() <= 1e-4 * np.abs(ob).max() and np.abs(ob[od + 1:]).max() > 0
    eng.close()


def test_mopo_shape_vs_fixture():
    g, c = _g("rambo_mopo.npz"), mr.MOPO
    eng = _eng(c)
    st = _model_params(c)
    for k, v in st.items():
        assert np.allclose(synth.digest(v), g[f"init/{k}/digest"], rtol=1e-6, atol=1e-6), k
    eng.set_params(0, st)
    eng.set_scaler(0, g["scaler_mu"], g["scaler_std"])
    eng.set_elites(0, c["elite_idx"])
    eng.adv_configure(c["adv_lr"], adv_weight=c["adv_weight"], rollout_rows=c["Ba"], sl_rows=c["Bs"])
    d = mr.step_inputs(c, 0)
    nxt, rew, _ = _fwd(eng, d, d["eps"], g["step0/model_idx"])
    assert np.abs(nxt[0] - g["step0/next_obs"]).max() <= 1e-5 * np.abs(g["step0/next_obs"]).max() + 1e-6
    m = eng.adv_update(g["step0/advantage"][None])[0]
    ref = dict(zip(mr.LOSS_KEYS, g["step0/losses"]))
    for k, v in zip(("all_loss", "sl_loss", "adv_loss", "adv_log_prob"), m):
        print(k, float(v), ref[k], abs(v - ref[k]) / abs(ref[k]))
    for k, v in zip(("all_loss", "sl_loss", "adv_loss", "adv_log_prob"), m):
        assert abs(v - ref[k]) <= 1e-4 * abs(ref[k]), (k, v, ref[k])
    for k, v in eng.get_params(0).items():
        dg, r = synth.digest(v), g[f"step0/{k}/digest"]
        assert np.abs(dg[2:] - r[2:]).max() <= 2e-5 + 1e-4 * np.abs(r[2:]).max(), k
    eng.close()


def test_stability_where_every_elite_underflows():
    """teacher-forced noise of +-24 standard deviations: every elite's lp_k is below -800 on every row, where the reference's
    exp(lp_k) is 0 in double and its log_prob -inf.  Metrics, gradients and parameters stay finite and match the float64 log-sum-exp.
    Tolerances: lp_k is a sum of fp32 terms, so its absolute error is about 8 ulp of max|lp_k| (e_lp = 8 * 2^-23 * max|lp_k|);
    log_prob carries that error (relative 1e-5 is far above it); the mixture weights exp(lp_k - max) carry it as a RELATIVE error, so the
    gradients are held to (1e-4 + 2 e_lp) of their max."""
    g, c = _g("rambo_tiny.npz"), mr.TINY
    rng = np.random.default_rng(7)
    Ba, Bs, K, D = c["Ba"], c["Bs"], c["K"], c["obs_dim"] + 1
    st = _state(g, "init")
    rows = _random_rows(rng, c, Ba, Bs)
    eps = (24.0 * rng.choice([-1.0, 1.0], size=(K, Ba, D))).astype(np.float32)
    midx = rng.choice(c["elite_idx"], size=Ba)
    adv = _normalised(rng, Ba)
    f = ro.step_forward(st, g["scaler_mu"], g["scaler_std"], rows, eps, midx, F64)
    m64, g64 = ro.step_grads(f, c["elite_idx"], adv, 1.0, c["decays"], F64)
    z = f["sample"].astype(F64)[None] - f["mean"][:, :Ba]
    lp = (-(z * z) / (2 * np.exp(f["lv"][:, :Ba])) - 0.5 * f["lv"][:, :Ba] - ro.LOG_SQRT_2PI).sum(-1)
    assert lp[c["elite_idx"]].max() < -800
    with np.errstate(divide="ignore"):
        assert np.all(np.isneginf(np.log(np.exp(lp[c["elite_idx"]]).sum(0))))          # the reference's formula
    e_lp = 8 * 2.0 ** -23 * np.abs(lp).max()
    eng = _tiny_engine(g, c, 1.0)
    _fwd(eng, rows, eps, midx)
    m = eng.adv_update(adv[None])[0]
    assert np.all(np.isfinite(m)), m
    for k, i in (("adv_log_prob", 3), ("adv_loss", 2)):
        print(k, float(m[i]), m64[k])
    assert abs(m[3] - m64["adv_log_prob"]) <= 1e-5 * abs(m64["adv_log_prob"])
    gr, p = eng.debug_grads(0), eng.get_params(0)
    for k in g64:
        assert np.all(np.isfinite(gr[k])) and np.all(np.isfinite(p[k])), k
        err = _rel(gr[k], g64[k])
        print(k, "grad err / max", err, "bound", 1e-4 + 2 * e_lp)
        assert err <= 1e-4 + 2 * e_lp, (k, err)
    eng.close()


def test_two_runs_equal_two_single_runs_and_inactive_run_unchanged():
    c = mr.TINY
    rng = np.random.default_rng(21)
    Ba, Bs, K, D = c["Ba"], c["Bs"], c["K"], c["obs_dim"] + 1
    runs = []
    for r in range(2):
        runs.append(dict(st=_model_params(c, seed=300 + r), el=[[2, 0], [1, 2]][r], rows=_random_rows(rng, c, Ba, Bs),
                         eps=rng.normal(size=(K, Ba, D)).astype(np.float32), adv=_normalised(rng, Ba),
                         mu=rng.normal(size=5).astype(np.float32), sd=rng.uniform(0.5, 2, size=5).astype(np.float32)))
        runs[r]["midx"] = rng.choice(runs[r]["el"], size=Ba)
    single = []
    for r in range(2):
        e1 = _eng(c)
        u = runs[r]
        e1.set_params(0, u["st"]); e1.set_scaler(0, u["mu"], u["sd"]); e1.set_elites(0, u["el"])
        e1.adv_configure(c["adv_lr"], adv_weight=1.0, rollout_rows=Ba, sl_rows=Bs)
        nxt, rew, _ = _fwd(e1, u["rows"], u["eps"], u["midx"])
        m = e1.adv_update(u["adv"][None])[0]
        single.append((nxt[0], rew[0], m, e1.get_params(0)))
        e1.close()
    e2 = _eng(c, n_runs=2)
    for r, u in enumerate(runs):
        e2.set_params(r, u["st"]); e2.set_scaler(r, u["mu"], u["sd"]); e2.set_elites(r, u["el"])
    e2.adv_configure(c["adv_lr"], adv_weight=1.0, rollout_rows=Ba, sl_rows=Bs)
    stack = lambda k: np.stack([u[k] for u in runs])
    args = [np.stack([u["rows"][k] for u in runs]) for k in ROWS]
    nxt, rew, _ = e2.adv_forward(*args, stack("eps"), stack("midx"))
    m = e2.adv_update(stack("adv"))
    for r in range(2):
        assert np.abs(nxt[r] - single[r][0]).max() <= 1e-5 * np.abs(single[r][0]).max()
        assert np.abs(rew[r] - single[r][1]).max() <= 1e-5 * np.abs(single[r][1]).max()
        assert np.abs(m[r] - single[r][2]).max() <= 1e-5 * np.abs(single[r][2]).max(), (m[r], single[r][2])
        for k, v in e2.get_params(r).items():
            assert np.abs(v - single[r][3][k]).max() <= 1e-5 * max(np.abs(v).max(), 1e-3), (r, k)
    before = (e2.get_params(1), e2.adv_adam_state(1))
    p0 = e2.get_params(0)
    e2.adv_forward(*args, stack("eps"), stack("midx"))
    m = e2.adv_update(stack("adv"), active=np.array([1, 0], np.int32))
    assert np.all(m[1] == 0) and m[0][0] != 0
    p1, (m1, v1, t1) = e2.get_params(1), e2.adv_adam_state(1)
    for k in p1:
        assert np.array_equal(p1[k].view(np.uint32), before[0][k].view(np.uint32)), k
        assert np.array_equal(m1[k].view(np.uint32), before[1][0][k].view(np.uint32)), k
        assert np.array_equal(v1[k].view(np.uint32), before[1][1][k].view(np.uint32)), k
    assert t1 == before[1][2] == 1 and e2.adv_adam_state(0)[2] == 2
    assert not np.array_equal(e2.get_params(0)["backbones.0.weight"], p0["backbones.0.weight"])
    e2.close()


def test_update_without_forward_is_an_error():
    g, c = _g("rambo_tiny.npz"), mr.TINY
    eng = _eng(c)
    adv = np.zeros((1, c["Ba"]), np.float32)
    eng.adv_rows = (c["Ba"], c["Bs"])                                   # not configured at all
    with pytest.raises(RuntimeError, match="pending forward"):
        eng.adv_update(adv)
    eng.close()
    eng = _tiny_engine(g, c, 1.0)
    with pytest.raises(RuntimeError, match="pending forward"):
        eng.adv_update(adv)
    tag = "w1/step0"
    _fwd(eng, {k: g[f"{tag}/{k}"] for k in ROWS}, g[f"{tag}/eps"], g[f"{tag}/model_idx"])
    eng.adv_update(adv)
    with pytest.raises(RuntimeError, match="pending forward"):        # one update per forward
        eng.adv_update(adv)
    eng.close()


def test_device_rng_forward_statistics():
    """without teacher forcing every chosen member is an elite (both about equally often) and the standardised residuals of the sample
    have mean 0 and variance 1, the checks of test_device_philox_step_statistics"""
    g, c = _g("rambo_tiny.npz"), mr.TINY
    n, Bs, K, D = 20000, 8, c["K"], c["obs_dim"] + 1
    eng = _eng(c, seed=9)
    eng.set_params(0, _state(g, "init"))
    eng.set_scaler(0, g["scaler_mu"], g["scaler_std"])
    eng.set_elites(0, c["elite_idx"])
    eng.adv_configure(c["adv_lr"], adv_weight=1.0, rollout_rows=n, sl_rows=Bs)
    rows = _random_rows(np.random.default_rng(3), c, n, Bs)
    zero = np.zeros((K, n, D), np.float32)
    base = []
    for k in range(K):
        mi = np.full(n, k, np.int64)
        a0, r0, _ = _fwd(eng, rows, zero, mi)
        a1, r1, _ = _fwd(eng, rows, zero + 1, mi)
        s0, s1 = np.concatenate([a0[0], r0[0][:, None]], 1), np.concatenate([a1[0], r1[0][:, None]], 1)
        base.append((s0, s1 - s0))
    nxt, rew, idx = _fwd(eng, rows)
    nxt2, _, _ = _fwd(eng, rows)
    assert not np.array_equal(nxt, nxt2)                                   # the call counter advances the stream
    s, idx = np.concatenate([nxt[0], rew[0][:, None]], 1), idx[0]
    assert set(np.unique(idx)) == set(c["elite_idx"])
    assert abs((idx == c["elite_idx"][0]).mean() - 0.5) < 0.02
    i = np.arange(n)
    m0 = np.stack([b[0] for b in base])[idx, i]
    sd = np.stack([b[1] for b in base])[idx, i]
    e = (s - m0) / sd
    print("eps mean", e.mean(), "var", e.var())
    assert abs(e.mean()) < 0.02 and abs(e.var() - 1.0) < 0.05, (e.mean(), e.var())
    eng.close()


def test_rambo_policy_end_to_end(tmp_path):
    """MBPolicyTrainer's host loop with RAMBOPolicy on the point-mass task: pretrain, a few hundred policy steps with an adversarial
    model update every 100 steps, the logged keys, the dynamics moving, select_action's scaler and the pretrain checkpoint"""
    from offlinerlkit.buffer import ReplayBuffer
    from offlinerlkit.dynamics import EnsembleDynamics
    from offlinerlkit.modules import ActorProb, Critic, EnsembleDynamicsModel, TanhDiagGaussian
    from offlinerlkit.nets import MLP
    from offlinerlkit.policy import RAMBOPolicy
    from offlinerlkit.policy_trainer import MBPolicyTrainer
    from offlinerlkit.utils.logger import Logger
    from offlinerlkit.utils.scaler import StandardScaler
    from offlinerlkit.utils.termination_fns import get_termination_fn
    from test_gpu_training import AD, DEV, HID, OD, PointMass, make_dataset
    torch.manual_seed(3)
    np.random.seed(3)
    ds = make_dataset(n_episodes=200)
    logger = Logger(str(tmp_path), {"consoleout_backup": "stdout", "policy_training_progress": "csv", "dynamics_training_progress": "csv"})
    real = ReplayBuffer(len(ds["rewards"]), (OD,), np.float32, AD, np.float32, device=DEV)
    real.load_dataset(ds)
    obs_mean, obs_std = real.normalize_obs()
    model = EnsembleDynamicsModel(OD, AD, [64, 64], num_ensemble=5, num_elites=3, weight_decays=[2.5e-5, 5e-5, 1e-4], device=DEV)
    dyn = EnsembleDynamics(model, torch.optim.Adam(model.parameters(), lr=1e-3), StandardScaler(), get_termination_fn("point2denv"))
    dyn.train(real.sample_all(), logger, max_epochs=10, max_epochs_since_update=5)

    def policy(adv_weight, steps=24):
        adam = lambda m, lr: torch.optim.Adam(m.parameters(), lr=lr)
        actor = ActorProb(MLP(OD, HID), TanhDiagGaussian(HID[-1], AD, unbounded=True, conditioned_sigma=True), DEV)
        c1, c2 = Critic(MLP(OD + AD, HID), DEV), Critic(MLP(OD + AD, HID), DEV)
        return RAMBOPolicy(dyn, actor, c1, c2, adam(actor, 1e-3), adam(c1, 1e-3), adam(c2, 1e-3), adam(model, 3e-4), tau=0.005, gamma=0.95,
                           alpha=0.2, adv_weight=adv_weight, adv_train_steps=steps, adv_rollout_batch_size=64, adv_rollout_length=3,
                           scaler=StandardScaler(obs_mean, obs_std), device=DEV)

    pol = policy(3e-4)
    # pretrain before the engine is bound: the BC loss falls and the checkpoint reloads
    data = real.sample_all()
    pol.pretrain(data, 4, 256, 1e-3, logger)
    assert pol.pretrain_losses[-1] < pol.pretrain_losses[0], pol.pretrain_losses
    assert (tmp_path / "model" / "rambo_pretrain.pth").exists()
    obs = data["observations"][:16]
    a_pre = pol.select_action(obs, deterministic=True)
    with torch.no_grad():
        for p in pol.actor.parameters():
            p.add_(0.1)
    assert not np.array_equal(pol.select_action(obs, deterministic=True), a_pre)
    pol.load(str(tmp_path / "model"))
    assert np.array_equal(pol.select_action(obs, deterministic=True), a_pre)
    # select_action applies the scaler; the parent's does not
    from offlinerlkit.policy import MOPOPolicy
    assert np.array_equal(a_pre, MOPOPolicy.select_action(pol, pol.scaler.transform(obs), True))

    class Env(PointMass):
        def get_normalized_score(self, x):
            return x / 20.0

    fake = ReplayBuffer(2 * 500 * 3, (OD,), np.float32, AD, np.float32, device=DEV)
    w_before = model.backbones[0].weight.detach().clone()
    MBPolicyTrainer(pol, Env(1000), real, fake, logger, (100, 500, 3), epoch=1, step_per_epoch=200, batch_size=128, real_ratio=0.5,
                    eval_episodes=2, dynamics_update_freq=100).train()
    rows = [ln.split(",") for ln in open(tmp_path / "record" / "policy_training_progress.csv").read().strip().split("\n")]
    keys = {"adv_dynamics_update/" + k for k in mr.LOSS_KEYS}
    assert keys <= set(rows[0]), keys - set(rows[0])
    for k in keys:
        assert np.isfinite(float(rows[1][rows[0].index(k)])), k
    assert not torch.equal(model.backbones[0].weight.detach(), w_before)
    # pretrain after the engine is bound trains the engine's live actor (the trainer closed its logger: a plain one here)
    class Log:
        model_dir = str(tmp_path / "model")
        log = staticmethod(lambda s: None)
    pol.pretrain(data, 2, 256, 1e-3, Log)
    assert pol.pretrain_losses[-1] < pol.pretrain_losses[0]
    out = pol.update_dynamics(real)
    assert set(out) == keys and all(np.isfinite(v) for v in out.values())
    # adv_weight 0: plain supervised steps on dataset rows, so the logged sl_loss does not rise over the updates
    pol0 = policy(0.0, steps=30)
    sl = [pol0.update_dynamics(real)["adv_dynamics_update/sl_loss"] for _ in range(4)]
    print("sl_loss over the updates", sl)
    assert sl[-1] <= sl[0], sl
