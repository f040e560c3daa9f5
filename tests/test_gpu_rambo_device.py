"""GPU: RAMBO's model update on the device -- the advantage on the policy engine (orl_engine_adv_advantage, csrc/kernels.h k_adv_*)
against the reference's fixture (tests/golden/rambo_adv_tiny.npz) and float64, the device loop (orl_rambo_update_dynamics) against the
separate calls it strings together, its refusals, and RAMBOPolicy.update_dynamics_device / MBPolicyTrainer(fused=True) end to end."""
import numpy as np
import pytest
import torch

import make_rambo_golden as mr
import rambo_adv_refs as ar

pytestmark = pytest.mark.gpu
F64 = np.float64
HOPPER = 2
LOOP_TAPS = ("loop.obs", "loop.act", "loop.sl_obs", "loop.sl_act", "loop.sl_next_obs", "loop.sl_rew", "loop.next_obs", "loop.reward")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _rel(a, b):
    return float(np.abs(np.asarray(a, F64) - np.asarray(b, F64)).max() / max(np.abs(np.asarray(b, F64)).max(), 1e-300))


def _sac(od=3, ad=2, hidden=(16, 16), n_runs=1, seed=5, algo="sac", **over):
    from offlinerlkit import _engine
    o = dict(obs_dim=od, act_dim=ad, hidden=list(hidden), batch_size=32, n_runs=n_runs, seed=seed, gamma=0.99, auto_alpha=0, alpha=0.2)
    o.update(over)
    return _engine.Engine(_engine.default_config(algo, **o))


def _random_nets(eng, run, seed, scale=0.4):
    """every net of the run <- normal(0, scale) in state_dict order; the targets get their own draws (the advantage must not read them)"""
    rng = np.random.default_rng(seed)
    for nid in range(5):
        eng.set_net(run, nid, {k: (scale * rng.normal(size=v.shape)).astype(np.float32) for k, v in eng.get_net(run, nid).items()})


def _fixture_engine():
    from offlinerlkit import _engine
    g = ar.fixture()
    eng = _sac(gamma=float(g["gamma"]), alpha=float(g["alpha"]))
    for nid, name in ((_engine.NET_ACTOR, "actor"), (_engine.NET_CRITIC1, "critic1"), (_engine.NET_CRITIC2, "critic2")):
        eng.set_net(0, nid, ar.net_params(g, name))
    rng = np.random.default_rng(0)      # targets that are NOT the critics: the advantage reads the live ones
    for nid in (_engine.NET_CRITIC1_OLD, _engine.NET_CRITIC2_OLD):
        eng.set_net(0, nid, {k: rng.normal(size=v.shape).astype(np.float32) for k, v in eng.get_net(0, nid).items()})
    return eng, g


def _taps(eng, run=0, names=("adv.term", "adv.q_next", "adv.q_base", "adv.logp_next", "adv.raw", "adv.norm")):
    return {n: eng.debug_read(run, n) for n in names}


@pytest.mark.parametrize("ent", [0, 1])
def test_advantage_vs_reference_fixture(ent):
    """adv.q_next (after the entropy term when it is on), adv.q_base and adv.raw within 1e-4 of the fixture's largest entry (the
    project's parity bar, the form of test_gpu_rambo.py's _rel); adv.term equals the reference's terminals exactly"""
    eng, g = _fixture_engine()
    for step in (0, 1):
        t = f"ent{ent}/step{step}/"
        adv, st = eng.adv_advantage(g[t + "obs"][None], g[t + "act"][None], g[t + "next_obs"][None], g[t + "reward"][None], HOPPER, bool(ent))
        tp = _taps(eng)
        assert np.array_equal(tp["adv.term"], g[t + "terminals"])
        assert 0.25 <= tp["adv.term"].mean() <= 0.75
        for tap, ref in (("adv.q_next", "next_q"), ("adv.q_base", "value_baseline"), ("adv.raw", "raw"), ("adv.logp_next", "logp_next")):
            err = _rel(tp[tap], g[t + ref])
            print(ent, step, tap, "err / max", err)
            assert err < 1e-4, (tap, err)
        assert _same(adv[0], tp["adv.norm"])
        want = ar.normalise(tp["adv.raw"])
        assert np.abs(adv[0] - want).max() <= 1e-5 * np.abs(want).max()
        # the reference's own normalised advantage: its raw differs from ours by the parity bar, amplified by max|raw| / std
        amp = np.abs(g[t + "raw"]).max() / g[t + "raw"].astype(F64).std(ddof=1)
        assert np.abs(adv[0] - g[t + "advantage"]).max() <= 1e-4 * amp * 2 + 1e-5, amp
        assert abs(st[0, 0] - tp["adv.norm"].astype(F64).mean()) <= 1e-6 and abs(st[0, 1] - tp["adv.raw"].astype(F64).std(ddof=1)) <= 1e-5 * st[0, 1]
    eng.close()


def _rows(rng, Ba, od, ad, rew_mean=0.0):
    obs = rng.normal(size=(Ba, od)).astype(np.float32)
    obs[:, 0] = 0.7 + 0.3 * rng.normal(size=Ba)
    obs[:, 1] = 0.15 * rng.normal(size=Ba)
    nxt = (obs + 0.1 * rng.normal(size=(Ba, od))).astype(np.float32)
    return obs, rng.uniform(-1, 1, size=(Ba, ad)).astype(np.float32), nxt, (rew_mean + rng.normal(size=Ba)).astype(np.float32)


@pytest.mark.parametrize("Ba,rew_mean", [(2, 0.0), (37, 0.0), (1030, 0.0), (37, 400.0), (1030, 400.0)])
def test_normalisation_vs_float64(Ba, rew_mean):
    """adv.norm against (x - mean) / (std + 1e-6) in float64 from the engine's own adv.raw.

    Bound c * 2^-24 * (1 + |want| + mean|raw| / std), c from k_adv_norm as written: a sum is block_sum256 over per-thread partial sums.
    A thread adds its ceil(Ba / 256) rows one after the other (ceil(Ba / 256) - 1 additions), the __shfl_down tree adds across the
    64 lanes in 6 additions, thread-uniform code adds the four wave sums from LDS in 3: the longest chain a partial sum passes through
    is n = ceil(Ba / 256) - 1 + 6 + 3 additions, each with relative rounding error at most 2^-24 of a partial sum bounded by sum|raw|.
    So |mean error| <= n 2^-24 mean|raw| (+ one rounding of the division), which the normalisation divides by std: the
    mean|raw| / std term.  The spread's own error ((n + 2) roundings on a sum of squares, halved by the square root) and the final
    subtraction and division scale |want|; the 1 covers the 1e-6 in the denominator and values near zero.  c = 4 n leaves the
    factor 4 for those second terms: Ba = 2, 37: n = 9, c = 36; Ba = 1030: n = 13, c = 52.
    rew_mean 400: the raw mean is more than 100 times its spread (asserted) -- the case where a one-pass variance would cancel."""
    eng = _sac()
    _random_nets(eng, 0, 11)
    rng = np.random.default_rng(100 + Ba)
    obs, act, nxt, rew = _rows(rng, Ba, 3, 2, rew_mean)
    adv, st = eng.adv_advantage(obs[None], act[None], nxt[None], rew[None], HOPPER, False)
    tp = _taps(eng)
    raw = tp["adv.raw"].astype(F64)
    assert raw.shape == (Ba,) and np.all(np.isfinite(raw))
    sd = raw.std(ddof=1)
    want = (raw - raw.mean()) / (sd + 1e-6)
    ratio = np.abs(raw).mean() / sd
    if rew_mean:
        assert abs(raw.mean()) >= 100 * sd, (raw.mean(), sd)
    n = -(-Ba // 256) - 1 + 6 + 3
    bound = 4 * n * 2.0 ** -24 * (1 + np.abs(want) + ratio)
    err = np.abs(tp["adv.norm"].astype(F64) - want)
    print("Ba", Ba, "mean|raw| / std", ratio, "worst err / bound", (err / bound).max())
    assert np.all(err <= bound), (err / bound).max()
    assert _same(adv[0], tp["adv.norm"])
    assert abs(st[0, 1] - sd) <= 4 * n * 2.0 ** -24 * (sd + ratio * sd)
    assert abs(st[0, 0]) <= 4 * n * 2.0 ** -24 * (1 + np.abs(want).mean() + ratio)
    eng.close()


def test_rows_below_two_and_other_engines_are_refused():
    eng = _sac()
    z = lambda *s: np.zeros(s, np.float32)
    with pytest.raises(RuntimeError, match="rows must be >= 2"):
        eng.adv_advantage(z(1, 1, 3), z(1, 1, 2), z(1, 1, 3), z(1, 1), HOPPER)
    with pytest.raises(RuntimeError, match="unknown termination kind"):
        eng.adv_advantage(z(1, 4, 3), z(1, 4, 2), z(1, 4, 3), z(1, 4), 99)
    with pytest.raises(RuntimeError, match="reads observation column 26"):
        eng.adv_advantage(z(1, 4, 3), z(1, 4, 2), z(1, 4, 3), z(1, 4), 6)
    eng.close()
    mob = _sac(algo="mobile")
    with pytest.raises(RuntimeError, match="not a SAC engine"):
        mob.adv_advantage(z(1, 4, 3), z(1, 4, 2), z(1, 4, 3), z(1, 4), HOPPER)
    mob.close()


def _state(eng, run=0):
    from offlinerlkit import _engine
    st = eng.optimizer_state(run)
    return ({n: eng.get_net(run, n) for n in range(5)}, st)


def _state_equal(a, b):
    for n in a[0]:
        for k in a[0][n]:
            assert _same(a[0][n][k], b[0][n][k]), (n, k)
    assert a[1]["step"] == b[1]["step"] and a[1]["scalars"] == b[1]["scalars"]
    for n in a[1]["adam"]:
        assert _same(a[1]["adam"][n][0], b[1]["adam"][n][0]) and _same(a[1]["adam"][n][1], b[1]["adam"][n][1]), n


def test_run_batching_and_isolation():
    """an R = 2 engine gives per run the bytes of two one-run engines (Ba grows between the calls: the workspaces regrow), and the
    call leaves parameters, Adam state, scalars, step count and the next orl_step of the engine as those of a twin that never made it"""
    rng = np.random.default_rng(3)
    e2 = _sac(n_runs=2, auto_alpha=1)
    for r in range(2):
        _random_nets(e2, r, 20 + r)
    for Ba in (5, 37, 300):
        rows = [_rows(rng, Ba, 3, 2) for _ in range(2)]
        both = [np.stack([rows[0][i], rows[1][i]]) for i in range(4)]
        adv2, st2 = e2.adv_advantage(*both, HOPPER, True)
        t2 = [_taps(e2, r) for r in range(2)]
        for r in range(2):
            e1 = _sac(auto_alpha=1)
            _random_nets(e1, 0, 20 + r)
            adv1, st1 = e1.adv_advantage(*[x[None] for x in rows[r]], HOPPER, True)
            t1 = _taps(e1)
            assert _same(adv1[0], adv2[r]) and _same(st1[0], st2[r]), (Ba, r)
            for k in t1:
                assert _same(t1[k], t2[r][k]), (Ba, r, k)
            e1.close()
    e2.close()
    # isolation: twins, one step each (nonzero Adam state), then one of them computes advantages
    B = 32
    batch = dict(observations=rng.normal(size=(1, B, 3)), actions=rng.uniform(-1, 1, size=(1, B, 2)), next_observations=rng.normal(size=(1, B, 3)),
                 rewards=rng.normal(size=(1, B)), terminals=(rng.uniform(size=(1, B)) < 0.2).astype(np.float32))
    twins = [_sac(auto_alpha=1), _sac(auto_alpha=1)]
    for e in twins:
        _random_nets(e, 0, 40)
        e.step(batch, None)
    a, b = twins
    obs, act, nxt, rew = _rows(rng, 37, 3, 2)
    a.adv_advantage(obs[None], act[None], nxt[None], rew[None], HOPPER, True)
    a.adv_advantage(obs[None, :9], act[None, :9], nxt[None, :9], rew[None, :9], HOPPER, False)
    _state_equal(_state(a), _state(b))
    ma, mb = a.step(batch, None), b.step(batch, None)
    assert _same(ma, mb), (ma, mb)
    _state_equal(_state(a), _state(b))
    for e in twins:
        e.close()


# ---- the device loop ----
TINY_LOOP = dict(od=3, ad=2, hidden=mr.TINY["hidden"], K=3, elites=2, elite_idx=[2, 0], decays=mr.TINY["decays"], pol_hidden=(16, 16), rows=37,
                 adv_weight=1.0, adv_lr=1e-3)
MOPO_LOOP = dict(od=17, ad=6, hidden=[200, 200, 200, 200], K=7, elites=5, elite_idx=[6, 1, 3, 0, 4], decays=mr.MOPO["decays"],
                 pol_hidden=(256, 256), rows=256, adv_weight=3e-4, adv_lr=3e-4)
_model_cache = {}


def _dyn_params(c):
    key = (c["od"], c["ad"], tuple(c["hidden"]))
    if key not in _model_cache:
        from offlinerlkit.modules import EnsembleDynamicsModel
        torch.manual_seed(17)
        m = EnsembleDynamicsModel(c["od"], c["ad"], c["hidden"], c["K"], c["elites"], weight_decays=c["decays"])
        p = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items() if k != "elites"}
        # a model as sure of itself as a trained one (std <= e^-2): with the initial max_logvar of 0.5 the sampled next observations
        # scatter by about one unit per dimension and nearly every row fails the hopper test
        p["max_logvar"] = np.full_like(p["max_logvar"], -4.0)
        _model_cache[key] = p
    return _model_cache[key]


def _dataset(c, n=400):
    rng = np.random.default_rng(77)
    obs, act, nxt, rew = _rows(rng, n, c["od"], c["ad"])
    return obs, act, nxt, rew, (rng.uniform(size=n) < 0.1).astype(np.float32)


def _twin(c, configure=True, rows=None, eng_over=None, dyn_over=None, load=True, buf_dims=None):
    """(policy engine, dynamics, buffer) in a fixed initial state: every twin of a shape starts from the same bytes and counters"""
    from offlinerlkit import _engine
    eng = _sac(c["od"], c["ad"], c["pol_hidden"], seed=9, **(eng_over or {}))
    for r in range(eng.n_runs):
        _random_nets(eng, r, 60, scale=0.4 if c["pol_hidden"][0] < 64 else 0.05)
    o = dict(obs_dim=c["od"], act_dim=c["ad"], hidden=c["hidden"], num_ensemble=c["K"], num_elites=c["elites"], weight_decay=c["decays"], lr=1e-3,
             batch_size=64, seed=13)
    o.update(dyn_over or {})
    dyn = _engine.Dynamics(_engine.default_dyn_config(**o))
    in_dim = c["od"] + c["ad"]
    for r in range(dyn.n_runs):
        dyn.set_params(r, _dyn_params(c))
        dyn.set_scaler(r, np.full(in_dim, 0.1, np.float32), np.full(in_dim, 1.3, np.float32))
        dyn.set_elites(r, c["elite_idx"])
    if configure:
        n = c["rows"] if rows is None else rows
        dyn.adv_configure(c["adv_lr"], adv_weight=c["adv_weight"], rollout_rows=n, sl_rows=n)
    od, ad = buf_dims or (c["od"], c["ad"])
    buf = _engine.DeviceBuffer(od, ad)
    if load:
        d = _dataset(dict(c, od=od, ad=ad))
        buf.load(d[0], d[1], d[2], d[3], d[4])
    return eng, dyn, buf


def _close(*objs):
    for o in objs:
        o.close()


def _loop(tw, c, segments, ent=True, rows=None, kind=HOPPER):
    eng, dyn, buf = tw
    m, ms = eng.rambo_update_dynamics(dyn, buf, c["rows"] if rows is None else rows, kind, ent, segments)
    assert ms > 0
    return np.array([m[k] for k in ("all_loss", "sl_loss", "adv_loss", "adv_advantage", "adv_log_prob")], np.float32)


def _loop_taps(eng, c):
    od, ad, n = c["od"], c["ad"], c["rows"]
    shape = {"loop.obs": (n, od), "loop.act": (n, ad), "loop.sl_obs": (n, od), "loop.sl_act": (n, ad), "loop.sl_next_obs": (n, od),
             "loop.sl_rew": (n,), "loop.next_obs": (n, od), "loop.reward": (n,)}
    return {k: eng.debug_read(0, k).reshape(shape[k]) for k in LOOP_TAPS}


def _replay(tw, c, tp, ent=True):
    """one step through the separate entries on the tapped rows -> (next_obs, reward, advantage, the five values)"""
    eng, dyn, _ = tw
    nxt, rew, _ = dyn.adv_forward(tp["loop.obs"][None], tp["loop.act"][None], tp["loop.sl_obs"][None], tp["loop.sl_act"][None],
                                  tp["loop.sl_next_obs"][None], tp["loop.sl_rew"][None], None, None)
    adv, st = eng.adv_advantage(tp["loop.obs"][None], tp["loop.act"][None], nxt, rew, HOPPER, ent)
    m = dyn.adv_update(adv)[0]
    return nxt[0], rew[0], adv[0], np.array([m[0], m[1], m[2], st[0, 0], m[3]], np.float32)


def _dyn_state(dyn):
    p = dyn.get_params(0)
    am, av, t = dyn.adv_adam_state(0)
    return p, am, av, t


def _dyn_state_same(a, b):
    assert a[3] == b[3], (a[3], b[3])
    for i in range(3):
        for k in a[i]:
            assert _same(a[i][k], b[i][k]), (i, k)


@pytest.mark.parametrize("shape", ["tiny", "mopo"])
def test_loop_equals_the_separate_calls(shape):
    """twin A runs one segment of one step; an identical twin fed A's tapped rows through orl_dynadv_forward (device draws at the same
    call counter), orl_engine_adv_advantage and orl_dynadv_update ends with the same bytes everywhere.  Tiny shape also: twin B runs
    one segment of TWO steps from the same state -- its second step starts where A's first ended, and its means are the mean of the
    two replayed steps up to the order of two fp32 additions (2^-22 relative)."""
    c = TINY_LOOP if shape == "tiny" else MOPO_LOOP
    A, R = _twin(c), _twin(c)
    before = _dyn_state(A[1])
    mA = _loop(A, c, [1])
    tA = _loop_taps(A[0], c)
    assert 0.1 <= A[0].debug_read(0, "adv.term").mean() <= 0.9          # both kinds of rows went through the loop
    assert tA["loop.sl_obs"].std() > 0 and not np.array_equal(tA["loop.obs"], tA["loop.sl_obs"])     # two draws of the buffer
    nxt, rew, adv, m1 = _replay(R, c, tA)
    assert _same(nxt, tA["loop.next_obs"]) and _same(rew, tA["loop.reward"])
    assert _same(adv, A[0].debug_read(0, "adv.norm"))
    assert _same(m1, mA), (m1, mA)
    sA, sR = _dyn_state(A[1]), _dyn_state(R[1])
    _dyn_state_same(sA, sR)
    assert sA[3] == 1 and not _same(sA[0]["backbones.0.weight"], before[0]["backbones.0.weight"])
    if shape == "tiny":
        Bt = _twin(c)
        mB = _loop(Bt, c, [2])
        tB = _loop_taps(Bt[0], c)
        assert _same(tB["loop.obs"], tA["loop.next_obs"])
        assert not _same(tB["loop.act"], tA["loop.act"]) and not _same(tB["loop.sl_obs"], tA["loop.sl_obs"])
        nxt2, rew2, adv2, m2 = _replay(R, c, tB)
        assert _same(nxt2, tB["loop.next_obs"]) and _same(adv2, Bt[0].debug_read(0, "adv.norm"))
        _dyn_state_same(_dyn_state(Bt[1]), _dyn_state(R[1]))
        want = (m1.astype(F64) + m2.astype(F64)) / 2
        scale = np.maximum(np.abs(m1), np.abs(m2)).astype(F64)
        assert np.all(np.abs(mB - want) <= 2.0 ** -22 * scale), (mB, want)
        # two segments of one step: the second starts from a fresh draw, not from the first one's next observations
        Ct = _twin(c)
        _loop(Ct, c, [1, 1])
        tC = _loop_taps(Ct[0], c)
        assert not _same(tC["loop.obs"], tA["loop.next_obs"]) and _dyn_state(Ct[1])[3] == 2
        _close(*Bt, *Ct)
    _close(*A, *R)


def test_loop_refusals_come_before_any_launch():
    """every refusal is an error, and the twin that met all of them then runs the loop to the bytes of a fresh twin: no parameter,
    optimizer step, draw counter of the dynamics or of the buffer moved"""
    c = TINY_LOOP
    good = _twin(c)
    eng, dyn, buf = good
    before = _dyn_state(dyn)

    def refused(match, tw, **kw):
        with pytest.raises(RuntimeError, match=match):
            _loop(tw, c, kw.pop("segments", [1]), **kw)

    refused("unknown termination kind", good, kind=99)
    refused("reads observation column 26", good, kind=6)
    refused("configured for 37 rollout and 37 dataset rows", good, rows=36)
    refused("at least one step", good, segments=[1, 0])
    refused("no segments", good, segments=[])
    e2, d2, b2 = _twin(c, eng_over=dict(n_runs=2))
    refused("n_runs == 1", (e2, dyn, buf))
    _close(e2, d2, b2)
    e2, d2, b2 = _twin(c, dyn_over=dict(n_runs=2))
    refused("n_runs == 1", (eng, d2, buf))
    _close(e2, d2, b2)
    e2, d2, b2 = _twin(c, configure=False, load=False)
    refused("orl_dynadv_configure first", (eng, d2, buf))
    refused("empty buffer", (eng, dyn, b2))
    _close(e2, d2, b2)
    e2, d2, b2 = _twin(dict(c, od=4), buf_dims=(3, 3))
    refused("dims", (e2, dyn, buf))
    refused("dims", (eng, d2, buf))
    refused("dims", (eng, dyn, b2))
    _close(e2, d2, b2)
    e2, d2, b2 = _twin(c, rows=1)
    refused("rows must be >= 2", (eng, d2, buf), rows=1)
    _close(e2, d2, b2)
    mob = _sac(algo="mobile", seed=9)
    refused("not a SAC engine", (mob, dyn, buf))
    mob.close()
    _dyn_state_same(_dyn_state(dyn), before)
    fresh = _twin(c)
    m0, m1 = _loop(good, c, [2]), _loop(fresh, c, [2])
    assert _same(m0, m1), (m0, m1)
    t0, t1 = _loop_taps(eng, c), _loop_taps(fresh[0], c)
    for k in LOOP_TAPS:
        assert _same(t0[k], t1[k]), k
    _dyn_state_same(_dyn_state(dyn), _dyn_state(fresh[1]))
    _close(*good, *fresh)


def test_nonfinite_metric_raises_the_health_flag():
    from offlinerlkit import _engine
    c = TINY_LOOP
    tw = _twin(c)
    eng, dyn, buf = tw
    p = dyn.get_params(0)
    p["max_logvar"] = np.full_like(p["max_logvar"], np.nan)
    dyn.set_params(0, p)
    with pytest.warns(_engine.EngineHealthWarning, match="non-finite loss"):
        m = _loop(tw, c, [1])
    assert not np.all(np.isfinite(m)) and int(eng.health()[0]) & _engine.HEALTH_NONFINITE_LOSS
    _close(*tw)


def test_update_dynamics_device_end_to_end(tmp_path):
    """the point-mass set-up of test_gpu_rambo.py's test_rambo_policy_end_to_end.

    The two host ``update_dynamics`` runs at the ends (same seeds, fresh copies of the trained ensemble, one before and one after the
    device loop, the fused trainer and a rebind have been used in the process) are runs of THIS build: their equality shows that the
    device path leaves nothing behind in the process that the host path sees (the redirected stream, draw counters, torch's and
    numpy's generators).  It does not compare with an earlier build; that the host entries compute what they computed before this
    loop existed rests on the fixtures of test_gpu_rambo.py, which are untouched and still met."""
    import copy
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
    trained = copy.deepcopy(model.state_dict())

    def fresh_dynamics():
        """the trained ensemble in a new object: its own engine, draw counters at zero"""
        m = EnsembleDynamicsModel(OD, AD, [64, 64], num_ensemble=5, num_elites=3, weight_decays=[2.5e-5, 5e-5, 1e-4], device=DEV)
        m.load_state_dict(trained)
        d = EnsembleDynamics(m, torch.optim.Adam(m.parameters(), lr=1e-3), StandardScaler(dyn.scaler.mu, dyn.scaler.std),
                             get_termination_fn("point2denv"))
        return m, d

    def policy(d, m, adv_weight, steps=24, seed=5):
        torch.manual_seed(seed)
        adam = lambda mod, lr: torch.optim.Adam(mod.parameters(), lr=lr)
        actor = ActorProb(MLP(OD, HID), TanhDiagGaussian(HID[-1], AD, unbounded=True, conditioned_sigma=True), DEV)
        c1, c2 = Critic(MLP(OD + AD, HID), DEV), Critic(MLP(OD + AD, HID), DEV)
        return RAMBOPolicy(d, actor, c1, c2, adam(actor, 1e-3), adam(c1, 1e-3), adam(c2, 1e-3), adam(m, 3e-4), tau=0.005, gamma=0.95,
                           alpha=0.2, adv_weight=adv_weight, adv_train_steps=steps, adv_rollout_batch_size=64, adv_rollout_length=3,
                           scaler=StandardScaler(obs_mean, obs_std), device=DEV)

    keys = {"adv_dynamics_update/" + k for k in mr.LOSS_KEYS}
    # the host path before the process has used the device loop
    m_h, d_h = fresh_dynamics()
    np.random.seed(8)
    host_before = policy(d_h, m_h, 3e-4).update_dynamics(real)
    assert set(host_before) == keys and all(np.isfinite(v) for v in host_before.values())
    # one device update: the five keys, finite, and the model moved
    pol = policy(dyn, model, 3e-4)
    w_before = model.backbones[0].weight.detach().clone()
    out = pol.update_dynamics_device(real)
    assert set(out) == keys and all(np.isfinite(v) for v in out.values()), out
    assert pol.last_update_dynamics_ms > 0 and model.training is False
    assert not torch.equal(model.backbones[0].weight.detach(), w_before)
    assert dyn._eng.adv_adam_state(0)[2] == 24
    # adv_weight 0: plain supervised steps on dataset rows, so the logged sl_loss does not rise over the updates
    m0, d0 = fresh_dynamics()
    pol0 = policy(d0, m0, 0.0, steps=30)
    sl = [pol0.update_dynamics_device(real)["adv_dynamics_update/sl_loss"] for _ in range(4)]
    print("sl_loss over the device updates", sl)
    assert sl[-1] <= sl[0], sl

    class Env(PointMass):
        def get_normalized_score(self, x):
            return x / 20.0

    fake = ReplayBuffer(2 * 500 * 3, (OD,), np.float32, AD, np.float32, device=DEV)
    w_before = model.backbones[0].weight.detach().clone()
    MBPolicyTrainer(pol, Env(1000), real, fake, logger, (100, 500, 3), epoch=1, step_per_epoch=200, batch_size=128, real_ratio=0.5,
                    eval_episodes=2, dynamics_update_freq=100, fused=True).train()
    rows = [ln.split(",") for ln in open(tmp_path / "record" / "policy_training_progress.csv").read().strip().split("\n")]
    assert keys <= set(rows[0]), keys - set(rows[0])
    for k in keys:
        assert np.isfinite(float(rows[1][rows[0].index(k)])), k
    assert not torch.equal(model.backbones[0].weight.detach(), w_before)
    assert dyn._eng.adv_adam_state(0)[2] == 24 * 3
    # the host path on a second policy from the same seeds, after all of the above: what the first one produced (see the docstring)
    m_h2, d_h2 = fresh_dynamics()
    np.random.seed(8)
    host_after = policy(d_h2, m_h2, 3e-4).update_dynamics(real)
    assert host_after == host_before, (host_before, host_after)
