"""GPU: the fused model-based epoch -- the HBM ring (orl_buffer_reserve / append / read), the termination + stable compaction kernel
(orl_buffer_append_rollout), the two-source minibatch draw inside orl_learn_n (orl_engine_attach_model_buffer), the device rollout
against the host rollout, and MBPolicyTrainer(fused=True) end to end."""
import os
import warnings

import numpy as np
import pytest
import torch
from scipy import stats

import synth
import test_gpu_mb as tm
from helpers import GOLDEN_DIR, clone_state, combo_oracle_setup, mopo_oracle_setup, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODEL_MARK = float(2 ** 23)               # model rows carry rewards 2^23 + i: exact in fp32, disjoint from the real rows' i


# ---- 4. the ring ------------------------------------------------------------------------------------------------------------
def test_ring_append_matches_add_batch():
    from offlinerlkit.buffer import ReplayBuffer
    od, ad, cap = 5, 3, 40
    host = ReplayBuffer(cap, (od,), np.float32, ad, np.float32)
    ring = ReplayBuffer(cap, (od,), np.float32, ad, np.float32, device=DEV)
    dev = ring.reserve_device()
    assert ring.reserve_device() is dev and ring._size == 0 and dev.size() == 0
    rng = np.random.RandomState(0)
    for k, n in enumerate([7, 1, 25, 12, cap, 3, 39, 40, 5]):          # wraps, n == capacity, a single row
        rows = (rng.standard_normal((n, od)).astype(np.float32), rng.standard_normal((n, od)).astype(np.float32),
                rng.standard_normal((n, ad)).astype(np.float32), rng.standard_normal((n, 1)).astype(np.float32),
                (rng.uniform(size=(n, 1)) < 0.3).astype(np.float32))
        host.add_batch(*rows)
        if k % 2:                                                       # device sources
            ring.add_batch(*[torch.tensor(x, device=DEV) for x in rows])
        else:
            ring.add_batch(*rows)
        assert (ring._ptr, ring._size) == (host._ptr, host._size) and dev.size() == host._size
        obs, act, nobs, rew, term = dev.read_rows(0, cap)
        for got, want in ((obs, host.observations), (nobs, host.next_observations), (act, host.actions), (rew, host.rewards),
                          (term, host.terminals)):
            assert np.array_equal(got, want), (k, n)
    host.add(*[x[0] for x in rows])
    ring.add(*[x[0] for x in rows])
    a, b = host.sample_all(), ring.sample_all()
    assert (ring._ptr, ring._size) == (host._ptr, host._size)
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    big = [np.zeros((cap + 1, d), np.float32) for d in (od, od, ad, 1, 1)]
    with pytest.raises(RuntimeError, match="capacity"):
        ring.add_batch(*big)
    with pytest.raises(RuntimeError, match="capacity"):
        dev.append(big[0], big[2], big[1], big[3], big[4])
    # np.random.randint index stream of ReplayBuffer.sample is unchanged by the store
    np.random.seed(4)
    idx = np.random.randint(0, ring._size, size=16)
    np.random.seed(4)
    s1 = ring.sample(16)
    assert np.array_equal(s1["observations"].cpu().numpy(), a["observations"][idx])
    assert np.array_equal(s1["rewards"].cpu().numpy(), a["rewards"][idx])


# ---- 5. termination + stable compaction ----------------------------------------------------------------------------------------
TERM_FIXTURE = {"TERM_NONE": "fn_default", "TERM_HALFCHEETAH": "fn_halfcheetah", "TERM_HOPPER": "fn_hopper", "TERM_WALKER2D": "fn_walker2d",
                "TERM_ANT": "fn_ant", "TERM_HUMANOID": "fn_humanoid", "TERM_PEN": "fn_pen"}


@pytest.mark.parametrize("kind", sorted(TERM_FIXTURE))
def test_append_rollout_terminates_and_compacts_like_the_host(kind):
    from offlinerlkit import _engine
    from offlinerlkit.utils import termination_fns as tf
    g = np.load(os.path.join(GOLDEN_DIR, "mb_termination.npz"))
    obs, act, nobs = g["obs"], g["act"], g["next_obs"]
    done = np.asarray(g[TERM_FIXTURE[kind]]).astype(bool).ravel()
    n, od, ad = obs.shape[0], obs.shape[1], act.shape[1]
    assert n > 256                                   # more than one block: the offsets of the second pass are exercised
    rew = np.linspace(-3.0, 5.0, n).astype(np.float32)
    buf = _engine.DeviceBuffer(od, ad)
    cap = n + 37
    buf.reserve(cap)
    t = lambda x: torch.tensor(x, device=DEV)
    alive = torch.full((n, od), -7.0, device=DEV)
    # two appends: the second one wraps around the ring
    for rep in range(2):
        n_alive, s = buf.append_rollout(getattr(tf, kind), t(obs), t(act), t(nobs), t(rew), alive)
        assert n_alive == int((~done).sum())
        assert abs(s - rew.astype(np.float64).sum()) <= 1e-9 * np.abs(rew).astype(np.float64).sum()
        got = alive[:n_alive].cpu().numpy()
        assert np.array_equal(got.view(np.uint32), nobs[~done].view(np.uint32))          # bit patterns: the fixture has NaNs
        where = (np.arange(n) + rep * n) % cap
        o, a, no, r, te = buf.read_rows(0, cap)
        assert np.array_equal(te[where].ravel(), done.astype(np.float32))
        assert np.array_equal(o[where], obs) and np.array_equal(a[where], act) and np.array_equal(r[where].ravel(), rew)
        assert np.array_equal(no[where].view(np.uint32), nobs.view(np.uint32))
    assert buf.size() == cap
    buf.close()


def test_append_rollout_refuses_kinds_that_read_missing_columns():
    from offlinerlkit import _engine
    from offlinerlkit.utils import termination_fns as tf
    for od, kinds in ((26, [tf.TERM_PEN]), (1, [tf.TERM_HOPPER, tf.TERM_WALKER2D, tf.TERM_PEN])):
        buf = _engine.DeviceBuffer(od, 2)
        buf.reserve(16)
        z = lambda c: torch.zeros((4, c), device=DEV)
        for k in kinds:
            with pytest.raises(RuntimeError, match="column"):
                buf.append_rollout(k, z(od), z(2), z(od), torch.zeros(4, device=DEV), z(od))
        assert buf.append_rollout(tf.TERM_HUMANOID, z(od), z(2), z(od), torch.zeros(4, device=DEV), z(od))[0] == 0      # z = 0 < 1: all done
        with pytest.raises(RuntimeError, match="unknown termination kind"):
            buf.append_rollout(7, z(od), z(2), z(od), torch.zeros(4, device=DEV), z(od))
        buf.close()


# ---- 6. the two-source draw, by provenance ---------------------------------------------------------------------------------------
def _marked_rows(i, od, ad, model):
    """rows whose reward names the source and the row index and whose other columns are a fixed function of both"""
    i = np.asarray(i, np.int64)
    sg = -1.0 if model else 1.0
    obs = sg * (((i[:, None] * (np.arange(od)[None] + 1)) % 97) / 97.0)
    nobs = sg * (((i[:, None] * 3 + np.arange(od)[None]) % 89) / 89.0)
    act = sg * (((i[:, None] + np.arange(ad)[None]) % 13) / 13.0 - 0.5)
    rew = i.astype(np.float64) + (MODEL_MARK if model else 0.0)
    term = (i % 5 == 0).astype(np.float64)
    f = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    return f(obs), f(act), f(nobs), f(rew), f(term)


def _uniform_ok(idx, n, what):
    assert idx.min() >= 0 and idx.max() < n, (what, idx.min(), idx.max())
    counts = np.bincount((idx * 100) // n, minlength=100)
    p = stats.chisquare(counts).pvalue
    assert p > 1e-4, (what, n, p)


@pytest.mark.parametrize("algo,precision", [("sac", 0), ("sac", 1), ("cql", 0), ("cql", 1)])
def test_two_source_draw_by_provenance(algo, precision):
    from offlinerlkit import _engine
    od, ad, B, R, real_rows = 17, 6, 256, 3, 12
    n_real, n_model0, n_more, cap = 5_000, 3_000, 9_000, 20_000
    over = dict(obs_dim=od, act_dim=ad, batch_size=B, n_runs=R, precision=precision, seed=99)
    N = 0
    if algo == "cql":
        N = 4
        over.update(num_repeat_actions=N, with_lagrange=0, cql_real_rows=real_rows, cql_cons_row0=0, cql_cons_rows=B)
    eng = _engine.Engine(_engine.default_config(algo, **over))
    real = _engine.DeviceBuffer(od, ad)
    o, a, no, r, t = _marked_rows(np.arange(n_real), od, ad, False)
    real.load(o, a, no, r, t)
    model = _engine.DeviceBuffer(od, ad)
    model.reserve(cap)
    eng.attach_buffer(real)
    with pytest.raises(RuntimeError, match="real_rows"):
        eng.attach_model_buffer(model, B)
    with pytest.raises(RuntimeError, match="real_rows"):
        eng.attach_model_buffer(model, 0)
    eng.attach_model_buffer(model, real_rows)
    with pytest.raises(RuntimeError, match="model buffer is empty"):
        eng.learn_n(1)
    o, a, no, r, t = _marked_rows(np.arange(n_model0), od, ad, True)
    model.append(o, a, no, r, t)

    def step():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", _engine.EngineHealthWarning)      # (rewards of 2^23 with untrained networks: the losses are huge)
            eng.learn_n(1)
        out = []
        for run in range(R):
            rew = eng.debug_read(run, "b_rew").reshape(B).astype(np.float64)
            is_model = rew >= MODEL_MARK
            assert not is_model[:real_rows].any() and is_model[real_rows:].all(), (run, rew[:real_rows + 2])
            idx = np.where(is_model, rew - MODEL_MARK, rew).astype(np.int64)
            got = dict(o=eng.debug_read(run, "b_obs").reshape(B, od), a=eng.debug_read(run, "b_act").reshape(B, ad),
                       no=eng.debug_read(run, "b_nobs").reshape(B, od), t=eng.debug_read(run, "b_term").reshape(B))
            for lo, hi, mdl in ((0, real_rows, False), (real_rows, B, True)):
                wo, wa, wno, _, wt = _marked_rows(idx[lo:hi], od, ad, mdl)
                assert np.array_equal(got["o"][lo:hi], wo) and np.array_equal(got["a"][lo:hi], wa)
                assert np.array_equal(got["no"][lo:hi], wno) and np.array_equal(got["t"][lo:hi], wt)
            if algo == "cql":
                xc = eng.debug_read(run, "xc").reshape(B + 3 * B * N, -1)
                assert np.array_equal(xc[:B, :od], got["o"]) and np.array_equal(xc[:B, od:od + ad], got["a"])
                rep = np.repeat(got["o"], N, axis=0)
                for j in range(3):
                    assert np.array_equal(xc[B + j * B * N:B + (j + 1) * B * N, :od], rep)
            out.append(idx)
        return np.stack(out)                                            # (runs, B)
    try:
        first = [step() for _ in range(40)]
        assert max(x[:, real_rows:].max() for x in first) < n_model0 and max(x[:, :real_rows].max() for x in first) < n_real
        # the ring grows; the captured graph is replayed without re-attaching and reads the new size from the device cell
        o, a, no, r, t = _marked_rows(np.arange(n_model0, n_model0 + n_more), od, ad, True)
        model.append(o, a, no, r, t)
        n_model = n_model0 + n_more
        second = [step() for _ in range(200)]
        allidx = np.stack(second)                                       # (steps, runs, B)
        m_idx, r_idx = allidx[:, :, real_rows:].ravel(), allidx[:, :, :real_rows].ravel()
        assert m_idx.max() < n_model and (m_idx >= n_model0).mean() > 0.6             # rows of the new range appear (3/4 of the ring)
        _uniform_ok(m_idx, n_model, "model source")
        _uniform_ok(r_idx, n_real, "real source")
        flat = allidx.reshape(-1, B)
        assert len({tuple(v) for v in flat}) == flat.shape[0]           # no run / step repeats another's index vector
        assert eng.step_count() == 240
    finally:
        eng.close(); real.close(); model.close()


def test_combo_learn_n_needs_the_engines_real_rows():
    from offlinerlkit import _engine
    od, ad, B = 5, 3, 16
    eng = _engine.Engine(_engine.default_config("cql", obs_dim=od, act_dim=ad, hidden=[32, 32], batch_size=B, num_repeat_actions=3, with_lagrange=0,
                                                cql_real_rows=8, cql_cons_row0=0, cql_cons_rows=B))
    real, model = _engine.DeviceBuffer(od, ad), _engine.DeviceBuffer(od, ad)
    real.load(*_marked_rows(np.arange(100), od, ad, False))
    model.reserve(100)
    model.append(*_marked_rows(np.arange(50), od, ad, True))
    eng.attach_buffer(real)
    eng.attach_model_buffer(model, 4)
    try:
        with pytest.raises(RuntimeError, match="cql_real_rows"):
            eng.learn_n(1)
        eng.attach_model_buffer(model, 8)
        eng.learn_n(1)
        eng.attach_model_buffer(None)
        eng.learn_n(1)                              # one source again
        assert (eng.debug_read(0, "b_rew") < MODEL_MARK).all()
    finally:
        eng.close(); real.close(); model.close()


# ---- 7. what is computed from the drawn batch ----------------------------------------------------------------------------------
def _ds(seed, n, od, ad):
    ds = synth.make_dataset(seed, n, od, ad, term_p=0.05)
    return ds["observations"], ds["actions"], ds["next_observations"], ds["rewards"], ds["terminals"].astype(np.float32)


@pytest.mark.parametrize("algo,case,precision", [("sac", "mopo_tiny", 0), ("sac", "mopo_halfcheetah", 1), ("cql", "combo_tiny", 0),
                                                 ("cql", "combo_halfcheetah", 1)])
def test_two_source_learn_n_matches_oracle_and_eager_step(algo, case, precision):
    """the bars of test_gpu_learn_n.py::test_learn_n_graph_replay_matches_oracle_and_eager_step: 1e-4 against the numpy oracle on the
    tapped batch and noise, 2e-6 between the graph and an eager orl_step on the same arrays"""
    from offlinerlkit import _engine
    R, steps = 3, 4
    if algo == "sac":
        from oracle import sac as mod
        cfg, st, _, _ = mopo_oracle_setup(case)
        c = synth.MOPO_CASES[case]
        make = lambda: tm._engine("sac", c, cfg, st, R, precision)
    else:
        from oracle import cql as mod
        cfg, st, _, _ = combo_oracle_setup(case)
        c = synth.COMBO_CASES[case]
        c0, Bc = cfg["cons_rows"]
        make = lambda: tm._engine("cql", c, cfg, st, R, precision, num_repeat_actions=c["N"], with_lagrange=int(cfg["with_lagrange"]),
                                  cql_alpha_lr=cfg["cql_alpha_lr"], cql_weight=cfg["cql_weight"], cql_cons_row0=c0, cql_cons_rows=Bc,
                                  cql_real_rows=cfg["real_rows"])
    eng, eager = make(), make()
    B, od, ad = c["B_real"] + c["B_fake"], c["obs_dim"], c["act_dim"]
    real, model = _engine.DeviceBuffer(od, ad), _engine.DeviceBuffer(od, ad)
    real.load(*_ds(11, 50_000, od, ad))
    model.reserve(60_000)
    model.append(*_ds(12, 30_000, od, ad))
    eng.attach_buffer(real)
    eng.attach_model_buffer(model, c["B_real"])
    states = [clone_state({k: v for k, v in st.items() if k not in ("opt", "cnt", "last_actor_loss")}) for _ in range(R)]
    for s in states:
        mod.init_opt(s)
    keys = eng.metric_names
    rd = lambda r, name, shape: eng.debug_read(r, name).reshape(shape)
    try:
        for k in range(steps):                      # k = 0: first launch of the freshly captured graph; k >= 1: replays
            m, _ = eng.learn_n(1)
            batches = [dict(observations=rd(r, "b_obs", (B, od)), actions=rd(r, "b_act", (B, ad)), next_observations=rd(r, "b_nobs", (B, od)),
                            rewards=rd(r, "b_rew", (B, 1)), terminals=rd(r, "b_term", (B, 1))) for r in range(R)]
            if algo == "sac":
                noises = [dict(eps_next=rd(r, "n_eps_next", (B, ad)), eps_actor=rd(r, "n_eps_actor", (B, ad))) for r in range(R)]
                nl = [np.stack([n[x] for n in noises]) for x in ("eps_next", "eps_actor")]
            else:
                BN = Bc * c["N"]
                noises = []
                for r in range(R):
                    xc = rd(r, "xc", (B + 3 * BN, -1))
                    noises.append(dict(eps_actor=rd(r, "n_eps_actor", (B, ad)), eps_next=rd(r, "n_eps_next", (-1, ad)),
                                       u_rand=xc[B + 2 * BN:, od:od + ad].copy(), eps_pi=rd(r, "n_eps_pi", (BN, ad)),
                                       eps_next_pi=rd(r, "n_eps_npi", (BN, ad))))
                nl = [np.stack([n[x] for n in noises]) for x in ("eps_actor", "eps_next", "u_rand", "eps_pi", "eps_next_pi")]
            for r in range(R):
                res, _ = mod.learn(states[r], cfg, batches[r], noises[r])
                ora = np.array([res[x] for x in keys])
                assert rel_err(m[r], ora, floor=1e-2) < 1e-4, (algo, case, "step", k, "run", r, m[r], ora)
            bb = {kk: np.stack([b[kk] for b in batches]) for kk in batches[0]}
            me = eager.step(bb, nl)
            assert rel_err(m, me, floor=1e-3) < 2e-6, (algo, case, k, np.abs(m - me).max())
            assert not np.array_equal(batches[0]["observations"], batches[R - 1]["observations"])
    finally:
        eng.close(); eager.close(); real.close(); model.close()


# ---- 8. device rollout == host rollout ---------------------------------------------------------------------------------------------
def test_rollout_device_matches_the_host_rollout_bit_for_bit(tmp_path):
    """Two EnsembleDynamics with the same parameters, scaler, elites, engine seed and call counter, one policy, the same torch seed:
    the device rollout must leave in the ring exactly the transitions the host rollout returns (same kernels on the same inputs; the
    stable compaction keeps every surviving row at the position whose Philox draws the host path consumes)."""
    import test_gpu_mb_trainer as tt
    from test_gpu_training import AD, OD, make_dataset
    from offlinerlkit.buffer import ReplayBuffer
    from offlinerlkit.dynamics import EnsembleDynamics
    from offlinerlkit.modules import EnsembleDynamicsModel
    from offlinerlkit.utils.logger import Logger
    from offlinerlkit.utils.scaler import StandardScaler
    from offlinerlkit.utils.termination_fns import TERM_ANT, termination_fn_ant
    torch.manual_seed(5)
    np.random.seed(5)
    ds = make_dataset(n_episodes=300)
    logger = Logger(str(tmp_path), {"consoleout_backup": "stdout", "dynamics_training_progress": "csv"})

    def dynamics():
        model = EnsembleDynamicsModel(OD, AD, [64, 64], num_ensemble=5, num_elites=3, weight_decays=[2.5e-5, 5e-5, 1e-4], device=DEV)
        d = EnsembleDynamics(model, torch.optim.Adam(model.parameters(), lr=1e-3), StandardScaler(), termination_fn_ant,
                             penalty_coef=0.5, uncertainty_mode="aleatoric")
        d.set_engine_options(seed=77)
        return d
    dyn_a = dynamics()
    data = ReplayBuffer(len(ds["rewards"]), (OD,), np.float32, AD, np.float32, device=DEV)
    data.load_dataset(ds)
    dyn_a.train(data.sample_all(), logger, max_epochs=10, max_epochs_since_update=5)           # saves into logger.model_dir
    dyn_b = dynamics()
    dyn_b.load(logger.model_dir)
    assert dyn_b.term_kind == TERM_ANT
    pol = tt._policy("mopo", dyn_a)
    n, L = 3000, 4
    rng = np.random.RandomState(1)
    init = np.stack([rng.uniform(0.25, 0.95, n), rng.uniform(-1.5, 1.5, n)], 1).astype(np.float32)      # x0 around TERM_ANT's 0.2 / 1.0 bounds
    torch.manual_seed(123)
    host, hinfo = pol.rollout(init, L)
    # not vacuous: some but not all rows terminate in each of the first two model steps
    term = host["terminals"].ravel()
    n1 = int((~term[:n]).sum())
    assert 0 < n1 < n and 0 < int((~term[n:n + n1]).sum()) < n1, (n, n1)
    pol.dynamics = dyn_b
    fake = ReplayBuffer(4 * n * L, (OD,), np.float32, AD, np.float32, device=DEV)
    real = ReplayBuffer(10, (OD,), np.float32, AD, np.float32, device=DEV)
    torch.manual_seed(123)
    dinfo = pol.rollout_device(real, fake, n, L, init_obss=init)
    assert dinfo["num_transitions"] == hinfo["num_transitions"] == fake._size == len(term)
    assert abs(dinfo["reward_mean"] - hinfo["reward_mean"]) <= 1e-6 * abs(hinfo["reward_mean"])
    got = fake.sample_all()
    for hk, dk in (("obss", "observations"), ("actions", "actions"), ("next_obss", "next_observations"), ("rewards", "rewards")):
        assert np.array_equal(np.asarray(host[hk], np.float32).view(np.uint32), got[dk].view(np.uint32)), hk
    assert np.array_equal(got["terminals"].ravel(), term.astype(np.float32))
    # a second rollout appends behind the first and samples its own initial states from the real buffer
    real.load_dataset(ds)
    info2 = pol.rollout_device(real, fake, 500, 2)
    assert fake._size == len(term) + info2["num_transitions"] and 500 <= info2["num_transitions"] <= 1000


def test_rollout_device_refuses_a_termination_function_without_a_kind():
    from offlinerlkit.utils import termination_fns as tf

    class Dyn:
        term_kind = tf.term_kind(tf.obs_unnormalization(tf.termination_fn_hopper, 0.0, 1.0))

        def step_device(self, o, a):
            raise AssertionError("not reached")
    from offlinerlkit.policy.model_based import _rollout_device

    class Pol:
        dynamics = Dyn()
    with pytest.raises(NotImplementedError, match="term_kind"):
        _rollout_device(Pol(), None, None, 4, 1, np.zeros((4, 2), np.float32), False)


# ---- 9. end to end -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo,n_runs,real_ratio", [("mopo", 1, 0.05), ("combo", 1, 0.5), ("mopo", 2, 0.05)])
def test_mb_trainer_fused_end_to_end(tmp_path, algo, n_runs, real_ratio):
    import test_gpu_mb_trainer as tt
    from test_gpu_training import AD, OD, PointMass, make_dataset
    from offlinerlkit.buffer import ReplayBuffer
    from offlinerlkit.policy_trainer import MBPolicyTrainer
    from offlinerlkit.utils.logger import Logger
    ROLLOUT = tt.ROLLOUT
    torch.manual_seed(3)
    np.random.seed(3)
    ds = make_dataset(n_episodes=300)
    logger = Logger(str(tmp_path), {"consoleout_backup": "stdout", "policy_training_progress": "csv", "dynamics_training_progress": "csv"})
    real = ReplayBuffer(len(ds["rewards"]), (OD,), np.float32, AD, np.float32, device=DEV)
    real.load_dataset(ds)
    dyn = tt._dynamics(real.sample_all(), logger)
    pol = tt._policy(algo, dyn)
    if n_runs > 1:
        pol.set_engine_options(n_runs=n_runs, seed=11)
    fake = ReplayBuffer(ROLLOUT[1] * ROLLOUT[2] * 2, (OD,), np.float32, AD, np.float32, device=DEV)
    lines = []
    log = logger.log
    logger.log = lambda s, *a, **k: (lines.append(s), log(s, *a, **k))

    class Env(PointMass):
        def get_normalized_score(self, x):
            return x / 20.0

    epochs, steps = 2, 250
    res = MBPolicyTrainer(pol, Env(1000), real, fake, logger, ROLLOUT, epoch=epochs, step_per_epoch=steps, batch_size=256,
                          real_ratio=real_ratio, eval_episodes=5, fused=True).train()
    rows = [ln.split(",") for ln in open(tmp_path / "record" / "policy_training_progress.csv").read().strip().split("\n")]
    head = rows[0]
    losses = ["loss/actor", "loss/critic1", "loss/critic2"] + (["loss/alpha", "alpha"] if algo == "mopo" else [])
    evals = ["eval/normalized_episode_reward", "eval/normalized_episode_reward_std", "eval/episode_length", "eval/episode_length_std"]
    want = set(losses + evals + ["rollout_info/num_transitions", "rollout_info/reward_mean", "timestep"])
    assert want <= set(head), want - set(head)
    assert "eval/episode_reward" not in head
    if n_runs > 1:
        assert {f"run{r}/{k}" for r in range(n_runs) for k in evals} <= set(head)
        assert {f"run{r}/{k}" for r in range(n_runs) for k in losses} <= set(head)
        for r in range(n_runs):
            assert (tmp_path / "model" / f"policy_run{r}.pth").exists()
    col = lambda k: np.array([float(x[head.index(k)]) for x in rows[1:]])
    for k in losses + evals:
        assert np.isfinite(col(k)).all(), k
    assert list(col("timestep")) == [steps * (e + 1) for e in range(epochs)]
    rl = [s for s in lines if s.startswith("num rollout transitions: ")]
    assert len(rl) == 5 and all(s.startswith("num rollout transitions: 3000,") for s in rl), rl
    assert np.allclose(col("rollout_info/num_transitions"), 3000.0)
    assert fake._size == fake._max_size == 6000 and fake.device_buffer().size() == 6000
    assert np.isfinite(fake.sample_all()["rewards"]).all() and np.abs(fake.sample_all()["observations"]).max() > 0
    for p in ("checkpoint/policy.pth", "model/policy.pth", "model/dynamics.pth"):
        assert (tmp_path / p).exists(), p
    assert np.isfinite(res["last_10_performance"]) and np.isfinite(col("eval/normalized_episode_reward")[-1])
    assert pol.engine.step_count() == epochs * steps
    print(f"fused {algo} x{n_runs}: normalised eval return per epoch {col('eval/normalized_episode_reward').round(2).tolist()}")
