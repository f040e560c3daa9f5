"""GPU: per-run model rings of a multi-run MOPO / COMBO policy -- the run-batched termination + compaction launch pair
(orl_buffer_append_rollout_runs) against R single-ring calls, the per-run source table of the minibatch draw
(orl_engine_attach_model_buffers) by provenance and against the single-ring attach, the per-run device rollout against a host loop,
and MBPolicyTrainer(fused=True) with a list of buffers end to end."""
import warnings

import numpy as np
import pytest
import torch

import test_gpu_mb_fused as tf1
from test_gpu_mb_fused import MODEL_MARK, _marked_rows, _uniform_ok

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RUN_MARK = float(2 ** 20)                 # ring r's rows carry rewards 2^23 + r * 2^20 + i: exact in fp32 for r <= 2, i < 2^20


# ---- 1. batched append == R single-ring appends ----------------------------------------------------------------------------------
def _straddling_next_obs(rng, shape, od):
    """next_obs whose columns 0 / 1 lie on both sides of TERM_ANT's [0.2, 1.0] and TERM_HOPPER's (x0 > 0.7, |x1| < 0.2) bounds"""
    x = (0.3 * rng.standard_normal(shape + (od,))).astype(np.float32)
    x[..., 0] = rng.uniform(0.0, 1.2, shape)
    x[..., 1] = rng.uniform(-0.3, 0.3, shape)
    return x


@pytest.mark.parametrize("od,ad", [(17, 6), (2, 2)])
@pytest.mark.parametrize("kind", ["TERM_ANT", "TERM_HOPPER", "TERM_NONE"])
def test_append_rollout_runs_equals_single_ring_appends_bit_for_bit(kind, od, ad):
    """Two ragged calls in a row into three rings of 700 rows (run 0 wraps on the second one) against three rings driven by the
    single-ring call: everything that comes back and everything in the rings is equal bit for bit.
    Non-vacuity: every run with at least two rows keeps some and loses some under TERM_ANT / TERM_HOPPER (a run of ONE row cannot
    have 0 < n_alive < n, and TERM_NONE never terminates: there n_alive == n is asserted instead)."""
    from offlinerlkit import _engine
    from offlinerlkit.utils import termination_fns as tf
    R, stride, cap = 3, 600, 700
    k = getattr(tf, kind)
    rng = np.random.RandomState(od * 10 + k)
    rings = [_engine.DeviceBuffer(od, ad) for _ in range(R)]
    refs = [_engine.DeviceBuffer(od, ad) for _ in range(R)]
    for b in rings + refs:
        b.reserve(cap)
    t = lambda x: torch.tensor(x, device=DEV)
    try:
        for n in ((600, 257, 0), (256, 1, 300)):
            obs = t(rng.standard_normal((R, stride, od)).astype(np.float32))
            act = t(rng.standard_normal((R, stride, ad)).astype(np.float32))
            nobs = t(_straddling_next_obs(rng, (R, stride), od))
            rew = t(rng.standard_normal((R, stride)).astype(np.float32))
            alive = torch.full((R, stride, od), -7.0, device=DEV)
            n_alive, rs = _engine.DeviceBuffer.append_rollout_runs(rings, k, obs, act, nobs, rew, n, alive)
            assert n_alive.shape == (R,) and rs.shape == (R,)
            got_alive = alive.cpu().numpy()
            for r in range(R):
                if n[r] == 0:
                    assert n_alive[r] == 0 and rs[r] == 0.0
                else:
                    ref_alive = torch.full((n[r], od), -7.0, device=DEV)
                    na, s = refs[r].append_rollout(k, obs[r, :n[r]], act[r, :n[r]], nobs[r, :n[r]], rew[r, :n[r]], ref_alive)
                    print(f"{kind} od={od} run {r}: n={n[r]} n_alive={n_alive[r]} (single {na}) rew_sum={rs[r]!r} (single {s!r})")
                    assert n_alive[r] == na and rs[r] == s                          # (float64 sums: equal, not close)
                    if kind == "TERM_NONE":
                        assert na == n[r]
                    elif n[r] >= 2:
                        assert 0 < na < n[r], (r, na, n[r])
                    assert np.array_equal(got_alive[r, :na].view(np.uint32), ref_alive[:na].cpu().numpy().view(np.uint32))
                # nothing behind a run's survivors is written: not the rest of its live rows, not its padding rows
                assert (got_alive[r, n_alive[r]:] == -7.0).all(), r
                assert rings[r].size() == refs[r].size()
                for a, b in zip(rings[r].read_rows(0, cap), refs[r].read_rows(0, cap)):
                    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), r
        assert [b.size() for b in rings] == [700, 258, 300]                         # the rings diverged
    finally:
        for b in rings + refs:
            b.close()


# ---- 2. refusals -------------------------------------------------------------------------------------------------------------------
def test_runs_entry_points_refuse():
    from offlinerlkit import _engine
    from offlinerlkit.utils import termination_fns as tf
    od, ad, R, B = 3, 2, 3, 16
    z = lambda *s: torch.zeros(s, device=DEV)
    rings = [_engine.DeviceBuffer(od, ad) for _ in range(R)]
    for b in rings:
        b.reserve(8)
    args = lambda st=4: (z(R, st, od), z(R, st, ad), z(R, st, od), z(R, st))
    eng = _engine.Engine(_engine.default_config("sac", obs_dim=od, act_dim=ad, hidden=[32, 32], batch_size=B, n_runs=R))
    real = _engine.DeviceBuffer(od, ad)
    try:
        with pytest.raises(ValueError, match="2 row counts for 3 rings"):
            _engine.DeviceBuffer.append_rollout_runs(rings, tf.TERM_NONE, *args(), (1, 1), z(R, 4, od))
        with pytest.raises(ValueError, match="expected"):                             # two rings, three row blocks
            _engine.DeviceBuffer.append_rollout_runs(rings[:2], tf.TERM_NONE, *args(), (1, 1), z(R, 4, od))
        bare = _engine.DeviceBuffer(od, ad)
        with pytest.raises(RuntimeError, match="run 1: not a ring"):
            _engine.DeviceBuffer.append_rollout_runs([rings[0], bare, rings[2]], tf.TERM_NONE, *args(), (1, 1, 1), z(R, 4, od))
        with pytest.raises(RuntimeError, match="run 2: more rows than the ring's capacity"):
            _engine.DeviceBuffer.append_rollout_runs(rings, tf.TERM_NONE, *args(12), (1, 0, 9), z(R, 12, od))
        with pytest.raises(RuntimeError, match="run 0: termination kind 6 reads observation column 26"):
            _engine.DeviceBuffer.append_rollout_runs(rings, tf.TERM_PEN, *args(), (1, 1, 1), z(R, 4, od))
        with pytest.raises(RuntimeError, match="run 2: the ring of run 0 again"):
            _engine.DeviceBuffer.append_rollout_runs([rings[0], rings[1], rings[0]], tf.TERM_NONE, *args(), (1, 1, 1), z(R, 4, od))
        assert [b.size() for b in rings] == [0, 0, 0]                                 # a refused call appends nothing
        real.load(*_marked_rows(np.arange(100), od, ad, False))
        eng.attach_buffer(real)
        with pytest.raises(RuntimeError, match="2 rings for an engine of 3 runs"):
            eng.attach_model_buffers(rings[:2], 4)
        with pytest.raises(RuntimeError, match="run 1: the model buffer must be a ring"):
            eng.attach_model_buffers([rings[0], bare, rings[2]], 4)
        for bad in (0, B, B + 1):
            with pytest.raises(RuntimeError, match="real_rows"):
                eng.attach_model_buffers(rings, bad)
        eng.attach_model_buffers(rings, 4)
        with pytest.raises(RuntimeError, match="model buffer of run 0 is empty"):
            eng.learn_n(1)
        rows = _marked_rows(np.arange(5), od, ad, True)
        rings[0].append(*rows)
        rings[2].append(*rows)
        with pytest.raises(RuntimeError, match="model buffer of run 1 is empty"):
            eng.learn_n(1)
        rings[1].append(*rows)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", _engine.EngineHealthWarning)
            eng.learn_n(1)
            eng.attach_model_buffers(None)                                            # detached: one source again
            eng.learn_n(1)
            assert (eng.debug_read(0, "b_rew") < MODEL_MARK).all()
            eng.attach_model_buffers(rings, 4)
            eng.attach_model_buffer(rings[1], 4)                                      # the single form replaces the per-run one
            eng.learn_n(1)
        for run in range(R):
            assert (eng.debug_read(run, "b_rew")[4:] >= MODEL_MARK).all()
        bare.close()
    finally:
        eng.close(); real.close()
        for b in rings:
            b.close()


# ---- 3. provenance per run -----------------------------------------------------------------------------------------------------------
def _ring_rows(i, r, od, ad):
    o, a, no, rew, t = _marked_rows(i, od, ad, True)
    return o, a, no, (rew.astype(np.float64) + r * RUN_MARK).astype(np.float32), t


@pytest.mark.parametrize("algo,precision", [("sac", 0), ("sac", 1), ("cql", 0), ("cql", 1)])
def test_per_run_draw_by_provenance(algo, precision):
    from offlinerlkit import _engine
    od, ad, B, R, real_rows = 17, 6, 256, 3, 12
    n_real, sizes, more, cap = 5_000, (3000, 500, 1), (9000, 1500, 0), 20_000
    over = dict(obs_dim=od, act_dim=ad, batch_size=B, n_runs=R, precision=precision, seed=99)
    N = 0
    if algo == "cql":
        N = 4
        over.update(num_repeat_actions=N, with_lagrange=0, cql_real_rows=real_rows, cql_cons_row0=0, cql_cons_rows=B)
    eng = _engine.Engine(_engine.default_config(algo, **over))
    real = _engine.DeviceBuffer(od, ad)
    real.load(*_marked_rows(np.arange(n_real), od, ad, False))
    rings = [_engine.DeviceBuffer(od, ad) for _ in range(R)]
    for r, b in enumerate(rings):
        b.reserve(cap)
        b.append(*_ring_rows(np.arange(sizes[r]), r, od, ad))
    eng.attach_buffer(real)
    eng.attach_model_buffers(rings, real_rows)

    def step():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", _engine.EngineHealthWarning)      # (rewards of 2^23 with untrained networks: the losses are huge)
            eng.learn_n(1)
        out = []
        for run in range(R):
            rew = eng.debug_read(run, "b_rew").reshape(B).astype(np.float64)
            is_model = rew >= MODEL_MARK
            assert not is_model[:real_rows].any() and is_model[real_rows:].all(), (run, rew[:real_rows + 2])
            ring = np.where(is_model, np.floor((rew - MODEL_MARK) / RUN_MARK), -1).astype(np.int64)
            assert (ring[real_rows:] == run).all(), (run, np.unique(ring[real_rows:]))       # run r's model rows: ring r only
            idx = np.where(is_model, rew - MODEL_MARK - run * RUN_MARK, rew).astype(np.int64)
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
        first = np.stack([step() for _ in range(20)])                   # (steps, runs, B)
        for r in range(R):
            assert first[:, r, real_rows:].max() < sizes[r], r          # below THAT ring's size
        assert (first[:, 2, real_rows:] == 0).all()                     # a ring of one row: always row 0
        assert first[:, 0, real_rows:].max() >= sizes[1]                # (ring 0's range is really its own)
        # rings 0 and 1 grow; the captured graph is replayed without re-attaching and reads each new size from that ring's cell
        for r in range(R):
            if more[r]:
                rings[r].append(*_ring_rows(np.arange(sizes[r], sizes[r] + more[r]), r, od, ad))
        second = np.stack([step() for _ in range(200)])
        for r in (0, 1):
            m_idx = second[:, r, real_rows:].ravel()
            assert m_idx.max() < sizes[r] + more[r] and (m_idx >= sizes[r]).mean() > 0.6, r      # rows of the new range appear (3/4 of the ring)
            _uniform_ok(m_idx, sizes[r] + more[r], f"model ring {r}")
        assert (second[:, 2, real_rows:] == 0).all()
        _uniform_ok(second[:, :, :real_rows].ravel(), n_real, "real source")
        assert eng.step_count() == 220
    finally:
        eng.close(); real.close()
        for b in rings:
            b.close()


# ---- 4. same rings, same arithmetic ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["sac", "cql"])
def test_per_run_rings_with_one_rings_rows_match_the_single_ring_attach(algo):
    from offlinerlkit import _engine
    od, ad, B, R, real_rows = 11, 3, 64, 3, 16
    over = dict(obs_dim=od, act_dim=ad, hidden=[64, 64], batch_size=B, n_runs=R, precision=0, seed=5)
    if algo == "cql":
        over.update(num_repeat_actions=3, with_lagrange=0, cql_real_rows=real_rows, cql_cons_row0=0, cql_cons_rows=B)
    one, per_run = _engine.Engine(_engine.default_config(algo, **over)), _engine.Engine(_engine.default_config(algo, **over))
    real, single = _engine.DeviceBuffer(od, ad), _engine.DeviceBuffer(od, ad)
    real.load(*tf1._ds(11, 4_000, od, ad))
    rows = tf1._ds(12, 1_500, od, ad)
    rings = [_engine.DeviceBuffer(od, ad) for _ in range(R)]
    for b in [single] + rings:
        b.reserve(2_000)
        b.append(*rows)
    one.attach_buffer(real)
    one.attach_model_buffer(single, real_rows)
    per_run.attach_buffer(real)
    per_run.attach_model_buffers(rings, real_rows)
    try:
        for k in range(4):                          # k = 0: the freshly captured graphs; k >= 1: replays
            ma, _ = one.learn_n(1)
            mb, _ = per_run.learn_n(1)
            assert np.isfinite(ma).all()
            assert np.array_equal(ma.view(np.uint32), mb.view(np.uint32)), (algo, k, np.abs(ma - mb).max())
            assert np.array_equal(one.debug_read(R - 1, "b_obs"), per_run.debug_read(R - 1, "b_obs"))
        assert not np.array_equal(ma[0], ma[R - 1])                     # (the runs are different trainings)
    finally:
        one.close(); per_run.close(); real.close(); single.close()
        for b in rings:
            b.close()


# ---- 5. device rollout == a host loop ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dyn_runs", [3, 1])
def test_rollout_device_runs_matches_a_host_loop_bit_for_bit(tmp_path, dyn_runs):
    """Twin dynamics (same parameters, scalers, elites, engine seed and call counter) and one 3-run policy under the same torch seed.
    The host loop steps ``EnsembleDynamics.step`` on [R, nmax] arrays padded with zero rows (or, for the shared one-run ensemble, on
    the R * nmax folded rows), applies the numpy termination function and compacts each run; ring r must hold run r's transitions."""
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
    R, N, L = 3, 3000, 4

    def dynamics():
        model = EnsembleDynamicsModel(OD, AD, [64, 64], num_ensemble=5, num_elites=3, weight_decays=[2.5e-5, 5e-5, 1e-4], device=DEV)
        d = EnsembleDynamics(model, torch.optim.Adam(model.parameters(), lr=1e-3), StandardScaler(), termination_fn_ant,
                             penalty_coef=0.5, uncertainty_mode="aleatoric")
        d.set_engine_options(n_runs=dyn_runs, seed=77)
        return d
    dyn_a = dynamics()
    data = ReplayBuffer(len(ds["rewards"]), (OD,), np.float32, AD, np.float32, device=DEV)
    data.load_dataset(ds)
    dyn_a.train(data.sample_all(), logger, max_epochs=10, max_epochs_since_update=5)
    dyn_b = dynamics()
    dyn_b._bind()
    for r in range(dyn_runs):                       # save / load act on the selected run
        where = tmp_path / f"dyn_run{r}"
        where.mkdir()
        dyn_a.select_run(r)
        dyn_a.save(str(where))
        dyn_b.select_run(r)
        dyn_b.load(str(where))
    dyn_a.select_run(0)
    dyn_b.select_run(0)
    assert dyn_b.term_kind == TERM_ANT
    pol = tt._policy("mopo", dyn_a)
    pol.set_engine_options(n_runs=R, seed=11)
    pol._bind(256)
    rng = np.random.RandomState(1)
    init = np.stack([rng.uniform(0.25, 0.95, R * N), rng.uniform(-1.5, 1.5, R * N)], 1).astype(np.float32).reshape(R, N, OD)

    # the host loop
    torch.manual_seed(123)
    host = [dict(o=[], a=[], no=[], r=[], t=[]) for _ in range(R)]
    obs, live, counts = [init[r] for r in range(R)], np.full(R, N), []
    for _ in range(L):
        nmax = int(live.max())
        pad = np.zeros((R, nmax, OD), np.float32)
        for r in range(R):
            pad[r, :live[r]] = obs[r]
        act = pol.actforward_runs(torch.tensor(pad, device=DEV), False).cpu().numpy()
        if dyn_runs == R:
            dyn_a.terminal_fn = lambda o, a, n: np.zeros(n.shape[:2] + (1,), bool)       # (3-d arrays: the test below is applied per run)
            nxt, rew, _, _ = dyn_a.step(pad, act)
            dyn_a.terminal_fn = termination_fn_ant
        else:
            nxt, rew, _, _ = dyn_a.step(pad.reshape(R * nmax, OD), act.reshape(R * nmax, AD))
            nxt, rew = nxt.reshape(R, nmax, OD), rew.reshape(R, nmax, 1)
        nxt_live = []
        for r in range(R):
            n = int(live[r])
            o, a, no, rw = pad[r, :n], act[r, :n], nxt[r, :n], rew[r, :n]
            term = termination_fn_ant(o, a, no).ravel() if n else np.zeros(0, bool)
            for key, v in zip(("o", "a", "no", "r", "t"), (o, a, no, rw.reshape(n), term.astype(np.float32))):
                host[r][key].append(v)
            nxt_live.append(no[~term])
        obs, live = nxt_live, np.array([len(x) for x in nxt_live])
        counts.append(live.copy())
        if live.max() == 0:
            break
    print("survivors per step and run:", [c.tolist() for c in counts])
    # not vacuous: in each of the first two steps at least two runs lose some rows but not all, and the runs differ
    prev = np.full(R, N)
    for c in counts[:2]:
        assert ((0 < c) & (c < prev)).sum() >= 2, (prev, c)
        prev = c
    assert len(set(counts[0].tolist())) > 1, counts[0]

    pol.dynamics = dyn_b
    fakes = [ReplayBuffer(N * L, (OD,), np.float32, AD, np.float32, device=DEV) for _ in range(R)]
    real = ReplayBuffer(10, (OD,), np.float32, AD, np.float32, device=DEV)
    torch.manual_seed(123)
    info = pol.rollout_device(real, fakes, N, L, init_obss=init)
    assert info["num_transitions"].shape == (R,) and info["reward_mean"].shape == (R,)
    for r in range(R):
        want = {k: np.concatenate(v) for k, v in host[r].items()}
        assert info["num_transitions"][r] == len(want["r"]) == fakes[r]._size
        mean = want["r"].astype(np.float64).mean()
        assert abs(info["reward_mean"][r] - mean) <= 1e-6 * abs(mean)
        got = fakes[r].sample_all()
        for hk, dk in (("o", "observations"), ("a", "actions"), ("no", "next_observations")):
            assert np.array_equal(want[hk].astype(np.float32).view(np.uint32), got[dk].view(np.uint32)), (r, hk)
        assert np.array_equal(want["r"].astype(np.float32).view(np.uint32), got["rewards"].ravel().view(np.uint32)), r
        assert np.array_equal(want["t"], got["terminals"].ravel()), r
    # a second rollout appends behind the first and samples its own R * n initial states from the real buffer
    real.load_dataset(ds)
    before = [f._size for f in fakes]
    info2 = pol.rollout_device(real, fakes, 200, 2)
    for r in range(R):
        assert fakes[r]._size == before[r] + info2["num_transitions"][r] and 200 <= info2["num_transitions"][r] <= 400


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo,n_runs,real_ratio", [("mopo", 2, 0.05), ("combo", 2, 0.5)])
def test_mb_trainer_fused_per_run_rings_end_to_end(tmp_path, algo, n_runs, real_ratio):
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
    dyn = tt._dynamics(real.sample_all(), logger)               # one shared ensemble
    pol = tt._policy(algo, dyn)
    pol.set_engine_options(n_runs=n_runs, seed=11)
    fakes = [ReplayBuffer(ROLLOUT[1] * ROLLOUT[2] * 2, (OD,), np.float32, AD, np.float32, device=DEV) for _ in range(n_runs)]
    lines = []
    log = logger.log
    logger.log = lambda s, *a, **k: (lines.append(s), log(s, *a, **k))

    class Env(PointMass):
        def get_normalized_score(self, x):
            return x / 20.0

    epochs, steps = 2, 250
    res = MBPolicyTrainer(pol, Env(1000), real, fakes, logger, ROLLOUT, epoch=epochs, step_per_epoch=steps, batch_size=256,
                          real_ratio=real_ratio, eval_episodes=5, fused=True).train()
    rows = [ln.split(",") for ln in open(tmp_path / "record" / "policy_training_progress.csv").read().strip().split("\n")]
    head = rows[0]
    losses = ["loss/actor", "loss/critic1", "loss/critic2"] + (["loss/alpha", "alpha"] if algo == "mopo" else [])
    evals = ["eval/normalized_episode_reward", "eval/normalized_episode_reward_std", "eval/episode_length", "eval/episode_length_std"]
    roll = ["rollout_info/num_transitions", "rollout_info/reward_mean"]
    want = set(losses + evals + roll + ["timestep"]) | {f"run{r}/{k}" for r in range(n_runs) for k in losses + evals + roll}
    assert want <= set(head), want - set(head)
    col = lambda k: np.array([float(x[head.index(k)]) for x in rows[1:]])
    for k in losses + evals + roll + [f"run{r}/{k}" for r in range(n_runs) for k in losses + roll]:
        assert np.isfinite(col(k)).all(), k
    assert list(col("timestep")) == [steps * (e + 1) for e in range(epochs)]
    rl = [s for s in lines if s.startswith("num rollout transitions: ")]
    assert len(rl) == 5 and all(s.startswith(f"num rollout transitions: {3000 * n_runs},") for s in rl), rl
    assert np.allclose(col("rollout_info/num_transitions"), 3000.0)
    assert np.allclose(col("rollout_info/reward_mean"), np.mean([col(f"run{r}/rollout_info/reward_mean") for r in range(n_runs)], axis=0))
    for r in range(n_runs):
        assert np.allclose(col(f"run{r}/rollout_info/num_transitions"), 3000.0)
        assert fakes[r]._size == fakes[r]._max_size == 6000 and fakes[r].device_buffer().size() == 6000      # full to capacity
        got = fakes[r].sample_all()
        assert np.isfinite(got["rewards"]).all() and np.abs(got["observations"]).max() > 0
        assert (tmp_path / "model" / f"policy_run{r}.pth").exists() and (tmp_path / "checkpoint" / f"policy_run{r}.pth").exists()
    a, b = fakes[0].sample_all(), fakes[1].sample_all()
    assert not np.array_equal(a["observations"], b["observations"]) and not np.array_equal(a["actions"], b["actions"])      # two trainings
    assert not np.array_equal(col("run0/loss/critic1"), col("run1/loss/critic1"))
    for p in ("checkpoint/policy.pth", "model/policy.pth", "model/dynamics.pth"):
        assert (tmp_path / p).exists(), p
    assert np.isfinite(res["last_10_performance"])
    assert pol.engine.step_count() == epochs * steps
