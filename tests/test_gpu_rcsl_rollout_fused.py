"""GPU: the MBRCSL rollout as one device loop -- the trajectory store's device-counted step (orl_traj_append_step_counted) against the
numpy bookkeeping of rcsl_rollout_ref.py bit for bit, under stale and exact row bounds; the refusals of the step and of the loop; the
loop (orl_mbrcsl_rollout) against a replay of every step through the public calls on its own stored rows; a rollout in which
everything dies at once; the same replay around a regrowth of the loop's workspaces; reproducibility, and the host-counted path around a
fused rollout."""
import os

import numpy as np
import pytest
import torch

import rcsl_fused_ref as fref
import rcsl_rollout_ref as ref
from helpers import GOLDEN_DIR
from test_gpu_rcsl_rollout import DEV, TERM_FIXTURE, _filtered, _rcsl_policy, _ring_rows, _same_rows, t

pytestmark = pytest.mark.gpu
# what the rows in [live, bound) of a counted step's inputs hold: a NaN the fixture (whose own NaNs are 0x7FC00000) does not contain, so
# "no such bit pattern in the store" says that no row beyond the live count was read into it
POISON = np.uint32(0x7FC0BEEF)


def _poisoned(a, live, bound):
    out = np.full((bound,) + a.shape[1:], POISON, dtype=np.uint32).view(np.float32)
    out[:live] = a[:live]
    return out


def _equals_the_book(store, book, rew_abs):
    """the finished store against the finished book: every column, the counts, returns and rtg bit for bit; no poisoned row stored"""
    want, winfo = book.finish()
    rows, rew_sum, returns = store.finish()
    assert rows == winfo["num_transitions"], (rows, winfo["num_transitions"])
    got = store.read(0, rows)
    for gk, wk in (("obs", "obss"), ("next_obs", "next_obss"), ("act", "actions"), ("acc_ret", "acc_rets")):
        assert got[gk].dtype == want[wk].dtype and np.array_equal(ref.bits(got[gk]), ref.bits(want[wk])), gk
    assert np.array_equal(ref.bits(got["rew"]), ref.bits(want["rewards"].ravel()))
    assert np.array_equal(got["term"], want["terminals"].ravel().astype(np.float32))
    assert np.array_equal(got["traj_idx"], want["traj_idxs"])
    assert got["rtg"].dtype == np.float64 and np.array_equal(ref.bits(got["rtg"]), ref.bits(want["rtgs"].ravel()))
    assert returns.dtype == np.float64 and np.array_equal(ref.bits(returns), ref.bits(winfo["returns"]))
    assert abs(rew_sum - book.rewards_arr.sum()) <= 1e-9 * max(rew_abs, 1e-300), (rew_sum, book.rewards_arr.sum(), rew_abs)
    for k in ("obs", "next_obs", "act", "rew"):
        assert not (ref.bits(got[k]) == POISON).any(), k
    for k, wk in (("obs", "obss"), ("next_obs", "next_obss"), ("act", "actions")):
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[wk])), k                # no NaN but the fixture's own
    assert np.isfinite(got["rew"]).all() and np.isfinite(got["rtg"]).all() and np.isfinite(returns).all()
    return rows


def _counted_against_the_book(kind, obs, act, nobs, done, steps, rew_of, stale, refresh=False):
    """``_steps_against_the_book`` of test_gpu_rcsl_rollout.py with counted steps: step k is fed ``bound`` rows -- the initial row count
    (``stale``) or the exact live count -- of which the first n_live are the fixture's and the rest poisoned, and ``alive`` prefilled with
    -7.  The live count the test tracks comes from the book, never from the device, unless ``refresh`` asks for ``live_count()``."""
    from offlinerlkit import _engine
    n, od, ad = obs.shape[0], obs.shape[1], act.shape[1]
    store = _engine.TrajStore(od, ad, n, steps * n)
    book = ref.HostBook(n)
    live, rew_abs = n, 0.0
    for k in range(steps):
        bound = n if stale else live
        rew = rew_of(k, live)
        mask = book.step(obs[:live], act[:live], nobs[:live], rew[:, None], done[:live, None])
        n_alive = int(mask.sum())
        alive = torch.full((bound, od), -7.0, device=DEV)
        store.append_step_counted(kind, t(_poisoned(obs, live, bound)), t(_poisoned(act, live, bound)), t(_poisoned(nobs, live, bound)),
                                  t(_poisoned(rew, live, bound)), bound, alive)
        assert np.array_equal(ref.bits(alive[:n_alive].cpu().numpy()), ref.bits(nobs[:live][mask])), k
        assert (alive[n_alive:] == -7.0).all()                       # nothing behind the survivors is written
        if refresh:
            assert store.live_count() == n_alive, k
        rew_abs += float(np.abs(rew).astype(np.float64).sum())
        live = n_alive
        if live == 0:
            break
    rows = _equals_the_book(store, book, rew_abs)
    assert store.live_count() == live
    store.close()
    return rows


# ---- 1. the counted store against numpy ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stale", [True, False], ids=["bound=initial", "bound=live"])
@pytest.mark.parametrize("rows", [368, 1, 255, 600])
@pytest.mark.parametrize("kind", sorted(TERM_FIXTURE))
def test_counted_store_matches_the_numpy_bookkeeping(kind, rows, stale):
    from offlinerlkit.utils import termination_fns as tf
    g = np.load(os.path.join(GOLDEN_DIR, "mb_termination.npz"))
    pick = np.arange(rows) % 368
    obs, act, nobs = g["obs"][pick], g["act"][pick], g["next_obs"][pick]
    assert not (ref.bits(nobs) == POISON).any()
    done = np.asarray(g[TERM_FIXTURE[kind]]).astype(bool).ravel()[pick]
    rew_of = lambda k, n: (np.linspace(-3.0, 5.0, n) + 0.37 * k).astype(np.float32)
    # (the exact-bound runs also refresh the host's counts after every step: counted steps go on after a refresh)
    _counted_against_the_book(getattr(tf, kind), obs, act, nobs, done, 3, rew_of, stale, refresh=not stale)


def test_counted_step_with_nothing_live_writes_nothing():
    """256 rows that all end in the first step (humanoid: x0 = 0 < 1), then a step of bound 256 on live 0 whose inputs are all poison"""
    from offlinerlkit import _engine
    from offlinerlkit.utils import termination_fns as tf
    n, od, ad = 256, 3, 2
    rng = np.random.RandomState(0)
    obs, act = rng.standard_normal((n, od)).astype(np.float32), rng.standard_normal((n, ad)).astype(np.float32)
    nobs = rng.standard_normal((n, od)).astype(np.float32)
    nobs[:, 0] = 0.0
    rew = rng.standard_normal(n).astype(np.float32)
    store = _engine.TrajStore(od, ad, n, 3 * n)
    book = ref.HostBook(n)
    book.step(obs, act, nobs, rew[:, None], np.ones((n, 1), bool))
    alive = torch.full((n, od), -7.0, device=DEV)
    store.append_step_counted(tf.TERM_HUMANOID, t(obs), t(act), t(nobs), t(rew), n, alive)
    for _ in range(2):
        store.append_step_counted(tf.TERM_HUMANOID, t(_poisoned(obs, 0, n)), t(_poisoned(act, 0, n)), t(_poisoned(nobs, 0, n)),
                                  t(_poisoned(rew, 0, n)), n, alive)
    assert (alive == -7.0).all()
    assert _equals_the_book(store, book, float(np.abs(rew).astype(np.float64).sum())) == n and store.live_count() == 0
    store.close()


def test_counted_store_beyond_256_blocks_under_a_stale_bound():
    """70 000 rows = 274 blocks, both steps launched for 70 000: in the second the blocks beyond the live count report zeros, and the
    sum of the counts of the blocks in front takes its second trip (b += 256)"""
    from offlinerlkit.utils import termination_fns as tf
    n = 70_000
    rng = np.random.RandomState(3)
    nobs = np.stack([rng.uniform(0.0, 1.2, n), rng.standard_normal(n)], 1).astype(np.float32)
    obs = rng.standard_normal((n, 2)).astype(np.float32)
    act = rng.standard_normal((n, 3)).astype(np.float32)
    done = np.asarray(tf.termination_fn_ant(obs, act, nobs)).astype(bool).ravel()
    assert 0.25 * n < done.sum() < 0.42 * n
    rew_of = lambda k, m: (np.linspace(-1.0, 2.0, m) + 0.5 * k).astype(np.float32)
    assert _counted_against_the_book(tf.TERM_ANT, obs, act, nobs, done, 2, rew_of, True) > n + 65_536 // 2


# ---- the rollout's collaborators --------------------------------------------------------------------------------------------------------------
N_TRAJ, LENGTH = 600, 6


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """test_gpu_rcsl_rollout.py's sizes: an EnsembleDynamics [64, 64] of 5 members / 3 elites trained for three epochs and saved, any
    number of twins loaded from it (same parameters, scaler, elites, engine seed, call counter 0), one untrained AutoregressivePolicy
    [32, 32], TERM_ANT, 600 initial states around its bounds"""
    from test_gpu_training import AD, OD, make_dataset
    from offlinerlkit.buffer import ReplayBuffer
    from offlinerlkit.dynamics import EnsembleDynamics
    from offlinerlkit.modules import EnsembleDynamicsModel
    from offlinerlkit.policy import AutoregressivePolicy
    from offlinerlkit.utils.logger import Logger
    from offlinerlkit.utils.scaler import StandardScaler
    from offlinerlkit.utils.termination_fns import TERM_ANT, termination_fn_ant
    tmp = tmp_path_factory.mktemp("rcsl_rollout_fused")
    torch.manual_seed(5)
    np.random.seed(5)
    ds = make_dataset(n_episodes=300)
    logger = Logger(str(tmp), {"consoleout_backup": "stdout", "dynamics_training_progress": "csv"})

    def dynamics(n_runs=1, with_reward=True):
        model = EnsembleDynamicsModel(OD, AD, [64, 64], num_ensemble=5, num_elites=3, weight_decays=[2.5e-5, 5e-5, 1e-4],
                                      with_reward=with_reward, device=DEV)
        d = EnsembleDynamics(model, torch.optim.Adam(model.parameters(), lr=1e-3), StandardScaler(), termination_fn_ant,
                             penalty_coef=0.5, uncertainty_mode="aleatoric")
        d.set_engine_options(n_runs=n_runs, seed=77)
        return d
    first = dynamics()
    data = ReplayBuffer(len(ds["rewards"]), (OD,), np.float32, AD, np.float32, device=DEV)
    data.load_dataset(ds)
    first.train(data.sample_all(), logger, max_epochs=3, max_epochs_since_update=3)           # saves into logger.model_dir

    def twin():
        d = dynamics()
        d.load(logger.model_dir)
        assert d.term_kind == TERM_ANT
        return d
    ar = AutoregressivePolicy(OD, AD, [32, 32], 1e-3, DEV)
    rng = np.random.RandomState(1)
    init = np.stack([rng.uniform(0.25, 0.95, N_TRAJ), rng.uniform(-1.5, 1.5, N_TRAJ)], 1).astype(np.float32)   # x0 around TERM_ANT's 0.2 / 1.0 bounds
    return dict(twin=twin, dynamics=dynamics, ar=ar, init=init, od=OD, ad=AD, kind=TERM_ANT, term_fn=termination_fn_ant, scaler=first.scaler)


def _loop(world, dyn, store, init, length, lag, eps, kind=None, mode=None, coef=None, pol=None):
    """orl_mbrcsl_rollout through the engines of ``dyn`` and of ``pol`` (the world's policy when none is given) -> (rows, reward sum,
    returns, steps enqueued, ms)"""
    deng, m, c = dyn.loop_engine()
    io = t(np.ascontiguousarray(init, dtype=np.float32))
    torch.cuda.synchronize()
    return (pol or world["ar"]).loop_engine().mbrcsl_rollout(deng, store, io.data_ptr(), len(init), length, world["kind"] if kind is None else kind,
                                                    m if mode is None else mode, c if coef is None else coef,
                                                    None if eps is None else eps.data_ptr(), lag)


def _step_sizes(term, n_traj):
    """the row count of every step of a finished store, from its terminal column"""
    sizes, off, n = [], 0, n_traj
    while off < len(term) and n > 0:
        sizes.append(n)
        nxt = int((term[off:off + n] == 0).sum())
        off, n = off + n, nxt
    assert off == len(term), (off, len(term), sizes)
    return sizes


def _book_of(world, got, n_traj):
    """HostBook run on a store's own rows, the terminals from the host's termination function -> (book, step sizes)"""
    sizes = _step_sizes(got["term"], n_traj)
    book, off = ref.HostBook(n_traj), 0
    for n in sizes:
        s = slice(off, off + n)
        term = np.asarray(world["term_fn"](got["obs"][s], got["act"][s], got["next_obs"][s])).astype(bool).reshape(n, 1)
        book.step(got["obs"][s], got["act"][s], got["next_obs"][s], got["rew"][s, None], term)
        off += n
    return book, sizes


def _store_equals_its_book(world, store, rows, returns, n_traj):
    got = store.read(0, rows)
    book, sizes = _book_of(world, got, n_traj)
    want, winfo = book.finish()
    assert rows == winfo["num_transitions"] == sum(sizes)
    assert np.array_equal(got["term"], want["terminals"].ravel().astype(np.float32))
    assert np.array_equal(got["traj_idx"], want["traj_idxs"])
    assert np.array_equal(ref.bits(got["acc_ret"]), ref.bits(want["acc_rets"]))
    assert np.array_equal(ref.bits(got["rtg"]), ref.bits(want["rtgs"].ravel()))
    assert returns.dtype == np.float64 and np.array_equal(ref.bits(returns), ref.bits(winfo["returns"]))
    off = 0
    for k, n in enumerate(sizes[:-1]):      # the observation rows of step k + 1 are the surviving next_obs rows of step k, in their order
        alive = got["term"][off:off + n] == 0
        assert np.array_equal(ref.bits(got["obs"][off + n:off + n + sizes[k + 1]]), ref.bits(got["next_obs"][off:off + n][alive])), k
        off += n
    return got, sizes


# ---- 2. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_counted_step_refusals():
    from offlinerlkit import _engine
    from offlinerlkit.utils import termination_fns as tf
    od, ad, n = 11, 3, 6
    store = _engine.TrajStore(od, ad, n, 2 * n + 1)
    z = lambda rows, c: torch.zeros((rows, c), device=DEV)
    counted = lambda kind, bound: store.append_step_counted(kind, z(n, od), z(n, ad), z(n, od), torch.zeros(n, device=DEV), bound, z(n, od))
    hosted = lambda rows: store.append_step(tf.TERM_NONE, z(rows, od), z(rows, ad), z(rows, od), torch.zeros(rows, device=DEV), z(rows, od))
    with pytest.raises(RuntimeError, match="reads observation column 26"):
        counted(tf.TERM_PEN, n)
    with pytest.raises(RuntimeError, match="unknown termination kind"):
        counted(7, n)
    nobs = z(n, od)
    with pytest.raises(RuntimeError, match="must not overlap"):
        store.append_step_counted(tf.TERM_NONE, z(n, od), z(n, ad), nobs, torch.zeros(n, device=DEV), n, nobs)
    counted(tf.TERM_NONE, n)
    with pytest.raises(RuntimeError, match="refresh"):                      # the host's counts are stale
        hosted(n)
    with pytest.raises(RuntimeError, match="orl_traj_live or orl_traj_finish"):
        store.read(0, n)
    counted(tf.TERM_NONE, n)
    with pytest.raises(RuntimeError, match="capacity"):                     # 2 n + 1 rows of room, the bounds sum to 3 n
        counted(tf.TERM_NONE, n)
    assert store.live_count() == n                                          # a refresh: the host-counted step is allowed again ...
    with pytest.raises(RuntimeError, match="capacity"):
        hosted(n)                                                           # ... and refused for its own reason
    rows, _, returns = store.finish()
    assert rows == 2 * n and not returns.any()                              # the refused calls wrote nothing
    assert np.array_equal(store.read(0, rows)["traj_idx"], np.tile(np.arange(n), 2))
    store.reset(n)
    assert hosted(n) == n                                                   # host-counted, then counted, then host-counted after a refresh
    store.append_step_counted(tf.TERM_NONE, z(n, od), z(n, ad), z(n, od), torch.zeros(n, device=DEV), 1, z(n, od))    # a bound below the live count
    with pytest.raises(RuntimeError, match="more live trajectories than its bound"):
        store.finish()
    store.reset(n - 2)                                                      # reset clears the overflow
    assert hosted(n - 2) == n - 2 and store.finish()[0] == n - 2
    store.close()


def test_loop_refusals_leave_everything_as_it_was(world):
    from offlinerlkit import _engine
    from offlinerlkit.policy import AutoregressivePolicy
    from offlinerlkit.utils import termination_fns as tf
    od, ad, init = world["od"], world["ad"], world["init"][:8]
    dyn = world["twin"]()
    deng = dyn.loop_engine()[0]
    peng = world["ar"].loop_engine()
    store = _engine.TrajStore(od, ad, 8, 8 * 3)
    z = lambda rows, c: torch.zeros((rows, c), device=DEV)
    store.append_step_counted(tf.TERM_NONE, t(init), z(8, ad), t(init + 1), torch.ones(8, device=DEV), 8, z(8, od))
    before = store.finish()
    rows_before = store.read(0, before[0])
    params = {k: v.copy() for k, v in deng.get_params(0).items()}
    pol_params = {k: v.detach().clone() for k, v in world["ar"].state_dict().items()}
    eps = torch.randn((3, 8, ad), device=DEV)
    io = t(init)

    def call(p=peng, d=deng, s=store, n=8, length=3, kind=tf.TERM_ANT, mode=0, lag=2):
        return p.mbrcsl_rollout(d, s, io.data_ptr(), n, length, kind, mode, 0.5, eps.data_ptr(), lag)
    two_pol = AutoregressivePolicy(od, ad, [32, 32], 1e-3, DEV)
    two_pol.set_engine_options(n_runs=2)
    two_dyn = world["dynamics"](n_runs=2)
    no_rew = world["dynamics"](with_reward=False)
    for sc in two_dyn.scalers + no_rew.scalers:
        sc.mu, sc.std = world["scaler"].mu, world["scaler"].std
    not_autoreg = _rcsl_policy(None, None, od, ad)
    not_autoreg._bind(64)
    wide_store = _engine.TrajStore(od + 1, ad, 8, 24)
    few_traj = _engine.TrajStore(od, ad, 7, 24)
    few_rows = _engine.TrajStore(od, ad, 8, 23)
    with pytest.raises(RuntimeError, match="n_runs == 1 on both"):
        call(p=two_pol.loop_engine())
    with pytest.raises(RuntimeError, match="n_runs == 1 on both"):
        call(d=two_dyn.loop_engine()[0])
    with pytest.raises(RuntimeError, match="not an AUTOREG engine"):
        call(p=not_autoreg.engine)
    with pytest.raises(RuntimeError, match="dims of engine, dynamics and trajectory store differ"):
        call(s=wide_store)
    with pytest.raises(RuntimeError, match="created for 7"):
        call(s=few_traj)
    with pytest.raises(RuntimeError, match="need 24 rows, the store's capacity is 23"):
        call(s=few_rows)
    with pytest.raises(RuntimeError, match="need 32 rows"):
        call(length=4)
    with pytest.raises(RuntimeError, match="unknown termination kind"):
        call(kind=7)
    with pytest.raises(RuntimeError, match="reads observation column 26"):
        call(kind=tf.TERM_PEN)
    with pytest.raises(RuntimeError, match="unknown penalty mode"):
        call(mode=3)
    with pytest.raises(RuntimeError, match="lag must be >= 0"):
        call(lag=-1)
    with pytest.raises(RuntimeError, match="needs a dynamics with_reward"):
        call(d=no_rew.loop_engine()[0])
    after = store.finish()
    assert after[0] == before[0] and after[1] == before[1] and np.array_equal(ref.bits(after[2]), ref.bits(before[2]))
    rows_after = store.read(0, after[0])
    assert all(np.array_equal(ref.bits(rows_after[k]), ref.bits(rows_before[k])) for k in rows_before)
    assert all(np.array_equal(ref.bits(v), ref.bits(params[k])) for k, v in deng.get_params(0).items())
    assert all(torch.equal(v, pol_params[k]) for k, v in world["ar"].state_dict().items())
    # ... and the dynamics' call counter did not move: the loop now draws what an untouched twin's loop draws
    other = world["twin"]()
    s2 = _engine.TrajStore(od, ad, 8, 24)
    a, b = _loop(world, dyn, store, init, 3, 2, eps), _loop(world, other, s2, init, 3, 2, eps)
    assert a[0] == b[0] and a[3] == b[3]
    ra, rb = store.read(0, a[0]), s2.read(0, b[0])
    assert all(np.array_equal(ref.bits(ra[k]), ref.bits(rb[k])) for k in ra)
    for s in (store, s2, wide_store, few_traj, few_rows):
        s.close()


# ---- 3. the loop against a per-step replay through the public calls ---------------------------------------------------------------------------
def _loop_equals_its_replay(world, dyn, twin, store, init, length, lag, eps, pol=None):
    """One loop of ``dyn`` and ``pol`` over ``init`` into ``store``, checked against the store's own book, the enqueue plan and a replay of
    every step through orl_autoreg_sample / orl_dyn_step on the loop's own rows (bit for bit at lag 0, where the replay launches the
    loop's shapes).  ``twin``'s call counter must equal ``dyn``'s before the call and does so again after it.  -> (rows, step sizes, got)"""
    n_traj = len(init)
    rows, rew_sum, returns, enq, ms = _loop(world, dyn, store, init, length, lag, eps, pol=pol)
    got, sizes = _store_equals_its_book(world, store, rows, returns, n_traj)
    per_traj = np.bincount(got["traj_idx"], minlength=n_traj)
    print(f"lag {lag}: {rows} transitions, survivors {sizes}, {int((per_traj == length).sum())} of full length, {enq} steps enqueued, "
          f"loop {ms:.3f} ms")
    assert sizes[0] == n_traj
    assert np.array_equal(ref.bits(got["obs"][:n_traj]), ref.bits(init))
    counts = sizes[1:] + [int((got["term"][rows - sizes[-1]:] == 0).sum())] + [0] * length
    assert enq == len(fref.enqueue_plan(n_traj, counts[:length], lag))
    assert abs(rew_sum - got["rew"].astype(np.float64).sum()) <= 1e-9 * np.abs(got["rew"]).astype(np.float64).sum()
    # step k through orl_autoreg_sample / orl_dyn_step on the loop's own rows; the twin's call counter runs with the loop's
    peng = (pol or world["ar"]).loop_engine()
    teng, mode, coef = twin.loop_engine()
    eps_h, off, worst = eps.cpu().numpy(), 0, {}
    for k, n in enumerate(sizes):
        s = slice(off, off + n)
        act = peng.autoreg_sample(got["obs"][s][None], eps_h[k, :n][None])[0]
        nxt, rew, _, _, _ = teng.step(got["obs"][s][None], got["act"][s][None], None, None, "aleatoric", coef)
        for name, a, b in (("act", act, got["act"][s]), ("next_obs", nxt[0], got["next_obs"][s]), ("rew", rew[0], got["rew"][s])):
            assert np.isfinite(a).all() and np.isfinite(b).all()
            d = float(np.abs(a.astype(np.float64) - b).max()) / max(float(np.abs(b).max()), 1e-30)
            worst[name] = max(worst.get(name, 0.0), d)
            if lag == 0:
                assert np.array_equal(ref.bits(a), ref.bits(b)), (name, k)
        off += n
    print(f"lag {lag}: largest difference to the replay, relative to each array's scale: {worst}")
    assert all(v <= 1e-4 for v in worst.values()), worst
    for _ in range(enq - len(sizes)):       # the steps the loop enqueued on rows that had all ended advanced its dynamics' call counter too
        twin.step_device(torch.zeros((3, world["od"]), device=DEV), torch.zeros((3, world["ad"]), device=DEV))
    return rows, sizes, got


@pytest.mark.parametrize("lag", [0, 2, 6])
def test_loop_matches_a_per_step_replay(world, lag):
    from offlinerlkit import _engine
    od, ad, init = world["od"], world["ad"], world["init"]
    dyn, twin = world["twin"](), world["twin"]()
    torch.manual_seed(123)
    eps = torch.randn((LENGTH, N_TRAJ, ad), device=DEV)
    store = _engine.TrajStore(od, ad, N_TRAJ, N_TRAJ * LENGTH)
    _, sizes, _ = _loop_equals_its_replay(world, dyn, twin, store, init, LENGTH, lag, eps)
    assert len(sizes) >= 3 and 0 < sizes[1] < N_TRAJ and 0 < sizes[2] < sizes[1]      # the thinning is not vacuous
    store.close()


@pytest.mark.parametrize("lag", [0, 2])
def test_loop_matches_its_replay_around_a_regrowth(world, lag):
    """ONE policy engine (a fresh one: its loop workspaces start empty), one dynamics and one store, three loops of 8, 40 and 8
    trajectories: the second regrows the row workspaces of the sampling and of the loop, the third views 8 rows at the front of the
    40-row allocation.  Every call equals its replay the way a first call does."""
    from offlinerlkit import _engine
    from offlinerlkit.policy import AutoregressivePolicy
    od, ad, init, length = world["od"], world["ad"], world["init"], 3
    torch.manual_seed(17)
    pol = AutoregressivePolicy(od, ad, [32, 32], 1e-3, DEV)
    dyn, twin = world["twin"](), world["twin"]()
    store = _engine.TrajStore(od, ad, 40, 40 * length)
    row0 = 0
    for n in (8, 40, 8):
        eps = torch.randn((length, n, ad), device=DEV)
        rows, sizes, _ = _loop_equals_its_replay(world, dyn, twin, store, init[row0:row0 + n], length, lag, eps, pol=pol)
        assert n <= rows <= n * length
        row0 += n
    store.close()


# ---- 4. everything dies at step 0 -------------------------------------------------------------------------------------------------------------
def test_everything_dies_at_step_0(world):
    from offlinerlkit import _engine
    od, ad = world["od"], world["ad"]
    rng = np.random.RandomState(2)
    dead = np.stack([rng.uniform(3.0, 5.0, N_TRAJ), rng.uniform(-1.5, 1.5, N_TRAJ)], 1).astype(np.float32)     # outside [0.2, 1.0] by many model steps
    torch.manual_seed(9)
    eps = torch.randn((5, N_TRAJ, ad), device=DEV)
    a, b = world["twin"](), world["twin"]()
    shared, s1, s2 = (_engine.TrajStore(od, ad, N_TRAJ, N_TRAJ * 5) for _ in range(3))
    rows, _, returns, enq, _ = _loop(world, a, shared, dead, 5, 2, eps)
    print(f"dead start: {rows} rows, {enq} steps enqueued")
    assert rows == N_TRAJ and enq <= 3 and enq == len(fref.enqueue_plan(N_TRAJ, [0] * 5, 2))
    got, sizes = _store_equals_its_book(world, shared, rows, returns, N_TRAJ)
    assert sizes == [N_TRAJ] and got["term"].all() and shared.live_count() == 0
    # the same store again (the loop resets it) against a fresh one, behind the same history on a twin
    assert _loop(world, b, s1, dead, 5, 2, eps)[0] == N_TRAJ
    ra = _loop(world, a, shared, world["init"], 5, 2, eps)
    rb = _loop(world, b, s2, world["init"], 5, 2, eps)
    assert ra[0] == rb[0] > N_TRAJ and ra[3] == rb[3] and np.array_equal(ref.bits(ra[2]), ref.bits(rb[2])) and ra[1] == rb[1]
    ga, gb = shared.read(0, ra[0]), s2.read(0, rb[0])
    assert all(np.array_equal(ref.bits(ga[k]), ref.bits(gb[k])) for k in ga)
    _store_equals_its_book(world, shared, ra[0], ra[2], N_TRAJ)
    for s in (shared, s1, s2):
        s.close()


# ---- 5. reproducibility and isolation ---------------------------------------------------------------------------------------------------------
def _host(roll):
    return {k: ref.bits(v) for k, v in roll.to_host().items()}


def test_fused_rollout_reproduces_and_leaves_the_unfused_path_alone(world):
    from offlinerlkit import _engine
    from offlinerlkit.policy.rcsl import epoch_order
    od, ad, init = world["od"], world["ad"], world["init"]
    pol = _rcsl_policy(None, world["ar"], od, ad)
    a, b = world["twin"](), world["twin"]()

    def run(dyn, fused, n=N_TRAJ, seed=31, **kw):
        pol.dynamics = dyn
        torch.manual_seed(seed)
        return pol.rollout_device(init[:n], 4, fused=fused, **kw)
    # twin a: unfused, fused, unfused.  twin b: unfused, as many plain steps as the fused rollout enqueued, unfused
    a1, a1i = run(a, False)
    fa, fai = run(a, True)
    a2, a2i = run(a, False)
    b1, b1i = run(b, False)
    assert all(np.array_equal(v, _host(b1)[k]) for k, v in _host(a1).items())
    assert list(fai.keys()) == ["num_transitions", "reward_mean", "returns", "steps_enqueued", "loop_ms"] and 1 <= fai["steps_enqueued"] <= 4
    for _ in range(fai["steps_enqueued"]):
        b.step_device(torch.zeros((3, od), device=DEV), torch.zeros((3, ad), device=DEV))
    b2, b2i = run(b, False)
    assert a2i["num_transitions"] == b2i["num_transitions"] and np.array_equal(ref.bits(a2i["returns"]), ref.bits(b2i["returns"]))
    assert all(np.array_equal(v, _host(b2)[k]) for k, v in _host(a2).items())
    # two fused rollouts under one seed on twins (call counters equal again) are the same bits
    fb, fbi = run(b, True)
    fa2, fa2i = run(a, True)
    assert fa2i["num_transitions"] == fbi["num_transitions"] and fa2i["steps_enqueued"] == fbi["steps_enqueued"]
    assert np.array_equal(ref.bits(fa2i["returns"]), ref.bits(fbi["returns"])) and fa2i["reward_mean"] == fbi["reward_mean"]
    assert all(np.array_equal(v, _host(fb)[k]) for k, v in _host(fa2).items())
    h = fa2.to_host()
    assert list(h.keys()) == ref.KEYS and len(h["obss"]) == fa2i["num_transitions"] > N_TRAJ
    assert abs(fa2i["reward_mean"] - h["rewards"].astype(np.float64).mean()) <= 1e-9 * np.abs(h["rewards"]).astype(np.float64).mean()
    # n_traj 1 and 257, every lag the tool measures
    for n, lag in ((1, 2), (257, 0), (257, 1), (257, 4)):
        r, info = run(a, True, n=n, lag=lag)
        hh = r.to_host()
        assert n <= info["num_transitions"] <= 4 * n and all(np.isfinite(hh[k]).all() for k in ("obss", "actions", "next_obss", "rewards", "rtgs"))
        assert np.array_equal(hh["traj_idxs"][:n], np.arange(n))
    # one epoch on the exported ring == one epoch of a twin policy on the same rows loaded from the host
    returns, N = fa2i["returns"], len(h["obss"])
    thr = float(np.median(returns))
    keep = returns[h["traj_idxs"]] > thr
    n_keep = int(keep.sum())
    assert 0 < n_keep < N
    want = _filtered(h, keep)
    single = _engine.DeviceBuffer(od, ad)
    single.reserve(n_keep)
    assert fa2.export(single, thr) == (n_keep, int((returns > thr).sum()))
    _same_rows(_ring_rows(single, 0, n_keep), want)
    loaded = _engine.DeviceBuffer(od, ad)
    loaded.load(want["obs"], want["act"], want["nobs"], want["rew"], want["term"])
    order = epoch_order(n_keep, 64, generator=torch.Generator().manual_seed(9))
    pa, pb = _rcsl_policy(None, None, od, ad, seed=4), _rcsl_policy(None, None, od, ad, seed=4)
    ma, mb = pa.learn_epoch(single, order, 64), pb.learn_epoch(loaded, order, 64)
    assert list(ma) == list(mb) and all(np.float32(ma[k]).view(np.uint32) == np.float32(mb[k]).view(np.uint32) for k in ma), (ma, mb)
    sa, sb = pa.state_dict(), pb.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa) and np.isfinite(ma["loss"])
    for x in (single, loaded):
        x.close()
