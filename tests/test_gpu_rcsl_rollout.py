"""GPU: the RCSL rollout on the device -- the trajectory store (orl_traj_*: termination, rows with trajectory index / accumulated return /
return-to-go, stable compaction, float64 returns) against the numpy bookkeeping of rcsl_rollout_ref.py, ``rollout_device`` against
``rollout``, the thresholded export into the ring ``learn_epoch`` reads, ``collect_rollouts_device`` and ``RcslPolicyTrainer`` on both."""
import os

import numpy as np
import pytest
import torch

import rcsl_cases as rc
import rcsl_rollout_ref as ref
from helpers import GOLDEN_DIR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TERM_FIXTURE = {"TERM_NONE": "fn_default", "TERM_HALFCHEETAH": "fn_halfcheetah", "TERM_HOPPER": "fn_hopper", "TERM_WALKER2D": "fn_walker2d",
                "TERM_ANT": "fn_ant", "TERM_HUMANOID": "fn_humanoid", "TERM_PEN": "fn_pen"}
t = lambda x: torch.tensor(x, device=DEV)


def _steps_against_the_book(kind, obs, act, nobs, done, steps, rew_of):
    """``steps`` append_steps on a fresh store -- step k is fed the first n_live rows of (obs, act, nobs) with the verdicts ``done`` and
    the rewards ``rew_of(k, n_live)`` -- against HostBook on the same arrays: every column, the survivors and the counts, bit for bit"""
    from offlinerlkit import _engine
    n, od, ad = obs.shape[0], obs.shape[1], act.shape[1]
    store = _engine.TrajStore(od, ad, n, steps * n)
    book = ref.HostBook(n)
    live, rew_abs = n, 0.0
    for k in range(steps):
        rew = rew_of(k, live)
        mask = book.step(obs[:live], act[:live], nobs[:live], rew[:, None], done[:live, None])
        alive = torch.full((live, od), -7.0, device=DEV)
        n_alive = store.append_step(kind, t(obs[:live]), t(act[:live]), t(nobs[:live]), t(rew), alive)
        assert n_alive == int(mask.sum()), (k, n_alive, int(mask.sum()))
        assert np.array_equal(ref.bits(alive[:n_alive].cpu().numpy()), ref.bits(nobs[:live][mask])), k
        assert (alive[n_alive:] == -7.0).all()                       # nothing behind the survivors is written
        rew_abs += float(np.abs(rew).astype(np.float64).sum())
        live = n_alive
        if live == 0:
            break
    want, winfo = book.finish()
    rows, rew_sum, returns = store.finish()
    assert rows == winfo["num_transitions"]
    got = store.read(0, rows)
    for gk, wk in (("obs", "obss"), ("next_obs", "next_obss"), ("act", "actions"), ("acc_ret", "acc_rets")):
        assert got[gk].dtype == want[wk].dtype and np.array_equal(ref.bits(got[gk]), ref.bits(want[wk])), (gk, k)
    assert np.array_equal(ref.bits(got["rew"]), ref.bits(want["rewards"].ravel()))
    assert np.array_equal(got["term"], want["terminals"].ravel().astype(np.float32))
    assert np.array_equal(got["traj_idx"], want["traj_idxs"])
    assert got["rtg"].dtype == np.float64 and np.array_equal(ref.bits(got["rtg"]), ref.bits(want["rtgs"].ravel()))
    assert returns.dtype == np.float64 and np.array_equal(ref.bits(returns), ref.bits(winfo["returns"]))
    assert abs(rew_sum - book.rewards_arr.sum()) <= 1e-9 * rew_abs, (rew_sum, book.rewards_arr.sum(), rew_abs)
    assert store.finish()[0] == rows and np.array_equal(ref.bits(store.read(0, rows)["rtg"]), ref.bits(got["rtg"]))      # twice: harmless
    store.close()
    return rows


# ---- 1. the store against numpy, every termination kind ---------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [368, 1, 255, 600])
@pytest.mark.parametrize("kind", sorted(TERM_FIXTURE))
def test_store_matches_the_numpy_bookkeeping(kind, rows):
    """the fixture's rows and the reference's own verdicts on them (NaN rows included); 368 = the whole fixture (two blocks), 1 row, one
    short block, three blocks with a partial last one (the fixture's rows repeated)"""
    from offlinerlkit.utils import termination_fns as tf
    g = np.load(os.path.join(GOLDEN_DIR, "mb_termination.npz"))
    assert g["obs"].shape[0] == 368 > 256
    pick = np.arange(rows) % 368
    obs, act, nobs = g["obs"][pick], g["act"][pick], g["next_obs"][pick]
    done = np.asarray(g[TERM_FIXTURE[kind]]).astype(bool).ravel()[pick]
    rew_of = lambda k, n: (np.linspace(-3.0, 5.0, n) + 0.37 * k).astype(np.float32)
    _steps_against_the_book(getattr(tf, kind), obs, act, nobs, done, 3, rew_of)


# ---- 2. more than 256 blocks ----------------------------------------------------------------------------------------------------------------
def test_store_beyond_256_blocks():
    """70 000 rows = 274 blocks: the sum of the counts of the blocks in front takes its second trip (b += 256) above 65 536 rows"""
    from offlinerlkit.utils import termination_fns as tf
    n = 70_000
    rng = np.random.RandomState(3)
    nobs = np.stack([rng.uniform(0.0, 1.2, n), rng.standard_normal(n)], 1).astype(np.float32)
    obs = rng.standard_normal((n, 2)).astype(np.float32)
    act = rng.standard_normal((n, 3)).astype(np.float32)
    done = np.asarray(tf.termination_fn_ant(obs, act, nobs)).astype(bool).ravel()
    assert 0.25 * n < done.sum() < 0.42 * n
    rew_of = lambda k, m: (np.linspace(-1.0, 2.0, m) + 0.5 * k).astype(np.float32)
    assert _steps_against_the_book(tf.TERM_ANT, obs, act, nobs, done, 2, rew_of) > n + 65_536 // 2


# ---- 3. rollout_device == rollout -----------------------------------------------------------------------------------------------------------
N_TRAJ, LENGTH = 600, 4


def _rcsl_policy(dynamics, rollout_policy, od, ad, seed=0):
    from offlinerlkit.modules import RcslModule
    from offlinerlkit.nets import MLP
    from offlinerlkit.policy import RcslPolicy
    torch.manual_seed(seed)
    mod = RcslModule(MLP(input_dim=od + 1, hidden_dims=[32, 32], output_dim=ad), DEV)
    return RcslPolicy(dynamics, rollout_policy, mod, torch.optim.Adam(mod.parameters(), lr=1e-3), DEV)


@pytest.fixture(scope="module")
def rolled(tmp_path_factory):
    """Two EnsembleDynamics with the same parameters, scaler, elites, engine seed and call counter, one untrained AutoregressivePolicy,
    the same torch seed: the host rollout through the first, the device rollout through the second."""
    from test_gpu_training import AD, OD, make_dataset
    from offlinerlkit.buffer import ReplayBuffer
    from offlinerlkit.dynamics import EnsembleDynamics
    from offlinerlkit.modules import EnsembleDynamicsModel
    from offlinerlkit.policy import AutoregressivePolicy
    from offlinerlkit.utils.logger import Logger
    from offlinerlkit.utils.scaler import StandardScaler
    from offlinerlkit.utils.termination_fns import TERM_ANT, termination_fn_ant
    tmp = tmp_path_factory.mktemp("rcsl_rollout")
    torch.manual_seed(5)
    np.random.seed(5)
    ds = make_dataset(n_episodes=300)
    logger = Logger(str(tmp), {"consoleout_backup": "stdout", "dynamics_training_progress": "csv"})

    def dynamics():
        model = EnsembleDynamicsModel(OD, AD, [64, 64], num_ensemble=5, num_elites=3, weight_decays=[2.5e-5, 5e-5, 1e-4], device=DEV)
        d = EnsembleDynamics(model, torch.optim.Adam(model.parameters(), lr=1e-3), StandardScaler(), termination_fn_ant,
                             penalty_coef=0.5, uncertainty_mode="aleatoric")
        d.set_engine_options(seed=77)
        return d
    dyn_a = dynamics()
    data = ReplayBuffer(len(ds["rewards"]), (OD,), np.float32, AD, np.float32, device=DEV)
    data.load_dataset(ds)
    dyn_a.train(data.sample_all(), logger, max_epochs=3, max_epochs_since_update=3)           # saves into logger.model_dir
    dyn_b = dynamics()
    dyn_b.load(logger.model_dir)
    assert dyn_b.term_kind == TERM_ANT
    ar = AutoregressivePolicy(OD, AD, [32, 32], 1e-3, DEV)
    pol = _rcsl_policy(dyn_a, ar, OD, AD)
    rng = np.random.RandomState(1)
    init = np.stack([rng.uniform(0.25, 0.95, N_TRAJ), rng.uniform(-1.5, 1.5, N_TRAJ)], 1).astype(np.float32)   # x0 around TERM_ANT's 0.2 / 1.0 bounds
    torch.manual_seed(123)
    host, hinfo = pol.rollout(init, LENGTH)
    pol.dynamics = dyn_b
    torch.manual_seed(123)
    roll, dinfo = pol.rollout_device(init, LENGTH)
    return dict(pol=pol, init=init, host=host, hinfo=hinfo, roll=roll, dinfo=dinfo, od=OD, ad=AD)


def test_rollout_device_matches_the_host_rollout_bit_for_bit(rolled):
    host, hinfo, roll, dinfo = rolled["host"], rolled["hinfo"], rolled["roll"], rolled["dinfo"]
    # not vacuous (on the HOST rollout): some but not all trajectories end in each of the first two steps, one at least reaches the last
    term = host["terminals"].ravel()
    n1 = int((~term[:N_TRAJ]).sum())
    n2 = int((~term[N_TRAJ:N_TRAJ + n1]).sum())
    per_traj = np.bincount(host["traj_idxs"], minlength=N_TRAJ)
    print(f"host rollout: {len(term)} transitions, survivors {N_TRAJ} -> {n1} -> {n2}, {int((per_traj == LENGTH).sum())} of full length")
    assert 0 < n1 < N_TRAJ and 0 < n2 < n1 and (per_traj == LENGTH).any()
    got = roll.to_host()
    assert list(got.keys()) == list(host.keys()) == ref.KEYS
    for k in ref.KEYS:
        assert got[k].dtype == host[k].dtype and got[k].shape == host[k].shape, (k, got[k].dtype, got[k].shape, host[k].dtype, host[k].shape)
        assert np.array_equal(ref.bits(got[k]), ref.bits(host[k])), k
    assert list(dinfo.keys()) == list(hinfo.keys())
    assert dinfo["num_transitions"] == hinfo["num_transitions"] == len(term)
    assert dinfo["returns"].dtype == np.float64 and np.array_equal(ref.bits(dinfo["returns"]), ref.bits(hinfo["returns"]))
    print(f"reward_mean: device {dinfo['reward_mean']!r}, host {hinfo['reward_mean']!r}")
    assert abs(dinfo["reward_mean"] - hinfo["reward_mean"]) <= 1e-9 * np.abs(host["rewards"]).astype(np.float64).mean()


# ---- 4. export ------------------------------------------------------------------------------------------------------------------------------
def _ring_rows(ring, row0, n):
    obs, act, nobs, rew, term = ring.read_rows(row0, n)
    return dict(obs=obs, act=act, nobs=nobs, rew=rew.ravel(), term=term.ravel())


def _filtered(host, keep):
    return dict(obs=host["obss"][keep], act=host["actions"][keep], nobs=host["next_obss"][keep],
                rew=np.float32(host["rtgs"].ravel()[keep]), term=host["terminals"].ravel()[keep].astype(np.float32))


def _same_rows(got, want):
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(ref.bits(got[k]), ref.bits(want[k])), k


def test_export_filters_by_return_and_feeds_learn_epoch(rolled):
    from offlinerlkit import _engine
    from offlinerlkit.policy.rcsl import epoch_order
    host, hinfo, roll, od, ad = rolled["host"], rolled["hinfo"], rolled["roll"], rolled["od"], rolled["ad"]
    returns, N = hinfo["returns"], len(host["obss"])
    thr = float(np.median(returns))
    keep = returns[host["traj_idxs"]] > thr
    n_keep, t_keep = int(keep.sum()), int((returns > thr).sum())
    assert 0 < t_keep < N_TRAJ and 0 < n_keep < N
    want = _filtered(host, keep)
    ring = _engine.DeviceBuffer(od, ad)
    ring.reserve(2 * n_keep + 5)
    assert roll.export(ring, thr) == (n_keep, t_keep) and ring.size() == n_keep
    _same_rows(_ring_rows(ring, 0, n_keep), want)
    assert roll.export(ring, thr) == (n_keep, t_keep) and ring.size() == 2 * n_keep         # the second one lands behind the first
    _same_rows(_ring_rows(ring, 0, n_keep), want)
    _same_rows(_ring_rows(ring, n_keep, n_keep), want)
    assert not _ring_rows(ring, 2 * n_keep, 5)["obs"].any()
    every = _engine.DeviceBuffer(od, ad)
    every.reserve(N)
    assert roll.export(every) == (N, N_TRAJ) and every.size() == N
    _same_rows(_ring_rows(every, 0, N), _filtered(host, np.ones(N, bool)))
    small = _engine.DeviceBuffer(od, ad)
    small.reserve(n_keep - 1)
    with pytest.raises(RuntimeError, match="room for"):
        roll.export(small, thr)
    assert small.size() == 0 and not any(v.any() for v in _ring_rows(small, 0, n_keep - 1).values())      # nothing was written
    assert roll.export(small, float("nan")) == (0, 0) and roll.export(small, float("inf")) == (0, 0)      # (numpy: nothing is > NaN)
    # one epoch on the exported ring == one epoch of a twin on the same rows loaded from the host dict
    single = _engine.DeviceBuffer(od, ad)
    single.reserve(n_keep)
    roll.export(single, thr)
    loaded = _engine.DeviceBuffer(od, ad)
    loaded.load(want["obs"], want["act"], want["nobs"], want["rew"], want["term"])
    B = 64
    assert n_keep % B != 0
    order = epoch_order(n_keep, B, generator=torch.Generator().manual_seed(9))
    pa, pb = _rcsl_policy(None, None, od, ad, seed=4), _rcsl_policy(None, None, od, ad, seed=4)
    ma, mb = pa.learn_epoch(single, order, B), pb.learn_epoch(loaded, order, B)
    assert list(ma) == list(mb) and all(np.float32(ma[k]).view(np.uint32) == np.float32(mb[k]).view(np.uint32) for k in ma), (ma, mb)
    sa, sb = pa.state_dict(), pb.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa) and np.isfinite(ma["loss"])
    for b in (ring, every, small, single, loaded):
        b.close()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from offlinerlkit import _engine
    from offlinerlkit.utils import termination_fns as tf

    class Dyn:
        term_kind = tf.TERM_ANT

        def step_device(self, o, a):
            raise AssertionError("not reached")

    class NoKind(Dyn):
        term_kind = tf.term_kind(tf.obs_unnormalization(tf.termination_fn_hopper, 0.0, 1.0))

    class HostOnly:
        act_dim = 2

        def select_action(self, obs, noise=None):
            raise AssertionError("not reached")

    class Frozen(HostOnly):
        def sample_init_noise(self, n):
            raise AssertionError("not reached")

        def select_action_device(self, obs):
            raise AssertionError("not reached")

    class Good(HostOnly):
        def select_action_device(self, obs):
            raise AssertionError("not reached")
    init = np.zeros((4, 2), np.float32)
    with pytest.raises(NotImplementedError, match="term_kind"):
        _rcsl_policy(NoKind(), Good(), 2, 2).rollout_device(init, 1)
    with pytest.raises(NotImplementedError, match="select_action_device"):
        _rcsl_policy(Dyn(), HostOnly(), 2, 2).rollout_device(init, 1)
    with pytest.raises(NotImplementedError, match="sample_init_noise"):
        _rcsl_policy(Dyn(), Frozen(), 2, 2).rollout_device(init, 1)
    with pytest.raises(NotImplementedError, match="needs both a dynamics model and a rollout"):
        _rcsl_policy(None, Good(), 2, 2).rollout_device(init, 1)
    od, ad, n = 11, 3, 6
    store = _engine.TrajStore(od, ad, n, 2 * n + 1)
    z = lambda rows, c: torch.zeros((rows, c), device=DEV)
    step = lambda kind, rows: store.append_step(kind, z(rows, od), z(rows, ad), z(rows, od), torch.zeros(rows, device=DEV), z(rows, od))
    with pytest.raises(RuntimeError, match="trajectories are live"):
        step(tf.TERM_NONE, n - 1)
    with pytest.raises(RuntimeError, match="reads observation column 26"):
        step(tf.TERM_PEN, n)
    with pytest.raises(RuntimeError, match="unknown termination kind"):
        step(7, n)
    nobs = z(n, od)
    with pytest.raises(RuntimeError, match="must not overlap"):
        store.append_step(tf.TERM_NONE, z(n, od), z(n, ad), nobs, torch.zeros(n, device=DEV), nobs)
    with pytest.raises(RuntimeError, match="created for"):
        store.reset(n + 1)
    assert step(tf.TERM_NONE, n) == n and step(tf.TERM_NONE, n) == n          # after the refusals the store works
    with pytest.raises(RuntimeError, match="capacity"):
        step(tf.TERM_NONE, n)                                                  # 2 n + 1 rows of room, 3 n asked for
    loaded = _engine.DeviceBuffer(od, ad)
    loaded.load(np.zeros((3, od), np.float32), np.zeros((3, ad), np.float32), np.zeros((3, od), np.float32), np.zeros(3), np.zeros(3))
    other = _engine.DeviceBuffer(od + 1, ad)
    other.reserve(64)
    with pytest.raises(RuntimeError, match="orl_traj_finish"):
        store.export(other)
    rows, _, returns = store.finish()
    assert rows == 2 * n and not returns.any()
    with pytest.raises(RuntimeError, match="not a ring"):
        store.export(loaded)
    with pytest.raises(RuntimeError, match="differ"):
        store.export(other)
    assert loaded.size() == 3 and other.size() == 0
    store.reset(n - 2)                                                         # and a new, smaller rollout starts clean
    assert step(tf.TERM_HUMANOID, n - 2) == 0 and store.finish()[0] == n - 2   # x0 = 0 < 1: all done
    assert np.array_equal(store.read(0, n - 2)["traj_idx"], np.arange(n - 2)) and store.read(0, n - 2)["term"].all()
    for b in (store, loaded, other):
        b.close()


# ---- 6. the collection loop -------------------------------------------------------------------------------------------------------------------
def test_collect_rollouts_device(rolled):
    from offlinerlkit.policy.rcsl import collect_rollouts_device
    pol, init = rolled["pol"], rolled["init"]
    batch, horizon = 200, 3
    # the first epoch alone, to place the threshold at its median and to know what each epoch keeps
    rng = np.random.RandomState(8)
    log = []
    inner = pol.rollout_device

    def spy(init_obss, length, store=None):
        roll, info = inner(init_obss, length, store=store)
        log.append((roll, info["returns"].copy()))
        return roll, info
    pol.rollout_device = spy
    try:
        _, probe = inner(init[rng.randint(len(init), size=batch)], horizon)
        thr = float(np.median(probe["returns"]))
        ring, info = collect_rollouts_device(pol, init, batch, horizon, thr, num_need_traj=batch // 2 + batch // 8, max_epochs=6,
                                             capacity_rows=6 * batch * horizon, rng=np.random.RandomState(8))
        per_epoch = [int((r > thr).sum()) for _, r in log]
        print(f"collect: threshold {thr:.4f}, kept per epoch {per_epoch}, rows {ring.size()}")
        assert info["epochs"] == len(log) == 2 and all(0 < k < batch for k in per_epoch)
        assert info["num_traj"] == sum(per_epoch) == len(info["returns"]) and info["returns"].dtype == np.float64
        assert info["max_return"] == max(info["returns"]) == max(r.max() for _, r in log)
        assert (info["returns"] > thr).all()
        # the ring holds what the epochs' own exports into a second ring hold: the last store still has the last epoch's rows
        last_rows = int((log[-1][1][log[-1][0].to_host()["traj_idxs"]] > thr).sum())
        assert 0 < last_rows < ring.size() <= 2 * batch * horizon
        got = _ring_rows(ring, ring.size() - last_rows, last_rows)
        h = log[-1][0].to_host()
        _same_rows(got, _filtered(h, log[-1][1][h["traj_idxs"]] > thr))
        ring.close()
        log.clear()
        ring, info = collect_rollouts_device(pol, init, batch, horizon, float("inf"), num_need_traj=1, max_epochs=3, capacity_rows=16,
                                             rng=np.random.RandomState(8))
        assert info["epochs"] == len(log) == 3 and info["num_traj"] == 0 and ring.size() == 0 and len(info["returns"]) == 0
        ring.close()
    finally:
        del pol.rollout_device


# ---- 7. the trainer ---------------------------------------------------------------------------------------------------------------------------
def test_trainer_accepts_the_rollout_dict_and_the_exported_buffer(rolled, tmp_path):
    from offlinerlkit import _engine
    from offlinerlkit.policy_trainer import RcslPolicyTrainer
    from offlinerlkit.utils.logger import Logger
    roll, od, ad = rolled["roll"], rolled["od"], rolled["ad"]
    assert (od, ad) == (rc.PM_OD, rc.PM_AD)
    host = roll.to_host()
    assert "obss" in host and "observations" not in host
    ring = _engine.DeviceBuffer(od, ad)
    ring.reserve(len(host["obss"]))
    roll.export(ring)
    losses = []
    for name, data in (("dict", host), ("ring", ring)):
        pol = _rcsl_policy(None, None, od, ad, seed=11)
        os.makedirs(tmp_path / name)
        logger = Logger(str(tmp_path / name), {"policy_training_progress": "csv"})
        torch.manual_seed(21)
        tr = RcslPolicyTrainer(pol, rc.PointMassEnv(5), None, data, 0.0, logger, 5, epoch=2, batch_size=64, offline_ratio=0, eval_episodes=1,
                               fused=True)
        assert np.isfinite(tr.train()["last_10_performance"])
        rows = [ln.split(",") for ln in open(tmp_path / name / "record" / "policy_training_progress.csv").read().strip().split("\n")]
        losses.append([r[rows[0].index("loss")] for r in rows[1:]])
        assert pol.engine.step_count() == 2 * -(-len(host["obss"]) // 64)
    print("trainer losses:", losses)
    assert len(losses[0]) == 2 and losses[0] == losses[1] and np.isfinite([float(x) for x in losses[0]]).all()
    assert tr._dbuf is ring                                                    # used as it is: nothing was uploaded
    ring.close()
