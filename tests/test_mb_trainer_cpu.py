"""CPU: the termination functions and MBPolicyTrainer's reference loop against fixtures of the REAL reference
(tests/golden/make_mb_trainer_golden.py)."""
import os

import numpy as np
import pytest
import torch

import mb_trainer_fakes as mf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def test_termination_fns_match_reference():
    from offlinerlkit.utils import termination_fns as T
    g = np.load(os.path.join(GOLD, "mb_termination.npz"), allow_pickle=False)
    obs, act, nxt = g["obs"], g["act"], g["next_obs"]
    assert np.isnan(nxt).any() and np.isinf(nxt).any()
    for name in mf.TERM_FNS:
        got = getattr(T, "termination_fn_" + name)(obs, act, nxt)
        ref = g["fn_" + name]
        assert got.dtype == ref.dtype and got.shape == ref.shape == (len(obs), 1), name
        assert np.array_equal(got, ref), name
    assert bool(g["door_is_none"][0]) and T.termination_fn_door(obs, act, nxt) is None
    wrapped = T.obs_unnormalization(T.termination_fn_hopper, np.float32(0.5), np.float32(2.0))
    assert np.array_equal(wrapped(obs, act, nxt), T.termination_fn_hopper(obs * 2.0 + 0.5, act, nxt * 2.0 + 0.5))


def test_get_termination_fn_name_order():
    from offlinerlkit.utils import termination_fns as T
    g = np.load(os.path.join(GOLD, "mb_termination.npz"), allow_pickle=False)
    assert [T.get_termination_fn(t).__name__ for t in mf.TASKS] == [str(x) for x in g["task_fn"]]
    assert T.get_termination_fn("pendulum") is T.termination_fn_pendulum        # not pen
    assert T.get_termination_fn("antmaze-umaze-v0") is T.termination_fn_ant     # 'ant' comes before 'maze'
    with pytest.raises(NotImplementedError):
        T.get_termination_fn("cartpole")


def test_termination_kinds():
    from offlinerlkit.utils import termination_fns as T
    kinds = {name: T.term_kind(getattr(T, "termination_fn_" + name)) for name in mf.TERM_FNS + ("door",)}
    assert kinds == {"halfcheetah": T.TERM_HALFCHEETAH, "hopper": T.TERM_HOPPER, "halfcheetahveljump": T.TERM_NONE,
                     "antangle": T.TERM_ANT, "ant": T.TERM_ANT, "walker2d": T.TERM_WALKER2D, "point2denv": T.TERM_NONE,
                     "point2dwallenv": T.TERM_NONE, "pendulum": T.TERM_NONE, "humanoid": T.TERM_HUMANOID, "pen": T.TERM_PEN,
                     "default": T.TERM_NONE, "door": None}
    assert T.term_kind(T.obs_unnormalization(T.termination_fn_hopper, 0.0, 1.0)) is None
    assert T.term_kind(lambda o, a, n: None) is None


def _host_buffer(cap, snaps=None):
    """this package's ReplayBuffer (host add / add_batch) with the reference's host ``sample`` (buffer.py:96-106)"""
    from offlinerlkit.buffer import ReplayBuffer

    class HostBuffer(ReplayBuffer):
        def sample(self, batch_size):
            idx = np.random.randint(0, self._size, size=batch_size)
            return {k: torch.tensor(getattr(self, k)[idx]) for k in ("observations", "actions", "next_observations", "terminals", "rewards")}

        def add_batch(self, *a, **k):
            super().add_batch(*a, **k)
            if snaps is not None:
                snaps.append((np.concatenate([self.observations, self.next_observations, self.actions, self.rewards, self.terminals], 1).copy(),
                              (self._ptr, self._size)))
    return HostBuffer(cap, (mf.OBS,), np.float32, mf.ACT, np.float32)


def test_mb_trainer_matches_reference_trace(tmp_path):
    from offlinerlkit.policy_trainer import MBPolicyTrainer
    from offlinerlkit.utils.logger import Logger
    g = np.load(os.path.join(GOLD, "mb_trainer_trace.npz"), allow_pickle=False)
    logger = Logger(str(tmp_path), {"consoleout_backup": "stdout", "policy_training_progress": "csv", "dynamics_training_progress": "csv"})
    lines = []
    logger.log = lambda s, *a, **k: lines.append(s)
    real = _host_buffer(mf.N_DATA)
    real.load_dataset(mf.dataset())
    snaps = []
    fake = _host_buffer(mf.FAKE_CAP, snaps)
    pol, sched = mf.FakePolicy(), mf.FakeScheduler()
    np.random.seed(mf.SEED)
    res = MBPolicyTrainer(pol, mf.FakeEnv(), real, fake, logger, mf.ROLLOUT, epoch=mf.EPOCHS, step_per_epoch=mf.STEPS, batch_size=mf.BATCH,
                          real_ratio=mf.REAL_RATIO, eval_episodes=mf.EVAL_EPS, lr_scheduler=sched).train()
    with open(tmp_path / "record" / "policy_training_progress.csv") as f:
        csv = f.read().strip().split("\n")
    assert csv[0].split(",") == [str(x) for x in g["csv_header"]]
    assert "eval/episode_reward" not in csv[0].split(",")                        # the reference logs the normalised return only
    rows = np.array([[float(x) if x else np.nan for x in ln.split(",")] for ln in csv[1:]])
    np.testing.assert_allclose(rows, g["csv_rows"], rtol=1e-6, atol=1e-9)
    # every draw: rollout initial states, real rows, model rows (the sums pin the numpy index streams)
    np.testing.assert_allclose(pol.init_sums, g["init_sums"], rtol=1e-7)
    np.testing.assert_allclose(pol.real_sums, g["real_sums"], rtol=1e-7)
    np.testing.assert_allclose(pol.fake_sums, g["fake_sums"], rtol=1e-7)
    assert len(pol.init_sums) == 7                                               # timesteps 0, 3, ..., 18 of 21
    assert [s for s in lines if s.startswith("num rollout")] == [str(x) for x in g["rollout_lines"]]
    assert len(snaps) == len(g["fake_snapshots"])
    for (arr, ps), ref, ref_ps in zip(snaps, g["fake_snapshots"], g["fake_ptr_size"]):
        assert np.array_equal(arr, ref) and tuple(ps) == tuple(int(x) for x in ref_ps)
    assert sched.n == int(g["sched_steps"][0]) == mf.EPOCHS
    assert abs(res["last_10_performance"] - float(g["last_10_performance"][0])) < 1e-9
    assert pol.dynamics.saved == [str(x) for x in g["dyn_saved"]] == ["model"]
    assert all(bool(x) for x in g["ckpt_exists"])
    for p in ("checkpoint/policy.pth", "model/policy.pth", "model/dynamics.pth"):
        assert (tmp_path / p).exists(), p


class _GymnasiumEnv(mf.FakeEnv):
    def reset(self):
        return super().reset(), {}

    def step(self, action):
        o, r, d, i = super().step(action)
        return o, r, d, False, i

    def get_true_observation(self, obs):
        return obs


def test_mb_trainer_horizon_and_gymnasium(tmp_path):
    """gymnasium evaluation needs a horizon; each episode is ``horizon`` steps whatever the terminals; the raw return is logged"""
    from offlinerlkit.policy_trainer import MBPolicyTrainer
    from offlinerlkit.utils.logger import Logger
    logger = Logger(str(tmp_path), {"consoleout_backup": "stdout", "policy_training_progress": "csv"})
    real = _host_buffer(mf.N_DATA)
    real.load_dataset(mf.dataset())
    fake = _host_buffer(mf.FAKE_CAP)
    with pytest.raises(AssertionError, match="Horizon"):
        MBPolicyTrainer(mf.FakePolicy(), _GymnasiumEnv(), real, fake, logger, mf.ROLLOUT)
    np.random.seed(mf.SEED)
    tr = MBPolicyTrainer(mf.FakePolicy(), _GymnasiumEnv(), real, fake, logger, mf.ROLLOUT, epoch=1, step_per_epoch=4, batch_size=mf.BATCH,
                         real_ratio=mf.REAL_RATIO, eval_episodes=2, horizon=5)
    res = tr.train()
    header = open(tmp_path / "record" / "policy_training_progress.csv").read().split("\n")[0].split(",")
    assert "eval/episode_reward" in header and "eval/normalized_episode_reward" not in header
    ev = tr._evaluate()
    assert ev["eval/episode_length"] == [5, 5]
    assert np.isfinite(res["last_10_performance"])
