"""Synthetic inputs of the RCSL fixtures, shared by make_rcsl_golden.py (which feeds them to the real reference) and by the tests (which
feed the same arrays to the numpy oracle and the HIP engine); and the duck-typed env / policy / logger / scheduler that pin
RcslPolicyTrainer.  Pure numpy / torch; no reference code.

Observations are normalised (N(0, 1)), returns-to-go are drawn at the magnitude of D4RL returns (hopper: up to ~3200), so the first layer
sees mixed scales, as it does in run_rcsl.py."""
from collections import OrderedDict

import numpy as np
import torch

import synth

f32 = np.float32
STEPS = 4
CASES = {
    # input width 6: no multiple of 4
    "rcsl_tiny": dict(obs_dim=5, act_dim=2, hidden=[32, 32], B=16, lr=3e-4, seed=71, rtg_hi=600.0, full=True),
    # input width 8: a multiple of 4; unequal layer widths
    "rcsl_odd": dict(obs_dim=7, act_dim=3, hidden=[48, 32, 40], B=24, lr=3e-4, seed=72, rtg_hi=900.0, full=True),
    # run_rcsl.py's shape on hopper
    "rcsl_hopper": dict(obs_dim=11, act_dim=3, hidden=[200] * 4, B=256, lr=1e-3, seed=73, rtg_hi=3200.0, full=False),
}


def make_net(rng, c):
    """MLP(obs_dim + 1, hidden, output_dim=act_dim): keys backbone.model.{0, 2, ..., 2L}.{weight, bias}, nn.Linear's init magnitudes"""
    p, _ = synth.make_backbone(rng, c["obs_dim"] + 1, list(c["hidden"]) + [c["act_dim"]])
    return p


def make_rows(rng, n, c):
    return OrderedDict(observations=rng.standard_normal((n, c["obs_dim"])).astype(f32),
                       actions=np.tanh(rng.standard_normal((n, c["act_dim"]))).astype(f32),
                       rtgs=rng.uniform(0.0, c["rtg_hi"], size=(n, 1)).astype(f32))


def case_inputs(case, run=0):
    """(case dict, initial net, STEPS batches); ``run`` > 0: other weights and batches of the same shape (many-runs tests)"""
    c = CASES[case]
    rng = np.random.RandomState(c["seed"] + 1000 * run)
    net = make_net(rng, c)
    return c, net, [make_rows(rng, c["B"], c) for _ in range(STEPS)]


def epoch_inputs(case, n_runs=3, n_epochs=2):
    """the ordered-epoch test: a dataset of N = 3 B + 5 rows (4 steps, the last holding 5 valid rows) and, per epoch, one row order
    [n_runs, 4 B]: a permutation of [0, N) per run, padded with -1"""
    c = CASES[case]
    B = c["B"]
    n = 3 * B + 5
    rng = np.random.RandomState(c["seed"] + 7)
    data = make_rows(rng, n, c)
    orders = []
    for _ in range(n_epochs):
        o = np.full((n_runs, 4 * B), -1, np.int64)
        for r in range(n_runs):
            o[r, :n] = rng.permutation(n)
        orders.append(o)
    return c, data, orders


def gather(data, idx):
    """rows ``idx`` of the dataset the way the engine's padding reads them: a negative index reads row 0"""
    j = np.where(idx < 0, 0, idx)
    return OrderedDict((k, v[j]) for k, v in data.items())


# ---- trajectory dataset (traj_rtg_datasets) ------------------------------------------------------------------------------------------

def traj_source(use_timeouts=True):
    """a synthetic ``get_dataset()``: episodes ended by terminals and by timeouts, an incomplete last trajectory"""
    rng = np.random.RandomState(5)
    n, od, ad = 260, 3, 2
    d = dict(observations=rng.standard_normal((n, od)).astype(f32), next_observations=rng.standard_normal((n, od)).astype(f32),
             actions=rng.uniform(-1, 1, (n, ad)).astype(f32), rewards=rng.uniform(0, 2, n).astype(f32), terminals=np.zeros(n, bool))
    d["terminals"][[30, 31, 95, 180]] = True
    if use_timeouts:
        d["timeouts"] = np.zeros(n, bool)
        d["timeouts"][[60, 95, 140, 230]] = True
    return d


class TrajEnv:
    def __init__(self, use_timeouts=True):
        self._d = traj_source(use_timeouts)

    def get_dataset(self, h5path=None):
        return self._d


# ---- trainer fakes ---------------------------------------------------------------------------------------------------------------------

T_OBS, T_ACT, T_N, T_BATCH, T_EPOCHS, T_EVAL_EPS, T_SEED, T_GOAL, T_HORIZON = 3, 2, 45, 8, 3, 3, 11, 7.5, 4


def trainer_dataset(shift=0.0):
    """rewards hold the row number: the recording policy reads the batch order off them"""
    rng = np.random.RandomState(4)
    return dict(observations=(rng.standard_normal((T_N, T_OBS)) + shift).astype(f32), next_observations=rng.standard_normal((T_N, T_OBS)).astype(f32),
                actions=rng.standard_normal((T_N, T_ACT)).astype(f32), rewards=np.arange(T_N, dtype=f32), terminals=np.zeros(T_N, bool),
                rtgs=rng.uniform(0, 10, (T_N, 1)).astype(f32))


class RecordingPolicy(torch.nn.Module):
    """learn is a deterministic function of the batch; select_action of (obs, rtg): the logged means pin the batches, the rewards the rtg"""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(2))
        self.orders, self.rtgs_seen, self.mode = [], [], None

    def train(self):
        self.mode = "train"

    def eval(self):
        self.mode = "eval"

    def learn(self, batch):
        assert self.mode == "train"
        self.orders.append(np.asarray(torch.as_tensor(batch["rewards"]).cpu().numpy(), np.int64).ravel())
        o = float(torch.as_tensor(batch["observations"]).double().sum())
        g = float(torch.as_tensor(batch["rtgs"]).double().sum())
        return {"loss": o + 0.25 * g}

    def select_action(self, obs, rtg):
        assert self.mode == "eval" and obs.shape == (1, T_OBS) and tuple(rtg.shape) == (1, 1)
        self.rtgs_seen.append(float(rtg))
        return np.full((1, T_ACT), 0.125 * float(rtg) + 0.5 * float(obs[0, 0]), dtype=np.float32)


class GymEnv:
    """gym convention: reset() -> obs (reset(seed=...) restarts the episode counter), step -> 4-tuple"""

    def __init__(self, normalized=False):
        self.t, self.ep, self.seeds = 0, 0, []
        if normalized:
            self.get_normalized_score = lambda x: x / 20.0

    def reset(self, seed=None):
        if seed is not None:
            self.seeds.append(seed)
            self.ep = 0
        self.t = 0
        return np.full(T_OBS, 0.1 * self.ep, dtype=np.float32)

    def _step(self, action):
        self.t += 1
        done = self.t >= 2 + (self.ep % 3)
        if done:
            self.ep += 1
        return np.full(T_OBS, 0.01 * self.t + 0.1 * self.ep, dtype=np.float32), 0.5 + 0.25 * float(np.sum(action)), done

    def step(self, action):
        o, r, d = self._step(action)
        return o, r, d, {}


class GymnasiumEnv(GymEnv):
    """gymnasium convention of the reference's pointmaze wrapper: reset -> (obs, info), step -> 5-tuple, get_true_observation"""

    def reset(self, seed=None):
        return {"observation": GymEnv.reset(self, seed)}, {}

    def step(self, action):
        o, r, d = self._step(action)
        return {"observation": o}, r, d, False, {}

    def get_true_observation(self, obs):
        return obs["observation"]


class RecordingLogger:
    """the Logger calls the trainer makes, as rows: at every dumpkvs the (key, value) pairs in first-log order (logkv_mean keys hold the
    mean), the timestep, and the exclude argument"""

    def __init__(self, root):
        import os
        self.checkpoint_dir, self.model_dir = os.path.join(root, "checkpoint"), os.path.join(root, "model")
        os.makedirs(self.checkpoint_dir); os.makedirs(self.model_dir)
        self._kv, self._cnt = OrderedDict(), {}
        self.rows, self.timesteps, self.lines, self.closed, self._t = [], [], [], False, None

    def logkv(self, k, v):
        self._kv[k] = v

    def logkv_mean(self, k, v):
        n = self._cnt.get(k, 0)
        self._kv[k] = (self._kv.get(k, 0.0) * n + v) / (n + 1)
        self._cnt[k] = n + 1

    def set_timestep(self, t):
        self._t = t

    def dumpkvs(self, exclude=None):
        assert list(exclude or []) == ["dynamics_training_progress"]
        self.rows.append(OrderedDict((k, float(v)) for k, v in self._kv.items()))
        self.timesteps.append(self._t)
        self._kv, self._cnt = OrderedDict(), {}

    def log(self, s, *a, **k):
        self.lines.append(s)

    def close(self):
        self.closed = True


class CountingScheduler:
    def __init__(self):
        self.n = 0

    def step(self):
        self.n += 1


TRAINER_VARIANTS = OrderedDict([      # name -> (env class, normalized score, eval_env2, horizon)
    ("gym", (GymEnv, False, False, None)),
    ("gym_norm_env2", (GymEnv, True, True, None)),
    ("gymnasium", (GymnasiumEnv, False, False, T_HORIZON)),
    ("gymnasium_env2", (GymnasiumEnv, False, True, T_HORIZON)),
])


def run_trainer(Trainer, variant, **extra):
    """drives a RcslPolicyTrainer class (the reference's or ours) through one variant; returns what the fixture holds"""
    import tempfile
    env_cls, norm, env2, horizon = TRAINER_VARIANTS[variant]
    with tempfile.TemporaryDirectory() as d:
        logger, pol, sched = RecordingLogger(d), RecordingPolicy(), CountingScheduler()
        torch.manual_seed(T_SEED)
        tr = Trainer(pol, env_cls(norm), trainer_dataset(), trainer_dataset(1.0), T_GOAL, logger, T_SEED, eval_env2=env_cls(norm) if env2 else None,
                     epoch=T_EPOCHS, batch_size=T_BATCH, offline_ratio=1 if variant.startswith("gymnasium") else 0, eval_episodes=T_EVAL_EPS,
                     lr_scheduler=sched, horizon=horizon, num_workers=0, **extra)
        res = tr.train()
        import os
        ckpt = [os.path.exists(os.path.join(logger.checkpoint_dir, "policy.pth")), os.path.exists(os.path.join(logger.model_dir, "policy.pth"))]
        seeds = list(tr.eval_env.seeds)
    keys = [list(r.keys()) for r in logger.rows]
    assert all(k == keys[0] for k in keys)
    return dict(keys=np.array(keys[0]), rows=np.array([[r[k] for k in keys[0]] for r in logger.rows], np.float64),
                timesteps=np.array(logger.timesteps, np.int64), last_10=np.array([res["last_10_performance"]], np.float64),
                orders=np.concatenate(pol.orders), order_lens=np.array([len(o) for o in pol.orders], np.int64),
                rtgs_seen=np.array(pol.rtgs_seen, np.float64), sched=np.array([sched.n]), ckpt=np.array(ckpt), seeds=np.array(seeds, np.int64),
                closed=np.array([logger.closed]))


# ---- end-to-end task: return-conditioned control of a point mass ---------------------------------------------------------------------
# obs = position in [-2, 2]^2, action in [-1, 1]^2, x' = clip(x + 0.25 a, -2, 2), reward -|x'|^2, 20 steps per episode (the task of
# tests/test_gpu_training.py).  Mixed-quality data: every episode follows a = clip(-g x + 0.3 noise) with its own gain g ~ U(-1, 1.5):
# negative gains push the mass to the walls (returns down to about -146), gains above 1 drive it to the origin (about -1.3);
# every episode starts at distance 1.2, so both ends of the return range are well populated.  A policy
# conditioned on a high return-to-go must therefore act like a high-gain controller and one conditioned on a low one like a negative-gain
# controller.
PM_OD, PM_AD, PM_T, PM_HID, PM_BATCH, PM_LR, PM_EPOCHS, PM_EPISODES = 2, 2, 20, [64, 64], 256, 1e-3, 10, 1500


class PointMassEnv:
    def __init__(self, seed=0):
        self.rng = np.random.RandomState(seed)
        self.x, self.t = np.zeros(PM_OD, f32), 0

    def reset(self, seed=None):
        if seed is not None:
            self.rng = np.random.RandomState(seed)
        self.t = 0
        phi = self.rng.uniform(0.0, 2.0 * np.pi)          # every episode starts 1.2 from the origin: the return depends on the controller, not the start
        self.x = (1.2 * np.array([np.cos(phi), np.sin(phi)])).astype(f32)
        return self.x.copy()

    def step(self, a):
        a = np.clip(np.asarray(a, f32).reshape(-1), -1, 1)
        self.x = np.clip(self.x + 0.25 * a, -2, 2).astype(f32)
        self.t += 1
        return self.x.copy(), -float((self.x ** 2).sum()), self.t >= PM_T, {}


def pm_dataset(seed=0):
    """-> (dataset with rtgs, per-episode returns)"""
    rng = np.random.RandomState(seed)
    env = PointMassEnv(seed + 1)
    obs, act, nobs, rew, rtg, rets = [], [], [], [], [], []
    for _ in range(PM_EPISODES):
        g = rng.uniform(-1.0, 1.5)
        o, done, rs = env.reset(), False, []
        while not done:
            a = np.clip(-g * o + 0.3 * rng.standard_normal(PM_AD), -1, 1).astype(f32)
            o2, r, done, _ = env.step(a)
            obs.append(o); act.append(a); nobs.append(o2); rs.append(r)
            o = o2
        rs = np.asarray(rs, f32)
        rew.append(rs); rtg.append(np.cumsum(rs[::-1])[::-1]); rets.append(float(rs.sum()))
    n = len(obs)
    data = dict(observations=np.array(obs, f32), actions=np.array(act, f32), next_observations=np.array(nobs, f32),
                rewards=np.concatenate(rew).astype(f32), terminals=np.zeros(n, bool), rtgs=np.concatenate(rtg).astype(f32).reshape(n, 1))
    return data, np.asarray(rets)


def pm_return(select_action, goal, episodes=10, seed=1000):
    """mean return of ``select_action(obs [1, 2], rtg tensor [1, 1])`` conditioned on ``goal``, the rtg dropping by every reward"""
    env = PointMassEnv(seed)
    out = []
    for _ in range(episodes):
        o, done, ret = env.reset(), False, 0.0
        rtg = torch.tensor([[goal]]).type(torch.float32)
        while not done:
            o, r, done, _ = env.step(np.asarray(select_action(o.reshape(1, -1), rtg)).flatten())
            ret += r
            rtg = rtg - r
        out.append(ret)
    return float(np.mean(out))
