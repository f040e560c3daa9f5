"""Deterministic duck-typed policy / dynamics / env used to pin MBPolicyTrainer semantics (by the golden generator that drives the real
reference trainer and by the tests that drive ours), and the termination-function inputs of the termination fixture."""
import os

import numpy as np
import torch

OBS, ACT, N_DATA, BATCH, EPOCHS, STEPS, EVAL_EPS, SEED = 4, 2, 300, 20, 3, 7, 3, 5
ROLLOUT = (3, 10, 4)             # rollout_freq (not a divisor of STEPS), rollout_batch_size, rollout_length
FAKE_CAP = 50                     # model buffer capacity: the rollouts wrap around it
REAL_RATIO = 0.25
TERM_DIM = 27                     # pen reads column 26


def dataset():
    rng = np.random.RandomState(2)
    return dict(observations=rng.standard_normal((N_DATA, OBS)).astype(np.float32),
                actions=rng.standard_normal((N_DATA, ACT)).astype(np.float32),
                next_observations=rng.standard_normal((N_DATA, OBS)).astype(np.float32),
                rewards=rng.standard_normal(N_DATA).astype(np.float32),
                terminals=(rng.uniform(size=N_DATA) < 0.1))


def term_inputs():
    """(obs, act, next_obs) rows for every termination family: random rows, every threshold of columns 0 / 1 / 26 with its
    neighbours, +-100 in other columns, NaN and +-inf in each of those columns"""
    rng = np.random.RandomState(3)
    rows = [rng.uniform(-1.5, 1.5, (64, TERM_DIM)), rng.uniform(0.0, 2.5, (64, TERM_DIM))]
    base = np.full(TERM_DIM, 0.5)
    for col in (0, 1, 5, 26):
        for v in (-100.0, 100.0, -1.0, 1.0, 0.7, 0.2, -0.2, 0.8, 2.0, 1.0, 0.075, 0.0, np.nan, np.inf, -np.inf):
            for d in (0.0, np.spacing(np.float32(v)) if np.isfinite(v) else 0.0):
                for sgn in (1.0, -1.0):
                    r = base.copy()
                    r[col] = v + sgn * d
                    rows.append(r[None])
    next_obs = np.concatenate(rows).astype(np.float32)
    obs = rng.standard_normal(next_obs.shape).astype(np.float32)
    act = rng.standard_normal((len(obs), 3)).astype(np.float32)
    return obs, act, next_obs


TERM_FNS = ("halfcheetah", "hopper", "halfcheetahveljump", "antangle", "ant", "walker2d", "point2denv", "point2dwallenv", "pendulum",
            "humanoid", "pen", "default")
TASKS = ("halfcheetah-medium-v2", "halfcheetahvel", "halfcheetahvel-jump", "hopper-medium-replay-v2", "antangle", "ant-medium-v2",
         "antmaze-umaze-v0", "walker2d-expert-v2", "point2denv", "point2dwallenv", "pendulum", "humanoid", "pen-human-v1",
         "door-human-v1", "maze2d-umaze-v1", "pointmaze")


class FakeDynamics:
    def __init__(self):
        self.saved = []

    def save(self, path):
        self.saved.append(os.path.basename(os.path.normpath(path)))
        torch.save({"w": torch.ones(2)}, os.path.join(path, "dynamics.pth"))


class FakePolicy(torch.nn.Module):
    """rollout / learn are deterministic functions of their inputs, so the logged means and the recorded sums pin every draw"""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(3))
        self.dynamics = FakeDynamics()
        self.init_sums, self.real_sums, self.fake_sums, self.rollouts = [], [], [], 0
        self.mode = None

    def train(self):
        self.mode = "train"

    def eval(self):
        self.mode = "eval"

    def select_action(self, obs, deterministic=False):
        assert deterministic and obs.shape == (1, OBS) and self.mode == "eval"
        return np.full((1, ACT), 0.25, dtype=np.float32)

    def rollout(self, init_obss, rollout_length):
        assert self.mode == "train" and isinstance(init_obss, np.ndarray)
        self.init_sums.append(float(init_obss.astype(np.float64).sum()))
        self.rollouts += 1
        out = {k: [] for k in ("obss", "next_obss", "actions", "rewards", "terminals")}
        obs = init_obss
        n = 0
        rews = []
        for t in range(rollout_length):
            nxt = (obs * 0.9 + 0.1 * (t + 1)).astype(np.float32)
            act = np.repeat(obs[:, :1], ACT, axis=1).astype(np.float32) * 0.5
            rew = (obs.sum(1, keepdims=True) * 0.1).astype(np.float32)
            term = nxt[:, :1] > 0.6
            for k, v in zip(out, (obs, nxt, act, rew, term)):
                out[k].append(v)
            n += len(obs)
            rews.append(rew.ravel())
            if (~term).sum() == 0:
                break
            obs = nxt[~term.ravel()]
        return {k: np.concatenate(v) for k, v in out.items()}, {"num_transitions": n, "reward_mean": np.concatenate(rews).mean()}

    def learn(self, batch):
        assert self.mode == "train" and set(batch) == {"real", "fake"}
        ro = float(torch.as_tensor(batch["real"]["observations"]).double().sum())
        fo = float(torch.as_tensor(batch["fake"]["observations"]).double().sum())
        fr = float(torch.as_tensor(batch["fake"]["rewards"]).double().sum())
        self.real_sums.append(ro)
        self.fake_sums.append(fo)
        return {"loss/actor": ro + fo, "loss/critic": fr * 0.5, "alpha": 0.125}


class FakeEnv:
    def __init__(self):
        self.t = 0
        self.ep = 0

    def reset(self):
        self.t = 0
        return np.full(OBS, 0.1 * self.ep, dtype=np.float32)

    def step(self, action):
        self.t += 1
        done = self.t >= 3 + (self.ep % 2)
        if done:
            self.ep += 1
        return np.full(OBS, 0.01 * self.t, dtype=np.float32), 1.0 + 0.5 * float(action.sum()), done, {}

    def get_normalized_score(self, x):
        return x / 10.0


class FakeScheduler:
    def __init__(self):
        self.n = 0

    def step(self):
        self.n += 1
