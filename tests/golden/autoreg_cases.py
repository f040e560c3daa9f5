"""Synthetic inputs of the autoregressive-policy fixtures, shared by make_autoreg_golden.py (which feeds them to the real reference) and by
the tests (numpy oracle, HIP engine); and the fake collaborators that pin ``rollout``.  Pure numpy; no reference code.

The net is ``AutoregressivePolicy.model``: keys model.{0, 2, ..., 2L}.{weight, bias}, Linear(obs_dim + 2 act_dim, h0) ... Linear(h, 2), a
LeakyReLU behind every Linear, the last one included.  With nn.Linear's default init every tail pre-activation of a small case can land on
one side of zero, which would leave one branch of the output LeakyReLU untested; so the output layer is drawn on a seed of its own
(RandomState(case seed + 1000 run + 500 + offset)) with its weights at twice the default magnitude and a spread bias (+0.1, -0.1), and
the offset is chosen so that IN THE REFERENCE, at every one of the 4 steps, each of the two output columns has at least 10 % of its
pre-activations on each side of zero and none within 1e-3 of max |z_tail| of zero (10x the 1e-4 bar of the taps): no test hinges on which
side a value falls.  make_autoreg_golden.py asserts it (and finds such offsets: --search).  Among the 2048 to 6144 tail values of the three
larger cases no offset of 400 kept that margin with independent Gaussian rows, so their rows are structured: ar_act32 ("bit": g) carries
a sign bit in observation column 0 (+-1) whose first-layer weights are scaled by g, so the tail values sit in two groups away from zero;
the rows of ar_ws and ar_hopper ("proto": P) are P prototypes per batch, each repeated with an N(0, 1e-3^2) perturbation (all rows
distinct), so the tail values sit in P x act_dim narrow groups.  Through ar_hopper's four layers of 200 the tail varies less over
the rows (std 0.01) than the hidden biases offset it, so its hidden weights are scaled by "hgain" = sqrt(6) (variance-preserving for
U(+-1/sqrt(fan_in)) weights behind a rectifier) and its output bias ("center") is minus the median of the tail over the first batch.
Even so, at the launcher's lr of 1e-3 the first Adam steps (every weight moves by lr, coherently over 200 units) shift the whole tail
by more than it varies over the rows: in the reference the logstd column is one-sided from the second or third step on, for every
offset of 400 and hidden gains up to 4.  The generator therefore asserts the sign conditions of ar_hopper at step 0 only ("sign_steps")
and prints the later steps; the five smaller cases, whose parameters and gradients the tests compare in full, meet them at every step.  Runs > 0 of a case (many-runs tests against
the oracle alone) use the same offset without that guarantee."""
from collections import OrderedDict

import numpy as np

import synth

f32 = np.float32
STEPS = 4
CASES = {
    # input width 9
    "ar_tiny": dict(obs_dim=5, act_dim=2, hidden=[32, 32], B=16, lr=3e-4, seed=81, full=True, offset=25),
    # input width 13, three unequal layers
    "ar_odd": dict(obs_dim=7, act_dim=3, hidden=[48, 32, 40], B=24, lr=3e-4, seed=82, full=True, offset=246),
    # no earlier dimension, one hidden layer
    "ar_one": dict(obs_dim=4, act_dim=1, hidden=[16], B=8, lr=3e-4, seed=83, full=True, offset=15),
    # the act_dim ceiling: 256 expanded rows
    "ar_act32": dict(obs_dim=6, act_dim=32, hidden=[32], B=8, lr=3e-4, seed=84, full=True, offset=33, bit=12.0),
    # the widths and row counts at which the ReLU-only few-rows and weight-stationary launches would otherwise be picked (256 expanded
    # rows; 16 runs of it are 4096 batched rows).  Digests and the step-0 gradient (full parameters would not fit a fixture file)
    "ar_ws": dict(obs_dim=6, act_dim=4, hidden=[256, 256], B=64, lr=3e-4, seed=85, full=False, grads=True, offset=387, proto=8),
    # run_regress.py's shape on hopper; digests only
    "ar_hopper": dict(obs_dim=11, act_dim=3, hidden=[200] * 4, B=256, lr=1e-3, seed=86, full=False, offset=3, proto=8, center=True, hgain=6.0 ** 0.5, sign_steps=1),
}
SAMPLE_CASES = ("ar_tiny", "ar_odd", "ar_act32")
SAMPLE_ROWS, SAMPLE_SEED0 = 8, 4000


def make_net(c, run=0, offset=None):
    rng = np.random.RandomState(c["seed"] + 1000 * run)
    net, d = synth.make_backbone(rng, c["obs_dim"] + 2 * c["act_dim"], list(c["hidden"]), prefix="model.")
    if c.get("bit"):
        net["model.0.weight"][:, 0] *= f32(c["bit"])
    if c.get("hgain"):
        for i in range(len(c["hidden"])):
            net[f"model.{2 * i}.weight"] *= f32(c["hgain"])
    off = c.get("offset", 0) if offset is None else offset
    hr = np.random.RandomState(c["seed"] + 1000 * run + 500 + off)
    k = 2.0 / np.sqrt(d)
    n = 2 * len(c["hidden"])
    net[f"model.{n}.weight"] = hr.uniform(-k, k, (2, d)).astype(f32)
    net[f"model.{n}.bias"] = np.array([0.1, -0.1], f32)
    return net, rng


def make_rows(rng, n, c):
    """rtgs ride along (the policy accepts and ignores them)"""
    rows = OrderedDict(observations=rng.standard_normal((n, c["obs_dim"])).astype(f32),
                       actions=np.tanh(rng.standard_normal((n, c["act_dim"]))).astype(f32),
                       rtgs=rng.uniform(0.0, 100.0, size=(n, 1)).astype(f32))
    if c.get("proto"):
        i = np.arange(n) % c["proto"]
        for k in ("observations", "actions"):
            rows[k] = (rows[k][:c["proto"]][i] + f32(1e-3) * rng.standard_normal(rows[k].shape)).astype(f32)
    if c.get("bit"):
        rows["observations"][:, 0] = np.where(rows["observations"][:, 0] > 0, f32(1), f32(-1))
    return rows


def case_inputs(case, run=0, offset=None):
    """(case dict, initial net, STEPS batches); ``run`` > 0: other weights and batches of the same shape (many-runs tests)"""
    c = CASES[case]
    net, rng = make_net(c, run, offset)
    batches = [make_rows(rng, c["B"], c) for _ in range(STEPS)]
    if c.get("center"):
        net[f"model.{2 * len(c['hidden'])}.bias"] -= np.median(_tail(net, c, batches[0]), axis=0).astype(f32)
    return c, net, batches


def _tail(net, c, b):
    """tail pre-activations of the expanded rows of batch ``b`` (a plain numpy forward)"""
    B, A = b["actions"].shape
    eye = np.eye(A, dtype=f32)
    mask = np.tril(np.ones((A, A), f32)) - eye
    h = np.concatenate([np.tile(b["observations"], (A, 1)), np.tile(b["actions"], (A, 1)) * np.repeat(mask, B, axis=0), np.repeat(eye, B, axis=0)], axis=1)
    n = len(c["hidden"])
    for i in range(n + 1):
        h = h @ net[f"model.{2 * i}.weight"].T + net[f"model.{2 * i}.bias"]
        if i < n:
            h = np.where(h > 0, h, f32(0.01) * h)
    return h


def epoch_inputs(n_runs=3, n_epochs=2):
    """the ordered-epoch test: a dataset of N = 3 B + 5 rows of ar_tiny's shape (4 steps, the last holding 5 valid rows) and, per epoch,
    one row order [n_runs, 4 B]: a permutation of [0, N) per run, padded with -1"""
    c = CASES["ar_tiny"]
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


def sample_obs(case):
    c = CASES[case]
    return np.random.RandomState(c["seed"] + 77).standard_normal((SAMPLE_ROWS, c["obs_dim"])).astype(f32)


# ---- rollout fakes -------------------------------------------------------------------------------------------------------------------------
R_OBS, R_ACT, R_N = 3, 2, 12
ROLLOUTS = OrderedDict([      # name -> (trajectories, horizon, steps a trajectory of index i survives, rollout policy with sample_init_noise)
    ("thinning_noise", (R_N, 6, lambda i: 1 + (i * 5) % 7, True)),
    ("thinning_plain", (R_N, 6, lambda i: 1 + (i * 5) % 7, False)),
    ("all_end_early", (7, 9, lambda i: 1 + i % 3, True)),
    ("none_ends", (5, 4, lambda i: 99, False)),
])


def rollout_init(name):
    n = ROLLOUTS[name][0]
    o = np.random.RandomState(31).standard_normal((n, R_OBS)).astype(f32)
    o[:, 0] = np.arange(n)                     # column 0 carries the trajectory's index, column 1 its age: the fake dynamics read both
    o[:, 1] = 0
    return o


class FakeDynamics:
    """a deterministic numpy ``step``: trajectory i (obs column 0) ends at the age ``life(i)``"""

    def __init__(self, life):
        self.life = life

    def step(self, obs, act):
        obs, act = np.asarray(obs, f32), np.asarray(act, f32)
        nxt = obs.copy()
        nxt[:, 1] += 1
        nxt[:, 2] = (0.5 * obs[:, 2] + 0.25 * act.sum(axis=1)).astype(f32)
        rew = (0.1 * obs[:, 0] + 0.01 * obs[:, 1] + act[:, 0] - 0.5 * act[:, 1]).astype(f32).reshape(-1, 1)
        term = np.array([nxt[i, 1] >= self.life(int(obs[i, 0])) for i in range(len(obs))], bool).reshape(-1, 1)
        return nxt, rew, term, {}


class NoisePolicy:
    """the diffusion interface: per-trajectory frozen noise, handed back (thinned by the survivor mask) as the second argument"""

    def sample_init_noise(self, n):
        return (np.arange(n, dtype=f32) * f32(0.125)).reshape(n, 1)

    def select_action(self, obs, noise):
        assert noise is not None and len(noise) == len(obs)
        obs = np.asarray(obs, f32)
        return np.concatenate([np.sin(obs[:, :1] + obs[:, 1:2]) + noise, np.cos(obs[:, 2:3]) - noise], axis=1).astype(f32)


class PlainPolicy:
    """no ``sample_init_noise`` (AutoregressivePolicy's interface): the second argument is None"""

    def select_action(self, obs, rtg=None):
        assert rtg is None
        obs = np.asarray(obs, f32)
        return np.concatenate([np.sin(obs[:, :1] + obs[:, 1:2]), np.cos(obs[:, 2:3])], axis=1).astype(f32)


def rollout_collaborators(name):
    n, horizon, life, noisy = ROLLOUTS[name]
    return FakeDynamics(life), (NoisePolicy() if noisy else PlainPolicy()), rollout_init(name), horizon


# ---- end-to-end task: correlated action dimensions -------------------------------------------------------------------------------------
# obs = noise (2 columns), a0 ~ N(0, 1), a1 = -a0 + 0.1 N(0, 1): corr(a0, a1) = -0.995.  A head with one Gaussian per dimension given the
# observation alone cannot represent it (its samples have correlation ~ 0); the autoregressive one conditions a1 on the sampled a0.
C_OD, C_AD, C_N, C_HID, C_BATCH, C_LR = 2, 2, 8192, [64, 64], 256, 1e-3


def corr_dataset(seed=0):
    rng = np.random.RandomState(seed)
    obs = rng.standard_normal((C_N, C_OD)).astype(f32)
    a0 = rng.standard_normal(C_N)
    act = np.stack([a0, -a0 + 0.1 * rng.standard_normal(C_N)], axis=1).astype(f32)
    return dict(observations=obs, actions=act, next_observations=obs, rewards=np.zeros(C_N, f32), terminals=np.zeros(C_N, bool),
                rtgs=np.zeros((C_N, 1), f32))
