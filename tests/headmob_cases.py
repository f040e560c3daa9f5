"""Cases of tests/test_gpu_headmob_kernels.py (k_rcsl_loss, k_rcslg_head, k_autoreg_head / k_autoreg_draw, k_mobile_assemble /
k_lcb_penalty / k_mobile_td_loss and the dynamic-scale kernels held to the float64 restatements of tests/row_refs.py) -- shapes and
value edges only, host arrays only: tests/test_headmob_refs_cpu.py runs the fp32 numpy oracles on the same inputs and requires them
inside the restatements' bounds, which is the condition that the inputs are fair.

One edge moves at a time from each family's base case; every case is a keyword set of ``inputs``."""
from collections import OrderedDict

import numpy as np

import synth

f32 = np.float32


def _next(x, to):
    return float(np.nextafter(f32(x), f32(to)))


def case_id(d):
    return "-".join(f"{k}{v.__name__ if callable(v) else v}" for k, v in d.items()) or "base"


class Ctx:
    pass


# ---------------------------------------------------------------------------------------------------------------------------------
# padding patterns of one ordered-epoch step: which of the B batch rows are valid
# ---------------------------------------------------------------------------------------------------------------------------------
def valid_rows(pad, B):
    v = np.ones(B, bool)
    if pad == "one_valid":                # 1 valid row of B, and not the first one
        v[:] = False
        v[B // 2] = True
    elif pad == "one_pad":                # B - 1 valid rows; the padding row sits inside the first 64-row chunk
        v[min(5, B - 1)] = False
    elif pad == "interleaved":            # padding between valid rows, not trailing
        v[1::3] = False
    elif pad == "last_chunk_only":        # the only valid row is the last one (the last 64-row chunk of k_rcslg_head)
        v[:] = False
        v[B - 1] = True
    elif pad is not None:
        raise ValueError(pad)
    return v


# ---------------------------------------------------------------------------------------------------------------------------------
# the supervised families: "rcsl", "rcslg", "autoreg".  One net per run, rows (observations, actions, rtgs), a validity mask
# ---------------------------------------------------------------------------------------------------------------------------------
def _sup_net(family, rng, od, A, hidden):
    if family == "autoreg":
        net, d = synth.make_backbone(rng, od + 2 * A, list(hidden), prefix="model.")
        k = 2.0 / np.sqrt(d)              # twice nn.Linear's magnitude and a spread bias: both branches of the output LeakyReLU are taken
        net[f"model.{2 * len(hidden)}.weight"] = rng.uniform(-k, k, (2, d)).astype(f32)
        net[f"model.{2 * len(hidden)}.bias"] = np.array([0.1, -0.1], f32)
        return net
    net, _ = synth.make_backbone(rng, od + 1, list(hidden) + [A])
    if family == "rcslg":                 # DiagGaussian's two A x A heads; the sigma bias spread beyond both clamps
        k = 1.0 / np.sqrt(A)
        net["dist_net.mu.weight"] = rng.uniform(-k, k, (A, A)).astype(f32)
        net["dist_net.mu.bias"] = rng.uniform(-k, k, A).astype(f32)
        net["dist_net.sigma.weight"] = rng.uniform(-k, k, (A, A)).astype(f32)
        net["dist_net.sigma.bias"] = np.linspace(-5.5, 2.5, A).astype(f32) if A > 1 else np.array([-1.0], f32)
    return net


def inputs(family, B=None, A=None, od=5, R=1, hidden=(32, 32), seed=0, pad=None, mutate=None, precision=0, **over):
    """nets and rows of every run of a supervised case.  ``rows``: what the dataset holds; ``batches``: what a step sees -- a padding row
    reads dataset row 0, as the engine's gather does"""
    c = Ctx()
    base = SUP_BASE[family]
    c.family, c.B, c.A, c.od, c.R, c.hidden, c.pad, c.precision = family, B or base["B"], A or base["A"], od, R, list(hidden), pad, precision
    c.over = over
    c.nets, c.rows, c.batches, c.valid, c.order = [], [], [], [], []
    for r in range(R):
        rng = np.random.RandomState(7919 * seed + 31 * r + c.B + 64 * c.A + SUP_BASE[family]["salt"])
        c.nets.append(_sup_net(family, rng, od, c.A, c.hidden))
        c.rows.append(OrderedDict(observations=rng.standard_normal((c.B, od)).astype(f32),
                                  actions=np.tanh(rng.standard_normal((c.B, c.A))).astype(f32),
                                  rtgs=rng.uniform(0.0, 10.0, size=(c.B, 1)).astype(f32)))
    if mutate:
        mutate(c)
    for r in range(R):
        v = valid_rows(pad, c.B)
        if pad == "interleaved" and r % 2:            # the runs of a padded case do not share their pattern
            v = np.roll(v, 1)
        o = np.where(v, np.arange(c.B), -1).astype(np.int64)
        c.valid.append(v)
        c.order.append(o)
        c.batches.append(OrderedDict((k, a[np.where(o < 0, 0, o)]) for k, a in c.rows[r].items()))
    return c


SUP_BASE = {"rcsl": dict(B=32, A=3, salt=1), "rcslg": dict(B=32, A=3, salt=2), "autoreg": dict(B=16, A=2, salt=3)}
PADS = [dict(pad="one_valid"), dict(pad="one_pad"), dict(pad="interleaved")]

# k_rcsl_loss: B A = 255 / 258 (the second trip of the 256-thread loop begins inside a row), B = 257 (second trip of the row count)
RCSL_SHAPES = [dict(), dict(B=1), dict(B=85), dict(B=86), dict(B=257), dict(A=1), dict(A=32), dict(R=3)] + PADS + [dict(precision=1), dict(precision=2)]

# k_rcslg_head: A 1 / 5 / 17 / 31 / 32 -> 2 / 60 / 612 / 1984 / 2112 head gradients = 1, 1, 3, 8, 9 per thread; B around the 64-row chunk;
# at A = 32 full 2048-element chunks, two and three of them
RCSLG_SHAPES = ([dict(), dict(A=1), dict(A=5), dict(A=17), dict(A=31), dict(A=32), dict(B=1), dict(B=63), dict(B=64), dict(B=65), dict(B=129),
                 dict(A=32, B=65), dict(A=32, B=129), dict(R=3)] + PADS +
                [dict(B=129, pad="one_pad"), dict(B=129, pad="last_chunk_only"), dict(precision=1), dict(precision=2)])

LV_TABLE = [-5.0, _next(-5, -9), _next(-5, 9), 2.0, _next(2, -9), _next(2, 9), -20.0, 20.0, 0.0]      # column j: LV_TABLE[j % 9]


def constant_sigma_head(c):
    """W_sigma = 0: the raw log-variance of column j is LV_TABLE[j % 9] on every row -- on each clamp end, one ulp inside and outside each,
    far beyond both.  Columns 0 and 9 (log-variance exactly -5) carry a mean bias of +20 / -20, so that mu - a reaches +-20 where e^-s is
    largest"""
    for net in c.nets:
        net["dist_net.sigma.weight"][:] = 0
        net["dist_net.sigma.bias"][:] = [LV_TABLE[j % 9] for j in range(c.A)]
        net["dist_net.mu.bias"][0] = 20.0
        net["dist_net.mu.bias"][9] = -20.0


RCSLG_EDGES = [dict(B=64, A=17, mutate=constant_sigma_head)]

# k_autoreg_head: M = A B expanded rows; M = 258 at B = 86, A = 3 (m % B with the second trip starting inside a block of rows); B = 257, A = 1
AUTOREG_SHAPES = ([dict(), dict(A=1), dict(A=3), dict(A=32), dict(B=1), dict(B=8), dict(B=86, A=3), dict(B=257, A=1), dict(R=3)] + PADS +
                  [dict(B=86, A=3, pad="interleaved"), dict(precision=1), dict(precision=2)])


def constant_tail(b_mean, b_ls):
    """last-layer weights 0: every expanded row has the tail pre-activation (b_mean, b_ls)"""
    def f(c):
        for net in c.nets:
            n = 2 * len(c.hidden)
            net[f"model.{n}.weight"][:] = 0
            net[f"model.{n}.bias"][:] = [b_mean, b_ls]
    f.__name__ = f"tail({b_mean:g},{b_ls:g})"
    return f


# both outputs exactly 0 (the slope branch: 0.01 * 0); logstd -8 (pre-activation -800) and +8; targets 50 away from the mean
AUTOREG_EDGES = [dict(mutate=constant_tail(0.0, 0.0)), dict(mutate=constant_tail(0.3, -800.0)), dict(mutate=constant_tail(-0.3, 8.0)),
                 dict(mutate=constant_tail(-50.0, 0.5)), dict(mutate=constant_tail(5000.0, -100.0))]

# k_autoreg_draw: n rows per run
DRAW_SHAPES = [dict(n=8), dict(n=1), dict(n=255), dict(n=257), dict(n=8, A=1), dict(n=257, A=1), dict(n=8, A=32), dict(n=8, R=3)]


def draw_inputs(n=8, A=2, od=5, R=1, hidden=(32, 32)):
    c = inputs("autoreg", B=16, A=A, od=od, R=R, hidden=hidden, seed=3)
    c.n = n
    rng = np.random.RandomState(991 + n + 64 * A)
    c.sobs = rng.standard_normal((R, n, od)).astype(f32)
    c.seps = rng.standard_normal((R, n, A)).astype(f32)
    return c


# the seed of a backward pass that is all zero: its dynamic scale must be 1
def zero_seed_rcsl(c):
    for net, rows in zip(c.nets, c.rows):
        n = 2 * len(c.hidden)
        net[f"backbone.model.{n}.weight"][:] = 0
        net[f"backbone.model.{n}.bias"][:] = 0.25
        rows["actions"][:] = 0.25


def zero_seed_rcslg(c):
    for net in c.nets:
        net["dist_net.mu.weight"][:] = 0
        net["dist_net.sigma.weight"][:] = 0


# ---------------------------------------------------------------------------------------------------------------------------------
# MOBILE: base B = 16, S = 3, E = 3, real_rows = 4, obs_dim 5, act_dim 2, hidden [32, 32].  The next-state samples are plain N(0, 1)
# rows in orl_dynsample_next's order (s E + e) B + b: the penalty pass does not care where they come from
# ---------------------------------------------------------------------------------------------------------------------------------
MOBILE_BASE = dict(B=16, A=2, od=5, S=3, E=3, real_rows=4)


def mobile_inputs(B=16, A=2, od=5, S=3, E=3, real_rows=4, R=1, hidden=(32, 32), seed=0, mutate=None, precision=0, **over):
    c = Ctx()
    c.family, c.B, c.A, c.od, c.S, c.E, c.real_rows, c.R, c.hidden, c.precision = "mobile", B, A, od, S, E, real_rows, R, list(hidden), precision
    c.M = S * E * B
    c.over = over
    c.sts, c.batches, c.noises, c.samples = [], [], [], []
    for r in range(R):
        rng = np.random.RandomState(7919 * seed + 31 * r + B + 64 * A + 5)
        c.sts.append(synth._sac_like_state(rng, dict(obs_dim=od, act_dim=A, hidden=list(hidden))))
        c.batches.append(synth.make_batch(rng, B, od, A))
        c.noises.append(OrderedDict(eps_lcb=rng.standard_normal((c.M, A)).astype(f32), eps_next=rng.standard_normal((B, A)).astype(f32),
                                    eps_actor=rng.standard_normal((B, A)).astype(f32)))
        c.samples.append(rng.standard_normal((c.M, od)).astype(f32))
    if mutate:
        mutate(c)
    return c


def identical_elites(c):
    """every elite draws the same next state and the same action noise: the mean over S is the same for every elite, the penalty exactly 0"""
    for smp, n in zip(c.samples, c.noises):
        for a, w in ((smp, c.od), (n["eps_lcb"], c.A)):
            v = a.reshape(c.S, c.E, c.B, w)
            v[:] = v[:, :1]


def tied_targets(c):
    for st in c.sts:
        st["critic2_old"] = {k: v.copy() for k, v in st["critic1_old"].items()}


def batch_edge(kind):
    def f(c):
        for b in c.batches:
            if kind == "terminal":
                b["terminals"][:] = 1
            elif kind == "alive":
                b["terminals"][:] = 0
            elif kind == "reward-1e3":          # y < 0 on every row: the clamp leaves exactly 0
                b["rewards"][:] = -1e3
            else:
                b["rewards"][:] = 1e3
    f.__name__ = kind
    return f


def zero_seed_mobile(c):
    """constant critics at 0.5, all-terminal rows with reward 0.5: q == y on every row, dq all zero"""
    for st, b in zip(c.sts, c.batches):
        for k in ("critic1", "critic2"):
            st[k]["last.weight"][:] = 0
            st[k]["last.bias"][:] = 0.5
        b["terminals"][:] = 1
        b["rewards"][:] = 0.5


ZERO_SEED_MOBILE = dict(mutate=zero_seed_mobile, penalty_coef=0.0)
MOBILE_SHAPES = [
    dict(),
    dict(E=2), dict(E=64),                                       # the smallest ensemble the config admits; LCB_MAX_E
    dict(S=1), dict(S=5),
    dict(B=1, real_rows=0), dict(B=257, S=1, E=2),               # a second workgroup of k_lcb_penalty / k_mobile_assemble
    dict(real_rows=0), dict(real_rows=16),
    dict(od=1), dict(od=31),                                     # input pitches 4 / 32, critic-input pitches 4 / 36
    dict(B=255, S=1, E=2), dict(B=513, S=1, E=2),                # k_mobile_td_loss: one trip short of full, three trips
    dict(deterministic_backup=1), dict(auto_alpha=0, alpha=0.2), dict(auto_alpha=0, alpha=0.2, deterministic_backup=1),
    dict(penalty_coef=0.0), dict(penalty_coef=7.0),
    dict(R=3),
    dict(precision=1), dict(precision=2),
    dict(B=257, S=1, E=2, precision=1),                          # dhead's scale from a k_grad_scale launch (k_head_bwd on two workgroups)
]
MOBILE_EDGES = [dict(mutate=identical_elites), dict(mutate=batch_edge("terminal")), dict(mutate=batch_edge("alive")),
                dict(mutate=batch_edge("reward-1e3")), dict(mutate=batch_edge("reward+1e3")), dict(mutate=tied_targets)]
