"""CPU: the pieces of RAMBO's device model update that need no GPU -- the numpy restatement of the advantage against the reference's
fixture (tests/golden/rambo_adv_tiny.npz, make_rambo_adv_golden.py), the segment schedule against a literal count of the reference's
loop, the header, ``update_dynamics_device``'s refusals and the trainer's chunk schedule with model updates."""
import os

import numpy as np
import pytest
import torch

import mb_trainer_fakes as fk
import rambo_adv_refs as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("all_loss", "sl_loss", "adv_loss", "adv_advantage", "adv_log_prob")


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(np.asarray(b, np.float64)).max())


@pytest.mark.parametrize("ent", [0, 1])
@pytest.mark.parametrize("step", [0, 1])
def test_numpy_advantage_vs_fixture(ent, step):
    """float64 against the reference's fp32 tensors: two 16-wide layers and a handful of fp32 roundings per element leave about 1e-6
    of the largest entry; held to 1e-5.  The normalised advantage divides by the spread of raw, which multiplies the relative error by
    max|raw| / std (printed), so it is held to 1e-5 of that.  The terminals are comparisons of the same fp32 rows: equal."""
    g = ar.fixture()
    t = f"ent{ent}/step{step}/"
    out = ar.advantage(g[t + "obs"], g[t + "act"], g[t + "next_obs"], g[t + "reward"], ar.net_params(g, "actor"),
                       ar.net_params(g, "critic1"), ar.net_params(g, "critic2"), float(g["gamma"]), float(g["alpha"]), bool(ent))
    assert np.array_equal(out["term"], g[t + "terminals"])
    frac = g[t + "terminals"].mean()
    assert 0.25 <= frac <= 0.75, frac
    for mine, ref in (("logp_next", "logp_next"), ("q_next", "next_q"), ("value", "value"), ("q_base", "value_baseline"), ("raw", "raw")):
        err = _rel(out[mine], g[t + ref])
        print(mine, "err / max", err)
        assert err <= 1e-5, (mine, err)
    amp = np.abs(g[t + "raw"]).max() / g[t + "raw"].astype(np.float64).std(ddof=1)
    err = _rel(out["norm"], g[t + "advantage"])
    print("norm err / max", err, "amplification", amp)
    assert err <= 1e-5 * max(amp, 1.0), err
    # the logged adv_advantage is the mean of the normalised advantage: zero up to fp32 rounding
    assert abs(g[t + "losses"][3]) <= 1e-6
    # the fixture's own normalisation, from its own raw, in float64
    assert _rel(ar.normalise(g[t + "raw"]), g[t + "advantage"]) <= 1e-5
    if ent:      # the entropy term is in: next_q differs from the other trajectory's at the same rows
        assert not np.array_equal(g[t + "next_q"], g[t.replace("ent1", "ent0") + "next_q"]) or step > 0


def _reference_loop_steps(adv_train_steps, rollout_length):
    """rambo.py:101-125, counted literally: -> (segments entered, steps of each)"""
    steps, segs = 0, []
    while steps < adv_train_steps:
        segs.append(0)
        for t in range(rollout_length):
            segs[-1] += 1
            steps += 1
            if steps == 1000:
                break
    return segs


@pytest.mark.parametrize("steps,length", [(1000, 5), (24, 3), (1, 5), (1003, 5), (2000, 7)])
def test_schedule_is_the_reference_loop(steps, length):
    from offlinerlkit.policy import rambo_adv_schedule
    got = rambo_adv_schedule(steps, length)
    assert got == _reference_loop_steps(steps, length)
    assert all(1 <= n <= length for n in got) and sum(got) >= steps
    if (steps, length) == (2000, 7):      # the quirk: the literal 1000 cuts segment 143 short, the loop goes on to 2001 steps
        assert got[142] == 6 and sum(got) == 2001 and len(got) == 286
    if (steps, length) == (1, 5):         # the for loop is not left when adv_train_steps is reached
        assert got == [5]
    assert rambo_adv_schedule(steps, length) == got      # pure


def test_header_declares_the_entries_and_the_struct():
    from offlinerlkit import _engine
    header = open(os.path.join(ROOT, "include", "orl_engine.h")).read()
    for sym in ("orl_engine_adv_advantage", "orl_rambo_update_dynamics"):
        assert f"int {sym}(" in header and sym in _engine.ABI_SYMBOLS and hasattr(_engine.load_library(), sym), sym
    assert "typedef struct orl_rambo_loop {" in header and "} orl_rambo_loop;" in header
    body = header[header.index("typedef struct orl_rambo_loop {"):header.index("} orl_rambo_loop;")]
    for field in ("int32_t rows;", "int32_t term_kind;", "int32_t include_ent;", "int32_t n_segments;", "const int32_t* segment_steps;"):
        assert field in body, field
    assert [f[0] for f in _engine.OrlRamboLoop._fields_] == ["rows", "term_kind", "include_ent", "n_segments", "segment_steps"]
    assert _engine.RAMBO_KEYS == KEYS
    for m in ("adv_advantage", "rambo_update_dynamics"):
        assert callable(getattr(_engine.Engine, m))


class _FakeDyn:
    _n_runs = 1
    term_kind = 2

    def __init__(self):
        self.model = torch.nn.Linear(1, 1)


class _HostBuffer:
    def sample(self, n):
        raise AssertionError("not reached")


class _DevBuffer(_HostBuffer):
    def device_buffer(self):
        raise AssertionError("not reached")


def _policy(dynamics, **kw):
    from offlinerlkit.modules import ActorProb, Critic, TanhDiagGaussian
    from offlinerlkit.nets import MLP
    from offlinerlkit.policy import RAMBOPolicy
    od, ad, hid = 3, 2, [16, 16]
    actor = ActorProb(MLP(od, hid), TanhDiagGaussian(hid[-1], ad, unbounded=True, conditioned_sigma=True), "cpu")
    c1, c2 = Critic(MLP(od + ad, hid), "cpu"), Critic(MLP(od + ad, hid), "cpu")
    dummy = torch.nn.Parameter(torch.zeros(1))
    return RAMBOPolicy(dynamics, actor, c1, c2, torch.optim.Adam(actor.parameters(), lr=1e-4), torch.optim.Adam(c1.parameters(), lr=3e-4),
                       torch.optim.Adam(c2.parameters(), lr=3e-4), torch.optim.Adam([dummy], lr=3e-4), **kw)


def test_update_dynamics_device_refusals():
    """each refusal comes before the engine is bound or anything is sampled (the fakes raise if they are touched)"""
    d = _FakeDyn()
    d._n_runs = 2
    with pytest.raises(NotImplementedError, match="n_runs"):
        _policy(d).update_dynamics_device(_DevBuffer())
    p = _policy(_FakeDyn())
    p._n_runs = 2
    with pytest.raises(NotImplementedError, match="n_runs"):
        p.update_dynamics_device(_DevBuffer())
    d = _FakeDyn()
    d.term_kind = None
    with pytest.raises(NotImplementedError, match="term_kind") as e:
        _policy(d).update_dynamics_device(_DevBuffer())
    # rollout_device's wording
    from offlinerlkit.policy import MOPOPolicy
    with pytest.raises(NotImplementedError) as e2:
        MOPOPolicy.rollout_device(_policy(d), _DevBuffer(), _DevBuffer(), 4, 2)
    assert str(e.value) == str(e2.value)
    with pytest.raises(NotImplementedError, match="device_buffer"):
        _policy(_FakeDyn()).update_dynamics_device(_HostBuffer())
    assert _policy(_FakeDyn())._eng is None


class _Ring:
    def reserve_device(self):
        return self


class _Logger:
    def __init__(self):
        self.mean, self.kv = [], {}

    def logkv_mean(self, k, v):
        self.mean.append((k, v))

    def logkv(self, k, v):
        self.kv[k] = v

    def log(self, s):
        pass


class _FusedPolicy(fk.FakePolicy):
    def __init__(self):
        super().__init__()
        self.events, self.t = [], 0
        self.dynamics.term_kind = 1

    def rollout_device(self, real, fake, n, length):
        self.events.append(("R", self.t))
        return {"num_transitions": n * length, "reward_mean": 0.5}

    def learn_n(self, steps, real, fake, batch, ratio):
        self.events += [("s", self.t + i) for i in range(steps)]
        self.t += steps
        return {"loss/actor": float(steps)}


class _RamboLike(_FusedPolicy):
    def update_dynamics_device(self, real):
        self.events.append(("U", self.t - 1))
        return {"adv_dynamics_update/" + k: float(self.t) for k in KEYS}


def _trainer(policy, logger, steps, rollout, **kw):
    from offlinerlkit.policy_trainer import MBPolicyTrainer
    return MBPolicyTrainer(policy, fk.FakeEnv(), object(), _Ring(), logger, rollout, epoch=1, step_per_epoch=steps, batch_size=fk.BATCH,
                           real_ratio=fk.REAL_RATIO, eval_episodes=1, **kw)


def test_fused_trainer_accepts_the_device_update_and_refuses_without():
    with pytest.raises(ValueError, match="dynamics_update_freq"):
        _trainer(_FusedPolicy(), None, 200, (100, 10, 4), fused=True, dynamics_update_freq=40)
    _trainer(_FusedPolicy(), None, 200, (100, 10, 4), fused=True)
    pol, log = _RamboLike(), _Logger()
    tr = _trainer(pol, log, 200, (100, 10, 4), fused=True, dynamics_update_freq=40)
    assert tr._train_mb_epoch_fused(1, 0) == 200
    # the reference loop (mb_policy_trainer.py:66-102), event by event
    want = []
    for t in range(200):
        if t % 100 == 0:
            want.append(("R", t))
        want.append(("s", t))
        if (t + 1) % 40 == 0:
            want.append(("U", t))
    assert pol.events == want
    ups = [(k, v) for k, v in log.mean if k.startswith("adv_dynamics_update/")]
    assert len(ups) == 5 * 5 and {k for k, _ in ups} == {"adv_dynamics_update/" + k for k in KEYS}
    assert log.kv["loss/actor"] == pytest.approx(sum(n * n for n in (40, 40, 20, 20, 40, 40)) / 200)


def test_chunk_schedule_with_model_updates():
    from offlinerlkit.policy_trainer import fused_mb_dyn_schedule, fused_mb_schedule
    assert fused_mb_dyn_schedule(0, 200, 100, 40) == [(True, 40, True), (False, 40, True), (False, 20, False), (True, 20, True),
                                                      (False, 40, True), (False, 40, True)]
    # an epoch that starts off the grid, and the launcher's 1000 / 1000
    assert fused_mb_dyn_schedule(950, 100, 100, 1000) == [(False, 50, True), (True, 50, False)]
    assert fused_mb_dyn_schedule(0, 1000, 1000, 1000) == [(True, 1000, True)]
    # without updates: the present schedule, and fused_mb_schedule's own results are what they were
    for t0, n, rf in ((0, 7, 3), (7, 7, 3), (5, 250, 1000), (0, 1000, 1)):
        assert fused_mb_dyn_schedule(t0, n, rf) == [(r, s, False) for r, s in fused_mb_schedule(t0, n, rf)]
    assert fused_mb_schedule(0, 7, 3) == [(True, 3), (True, 3), (True, 1)] and fused_mb_schedule(7, 7, 3) == [(False, 2), (True, 3), (True, 2)]
    for chunks in (fused_mb_dyn_schedule(3, 500, 7, 11), fused_mb_dyn_schedule(0, 64, 1000, 1)):
        assert all(n > 0 for _, n, _ in chunks) and sum(n for _, n, _ in chunks) in (500, 64)
