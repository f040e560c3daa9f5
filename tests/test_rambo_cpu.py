"""CPU: RAMBO's host side.  The numpy restatement of the adversarial model update (tests/rambo_oracle.py) against the fixture from the
reference (tests/golden/rambo_tiny.npz, make_rambo_golden.py) at the tolerances of test_dynamics_cpu.py; RAMBOPolicy's import,
constructor and refusals; ``update_dynamics``' keys, draw order and step count against a fake dynamics; the new C-ABI entries."""
import os

import numpy as np
import pytest
import torch

import make_rambo_golden as mr
import rambo_oracle as ro

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROWS = ("obs", "act", "sl_obs", "sl_act", "sl_next_obs", "sl_rew")


def _g(name):
    return np.load(os.path.join(GOLD, name))


def _state(g, tag):
    keys = sorted({k[len(tag) + 1:-len("/full")] for k in g.files if k.startswith(tag + "/") and k.endswith("/full")})
    return {k: g[f"{tag}/{k}/full"].copy() for k in keys}


@pytest.mark.parametrize("traj,w", [("w1", 1.0), ("w0", 0.0)])
def test_oracle_vs_fixture(traj, w):
    g, c = _g("rambo_tiny.npz"), mr.TINY
    st = {k: v for k, v in _state(g, "init").items() if k != "elites"}
    opt = {}
    for t in range(c["steps"]):
        tag = f"{traj}/step{t}"
        rows = {k: g[f"{tag}/{k}"] for k in ROWS}
        f, m, gr = ro.step(st, opt, g["scaler_mu"], g["scaler_std"], rows, g[f"{tag}/eps"], g[f"{tag}/model_idx"], c["elite_idx"],
                           g[f"{tag}/advantage"], w, c["decays"], c["adv_lr"])
        assert np.abs(f["sample"][:, :-1] - g[f"{tag}/next_obs"]).max() <= 1e-5 * np.abs(g[f"{tag}/next_obs"]).max() + 1e-6
        assert np.abs(f["sample"][:, -1] - g[f"{tag}/reward"]).max() <= 1e-5 * np.abs(g[f"{tag}/reward"]).max() + 1e-6
        assert np.abs(m["log_prob"] - g[f"{tag}/log_prob"]).max() <= 2e-5 * np.abs(g[f"{tag}/log_prob"]).max()
        ref = dict(zip(mr.LOSS_KEYS, g[f"{tag}/losses"]))
        for k in ("all_loss", "sl_loss", "adv_loss", "adv_log_prob"):
            assert abs(m[k] - ref[k]) <= 2e-5 * abs(ref[k]) + 1e-7, (t, k, m[k], ref[k])
        refst = _state(g, tag)
        for k in st:
            assert np.abs(st[k] - refst[k]).max() <= 1e-5 + 1e-4 * np.abs(refst[k]).max(), (t, k)
        for k in ("max_logvar", "min_logvar"):
            assert np.allclose(gr[k], g[f"{tag}/grad_{k}"], rtol=1e-4, atol=1e-7), (t, k)
        if t == 0:
            full = ro.with_decay(_state(g, "init"), gr, c["decays"])      # the parameters the gradient was taken at
            for k in full:
                r = g[f"{tag}/grad/{k}"]
                assert np.abs(full[k] - r).max() <= 1e-4 * np.abs(r).max() + 1e-7, k


def test_fixture_non_elite_member_gets_no_adversarial_gradient():
    g, c = _g("rambo_tiny.npz"), mr.TINY
    ne = [k for k in range(c["K"]) if k not in c["elite_idx"]][0]
    for k in ("backbones.0.weight", "output_layer.weight", "output_layer.bias"):
        a, b = g[f"w1/step0/grad/{k}"], g[f"w0/step0/grad/{k}"]
        assert np.array_equal(a[ne], b[ne]) and np.abs(b[ne]).max() > 0, k
        assert not np.array_equal(a[c["elite_idx"][0]], b[c["elite_idx"][0]]), k


def _policy(n_runs=None, dynamics=None, **kw):
    from offlinerlkit.modules import ActorProb, Critic, TanhDiagGaussian
    from offlinerlkit.nets import MLP
    from offlinerlkit.policy import RAMBOPolicy
    od, ad, hid = 3, 2, [16, 16]
    actor = ActorProb(MLP(od, hid), TanhDiagGaussian(hid[-1], ad, unbounded=True, conditioned_sigma=True), "cpu")
    c1, c2 = Critic(MLP(od + ad, hid), "cpu"), Critic(MLP(od + ad, hid), "cpu")
    dummy = torch.nn.Parameter(torch.zeros(1))
    return RAMBOPolicy(dynamics, actor, c1, c2, torch.optim.Adam(actor.parameters(), lr=1e-4), torch.optim.Adam(c1.parameters(), lr=3e-4),
                       torch.optim.Adam(c2.parameters(), lr=3e-4), torch.optim.Adam([dummy], lr=3e-4), **kw)


def test_import_constructor_and_refusals():
    import inspect
    import offlinerlkit.policy as pol
    from offlinerlkit.policy import MOPOPolicy, RAMBOPolicy
    assert "RAMBOPolicy" in pol.__all__ and issubclass(RAMBOPolicy, MOPOPolicy)
    names = list(inspect.signature(RAMBOPolicy.__init__).parameters)
    assert names == ["self", "dynamics", "actor", "critic1", "critic2", "actor_optim", "critic1_optim", "critic2_optim", "dynamics_adv_optim",
                     "tau", "gamma", "alpha", "adv_weight", "adv_train_steps", "adv_rollout_batch_size", "adv_rollout_length",
                     "include_ent_in_adv", "scaler", "device"]
    p = _policy(adv_weight=3e-4, adv_train_steps=7)
    assert p._adv_weight == 3e-4 and p._adv_train_steps == 7 and p._adv_rollout_length == 5 and p.scaler is None
    for m in ("pretrain", "load", "update_dynamics", "dynamics_step_and_forward", "rollout", "select_action"):
        assert callable(getattr(p, m))
    with pytest.raises(NotImplementedError, match="n_runs"):
        p.set_engine_options(n_runs=2)
    p.set_engine_options(n_runs=1, seed=3)


class _FakeBuffer:
    def __init__(self):
        self.calls = []

    def sample(self, n):
        self.calls.append(n)
        k = float(len(self.calls))
        return {"observations": torch.full((n, 3), k), "actions": torch.zeros(n, 2), "next_observations": torch.zeros(n, 3),
                "rewards": torch.zeros(n, 1), "terminals": torch.zeros(n, 1)}


class _FakeDyn:
    _n_runs = 1

    def __init__(self):
        self.model = torch.nn.Linear(1, 1)


@pytest.mark.parametrize("steps,length,expect,n_roll", [(7, 3, 9, 3), (4, 5, 5, 1), (1003, 7, 1007, 144)])
def test_update_dynamics_keys_and_step_count(steps, length, expect, n_roll):
    """the while / for structure of rambo.py:108-125: whole rollouts until adv_train_steps is reached; the ``steps == 1000`` break
    ends only the rollout it falls in (rollout 143 of the last case stops after 6 of its 7 steps, and one more rollout follows)"""
    p = _policy(dynamics=_FakeDyn(), adv_train_steps=steps, adv_rollout_length=length, adv_rollout_batch_size=4)
    seen = []

    def fake(obs, act, so, sa, sn, sr):
        seen.append((float(np.asarray(obs)[0, 0]), float(so[0, 0])))
        return np.asarray(obs) + 100.0, np.zeros((len(obs), 1), bool), {"adv_dynamics_update/" + k: 2.0 for k in mr.LOSS_KEYS}
    p.dynamics_step_and_forward = fake
    buf = _FakeBuffer()
    out = p.update_dynamics(buf)
    assert set(out) == {"adv_dynamics_update/" + k for k in mr.LOSS_KEYS}
    assert len(seen) == expect and all(abs(v - 2.0) < 1e-12 for v in out.values())
    # draw order: the initial observations, then one dataset batch per model step; the next observations feed the next step
    assert len(buf.calls) == expect + n_roll and set(buf.calls) == {4}
    assert seen[0] == (1.0, 2.0)
    if length > 1:
        assert seen[1] == (101.0, 3.0)
    assert p.dynamics.model.training is False


def test_update_dynamics_refuses_multi_run_dynamics():
    d = _FakeDyn()
    d._n_runs = 2
    with pytest.raises(NotImplementedError, match="n_runs"):
        _policy(dynamics=d).update_dynamics(_FakeBuffer())


def test_select_action_applies_scaler_cpu():
    from offlinerlkit.utils.scaler import StandardScaler
    sc = StandardScaler(np.array([[1.0, -2.0, 0.5]], np.float32), np.array([[2.0, 0.5, 4.0]], np.float32))
    p = _policy(scaler=sc)
    obs = np.random.default_rng(0).normal(size=(5, 3)).astype(np.float32)
    a = p.select_action(obs, deterministic=True)
    p.scaler = None
    b = p.select_action(sc.transform(obs), deterministic=True)
    assert np.array_equal(a, b) and not np.array_equal(a, p.select_action(obs, deterministic=True))


def test_adversarial_abi_symbols():
    from offlinerlkit import _engine
    lib = _engine.load_library()
    adv = [s for s in _engine.ABI_SYMBOLS if s.startswith("orl_dynadv_")]
    assert sorted(adv) == sorted(["orl_dynadv_configure", "orl_dynadv_forward", "orl_dynadv_update", "orl_dynadv_adam_get",
                                  "orl_dynadv_adam_set"])
    for s in adv:
        assert hasattr(lib, s), s
    assert _engine.ADV_METRICS == ("all_loss", "sl_loss", "adv_loss", "adv_log_prob")
