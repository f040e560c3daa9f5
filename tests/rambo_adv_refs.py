"""RAMBO's advantage (policy/model_based/rambo.py:164-181 of the reference) restated in numpy, any dtype: what k_adv_norm and the two
forward passes in front of it compute.  Shared by tests/test_rambo_device_cpu.py (against the reference's fixture) and
tests/test_gpu_rambo_device.py (against the engine)."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_cache = {}


def fixture():
    """rambo_adv_tiny.npz as a dict, loaded once and left unchanged"""
    if "g" not in _cache:
        with np.load(os.path.join(GOLD, "rambo_adv_tiny.npz")) as g:
            _cache["g"] = {k: g[k] for k in g.files}
    return _cache["g"]


def net_params(g, name):
    return {k[len(name) + 1:]: v for k, v in g.items() if k.startswith(name + "/")}


def _backbone(x, P):
    i = 0
    while f"backbone.model.{i}.weight" in P:
        x = np.maximum(x @ P[f"backbone.model.{i}.weight"].T + P[f"backbone.model.{i}.bias"], 0)
        i += 2
    return x


def actor_mode(obs, P):
    """a = tanh(mu), TanhNormalWrapper.log_prob at the mode with log sigma clamped to [-5, 2] (dist_module.py:17-42, 117-127)"""
    h = _backbone(obs, P)
    mu = h @ P["dist_net.mu.weight"].T + P["dist_net.mu.bias"]
    ls = np.clip(h @ P["dist_net.sigma.weight"].T + P["dist_net.sigma.bias"], -5.0, 2.0)
    a = np.tanh(mu)
    A = mu.shape[-1]
    logp = -ls.sum(-1) - 0.5 * A * np.log(2 * np.pi) - np.log(1 - a * a + 1e-6).sum(-1)
    return a, logp


def critic(obs, act, P):
    h = _backbone(np.concatenate([obs, act], -1), P)
    return (h @ P["last.weight"].T + P["last.bias"])[:, 0]


def hopper_done(next_obs):
    """termination_fn_hopper of the reference (its upper-bound-only ``abs(x < 100)`` included)"""
    ok = np.isfinite(next_obs).all(-1) & (next_obs[:, 1:] < 100).all(-1) & (next_obs[:, 0] > .7) & (np.abs(next_obs[:, 1]) < .2)
    return ~ok


def normalise(raw, dtype=np.float64):
    """(x - mean) / (std + 1e-6) with the unbiased standard deviation (torch's default)"""
    x = np.asarray(raw, dtype)
    return (x - x.mean()) / (x.std(ddof=1) + dtype(1e-6))


def advantage(obs, act, next_obs, reward, actor_p, c1_p, c2_p, gamma, alpha, include_ent, dtype=np.float64):
    cast = lambda P: {k: np.asarray(v, dtype) for k, v in P.items()}
    actor_p, c1_p, c2_p = cast(actor_p), cast(c1_p), cast(c2_p)
    term = hopper_done(np.asarray(next_obs))                       # on the fp32 rows, like the reference
    obs, act, nxt, rew = (np.asarray(x, dtype) for x in (obs, act, next_obs, reward))
    a2, logp = actor_mode(nxt, actor_p)
    qn = np.minimum(critic(nxt, a2, c1_p), critic(nxt, a2, c2_p))
    if include_ent:
        qn = qn - dtype(alpha) * logp
    value = rew + (1 - term.astype(dtype)) * dtype(gamma) * qn
    qb = np.minimum(critic(obs, act, c1_p), critic(obs, act, c2_p))
    raw = value - qb
    return dict(term=term.astype(np.float32), logp_next=logp, q_next=qn, value=value, q_base=qb, raw=raw, norm=normalise(raw, dtype))
