"""numpy fp32 restatement of MOBILE (reference: dynamics/ensemble_dynamics.py:82-99 ``sample_next_obss``,
policy/model_based/mobile.py:130-142 ``compute_lcb`` and :144-196 ``learn``) on dyn_oracle's ensemble forward and the network pieces
of oracle.nn / oracle.sac.  Pinned to tests/golden/mobile_*.npz by tests/test_mobile_cpu.py.  Test infrastructure.

State: oracle.sac's (actor, critic1, critic2, critic1_old, critic2_old, log_alpha, opt).  Noise in the reference's draw order:
``dyn`` (S, E, B, obs_dim + 1) [randn_like per sample, ensemble_dynamics.py:97], ``eps_lcb`` (S * E * B, A) [compute_lcb's actforward],
``eps_next`` (B, A), ``eps_actor`` (B, A)."""
from collections import OrderedDict

import numpy as np

import dyn_oracle as dorc
from oracle import nn
from oracle.nn import f32


def sample_next_obss(dyn, scaler, elites, obs, act, noise):
    """-> (S, E, B, obs_dim): mean + eps * std of every elite in ``elites`` order, mean[..., :obs_dim] += obs; two fp32 roundings"""
    mu, std = scaler
    obs, act = np.asarray(obs, f32), np.asarray(act, f32)
    od = obs.shape[1]
    x = ((np.concatenate([obs, act], 1) - mu) / std).astype(f32)
    mean, lv, _ = dorc.forward(dyn, x)
    mean = mean.copy()
    mean[..., :od] += obs
    sd = np.sqrt(np.exp(lv)).astype(f32)
    el = np.asarray(elites, np.int64)
    mean, sd = mean[el], sd[el]
    prod = (np.asarray(noise, f32) * sd[None]).astype(f32)
    return (mean[None] + prod).astype(f32)[..., :od]


def lcb_from_samples(state, samples, eps_lcb):
    """compute_lcb behind the samples: -> (penalty (B, 1), qmin (S * E * B, 1))"""
    S, E, B, od = samples.shape
    nxt = samples.reshape(-1, od)
    a, _, _ = nn.tanh_gauss_fwd(state["actor"], nxt, eps_lcb)
    q1, _ = nn.critic_fwd(state["critic1_old"], nxt, a)
    q2, _ = nn.critic_fwd(state["critic2_old"], nxt, a)
    qmin = np.minimum(q1, q2).astype(f32)
    m = qmin.reshape(S, E, B, 1).mean(axis=0, dtype=f32)
    pen = m.astype(np.float64).std(axis=0, ddof=1).astype(f32)      # torch.std: unbiased
    return pen, qmin


def compute_lcb(state, cfg, dyn, scaler, obs, act, noise):
    samples = sample_next_obss(dyn, scaler, cfg["elites"], obs, act, noise["dyn"])
    return lcb_from_samples(state, samples, noise["eps_lcb"])


def learn(state, cfg, dyn, scaler, batch, noise):
    """``batch``: the mixed batch (real rows first, cfg["real_rows"] of them)"""
    obs = np.asarray(batch["observations"], f32)
    act = np.asarray(batch["actions"], f32)
    nobs = np.asarray(batch["next_observations"], f32)
    rew = np.asarray(batch["rewards"], f32).reshape(-1, 1)
    term = np.asarray(batch["terminals"], f32).reshape(-1, 1)
    B, od = obs.shape
    actor, c1, c2, c1o, c2o = state["actor"], state["critic1"], state["critic2"], state["critic1_old"], state["critic2_old"]
    alpha = state.get("_alpha", f32(np.exp(state["log_alpha"][0])) if cfg["auto_alpha"] else f32(cfg["alpha"]))
    aux = {}

    # ---- critics (mobile.py:151-167) ----
    q1, h1 = nn.critic_fwd(c1, obs, act)
    q2, h2 = nn.critic_fwd(c2, obs, act)
    pen, qmin = compute_lcb(state, cfg, dyn, scaler, obs, act, noise)
    pen = pen.copy()
    pen[:cfg["real_rows"]] = 0
    na, nlogp, _ = nn.tanh_gauss_fwd(actor, nobs, noise["eps_next"])
    nq1, _ = nn.critic_fwd(c1o, nobs, na)
    nq2, _ = nn.critic_fwd(c2o, nobs, na)
    next_q = np.minimum(nq1, nq2).astype(f32)
    if not cfg["deterministic_backup"]:
        next_q = (next_q - (alpha * nlogp).astype(f32)).astype(f32)
    rp = (rew - (f32(cfg["penalty_coef"]) * pen).astype(f32)).astype(f32)
    raw_target = (rp + ((f32(cfg["gamma"]) * (f32(1) - term)).astype(f32) * next_q).astype(f32)).astype(f32)
    target_q = np.where(raw_target < 0, f32(0), raw_target).astype(f32)           # torch.clamp(x, 0, None): a NaN stays
    critic_loss = f32((np.stack([q1 - target_q, q2 - target_q]) ** 2).mean(dtype=f32))
    for name, net, qq, hh in (("critic1", c1, q1, h1), ("critic2", c2, q2, h2)):
        g, _ = nn.critic_bwd(net, hh, (f32(2) * (qq - target_q) / f32(2 * B)).astype(f32), need_dx=False)
        nn.adam_step(net, g, state["opt"][name], cfg["critic_lr"])      # critics_optim: one Adam over both, one step count
        aux[name + "_grads"] = g
    aux.update(q1=q1, q2=q2, target_q=target_q, raw_target=raw_target, penalty=pen, lcb_q=qmin)

    # ---- actor against the UPDATED critics (mobile.py:169-175) ----
    a, logp, cache = nn.tanh_gauss_fwd(actor, obs, noise["eps_actor"])
    q1a, h1a = nn.critic_fwd(c1, obs, a)
    q2a, h2a = nn.critic_fwd(c2, obs, a)
    actor_loss = f32(-np.minimum(q1a, q2a).mean(dtype=f32) + alpha * logp.mean(dtype=f32))
    g1, g2 = nn.min2_grad(q1a, q2a, np.full((B, 1), -1.0 / B, dtype=f32))
    _, dx1 = nn.critic_bwd(c1, h1a, g1, need_dx=True, need_dw=False)
    _, dx2 = nn.critic_bwd(c2, h2a, g2, need_dx=True, need_dw=False)
    agr = nn.tanh_gauss_bwd(actor, cache, dx1[:, od:] + dx2[:, od:], np.full((B, 1), alpha / f32(B), dtype=f32))
    nn.adam_step(actor, agr, state["opt"]["actor"], cfg["actor_lr"])
    aux["q1a"], aux["q2a"] = q1a, q2a

    result = OrderedDict([("loss/actor", float(actor_loss)), ("loss/critic", float(critic_loss))])
    if cfg["auto_alpha"]:          # mobile.py:177-183
        lp_t = logp + f32(cfg["target_entropy"])
        la = state["log_alpha"]
        alpha_loss = f32(-(la[0] * lp_t).mean(dtype=f32))
        nn.adam_step({"log_alpha": la}, {"log_alpha": np.array([-(lp_t.mean(dtype=f32))], f32)}, state["opt"]["alpha"], cfg["alpha_lr"])
        alpha = f32(min(max(np.exp(la[0]), f32(0.0)), f32(1.0)))
        state["_alpha"] = alpha
        result["loss/alpha"] = float(alpha_loss)
        result["alpha"] = float(alpha)
    nn.polyak(c1o, c1, cfg["tau"])
    nn.polyak(c2o, c2, cfg["tau"])
    return result, aux
