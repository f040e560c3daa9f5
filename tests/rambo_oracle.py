"""numpy restatement of RAMBO's adversarial model update (reference: policy/model_based/rambo.py:129-207) on dyn_oracle's network
conventions: the ensemble forward on the rollout + dataset rows, the sample, the elite mixture's log-probability (as a log-sum-exp),
the advantage-weighted policy-gradient term, the Gaussian NLL, their gradients and torch.optim.Adam (dyn_oracle.adam).  ``dtype`` is
np.float32 (pinned to tests/golden/rambo_tiny.npz by tests/test_rambo_cpu.py) or np.float64 (the reference of the GPU gradient and
stability tests).  Test infrastructure."""
import numpy as np

import dyn_oracle as orc

LOG_SQRT_2PI = 0.91893853320467274178
SL_LOGVAR_COEF = 0.001          # rambo.py:194 (not the config's logvar_loss_coef)


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def _softplus(y):
    return np.where(y > 20, y, np.log1p(np.exp(np.minimum(y, 20))))


def _dsoftplus(y):
    return np.where(y > 20, 1.0, _sig(y))


def forward(st, x, T):
    """x (N, in) shared by the members -> mean, logvar (K, N, D) and the cache of the backward, all in dtype T"""
    st = {k: np.asarray(v, T) for k, v in st.items()}
    L = orc.layers(st)
    h, hs, zs = np.asarray(x, T), [np.asarray(x, T)], []
    for i, (w, b) in enumerate(L):
        z = (np.matmul(h, st[w]) + st[b]).astype(T)
        if i < len(L) - 1:
            zs.append(z)
            h = (z * _sig(z)).astype(T)
            hs.append(h)
    D = z.shape[-1] // 2
    mean, raw = z[..., :D], z[..., D:]
    y1 = st["max_logvar"] - raw
    l1 = st["max_logvar"] - _softplus(y1)
    y2 = l1 - st["min_logvar"]
    lv = (st["min_logvar"] + _softplus(y2)).astype(T)
    return mean, lv, dict(hs=hs, zs=zs, y1=y1, y2=y2, st=st)


def step_forward(st, mu, std, rows, eps, model_idx, T=np.float32):
    """rows: obs, act, sl_obs, sl_act, sl_next_obs, sl_rew.  Returns the state the update needs; ``sample`` (Ba, D) is fp32-rounded
    like the engine's (and the reference's) even when T is float64"""
    Ba = len(rows["obs"])
    x = np.concatenate([np.concatenate([rows["obs"], rows["act"]], 1), np.concatenate([rows["sl_obs"], rows["sl_act"]], 1)], 0)
    x = ((x.astype(np.float32) - mu) / std).astype(np.float32)
    mean, lv, c = forward(st, x, T)
    mean = mean.copy()
    mean[:, :Ba, :-1] += rows["obs"].astype(T)
    sd = np.sqrt(np.exp(lv))
    i = np.arange(Ba)
    sample = (mean[model_idx, i] + sd[model_idx, i] * eps[model_idx, i].astype(T)).astype(np.float32)
    target = np.concatenate([rows["sl_next_obs"] - rows["sl_obs"], rows["sl_rew"].reshape(-1, 1)], 1).astype(np.float32)
    return dict(mean=mean, lv=lv, cache=c, sample=sample, target=target, Ba=Ba)


def step_grads(f, elites, advantage, adv_weight, decays, T=np.float32):
    """-> (dict all_loss, sl_loss, adv_loss, adv_log_prob, log_prob (Ba,)), gradients WITHOUT the decay terms)"""
    mean, lv, c, Ba = f["mean"], f["lv"], f["cache"], f["Ba"]
    st = c["st"]
    K, N, D = mean.shape
    Bs = N - Ba
    A = np.asarray(advantage, T).reshape(-1)
    inv = np.exp(-lv)
    # rollout rows: the mixture over the elites, log-sum-exp in double
    z = f["sample"].astype(T)[None] - mean[:, :Ba]
    sd = np.sqrt(np.exp(lv[:, :Ba]))
    var = sd * sd
    lp = (-(z * z) / (2 * var) - np.log(sd) - T(LOG_SQRT_2PI)).astype(np.float64).sum(-1)          # (K, Ba)
    el = np.asarray(elites)
    m = lp[el].max(0)
    ex = np.zeros_like(lp)
    ex[el] = np.exp(lp[el] - m)
    ssum = ex.sum(0)
    log_prob = m + np.log(ssum) - np.log(len(el))
    w = (ex / ssum).astype(T)
    coef = (T(adv_weight) * A / T(Ba))[None, :, None] * w[:, :, None]
    dmean_r = coef * z * inv[:, :Ba]
    dlv_r = coef * T(0.5) * (z * z * inv[:, :Ba] - 1)
    # dataset rows: the Gaussian NLL
    diff = mean[:, Ba:] - f["target"].astype(T)[None]
    s = T(1) / T(Bs * D)
    dmean_s = 2 * diff * inv[:, Ba:] * s
    dlv_s = (1 - diff ** 2 * inv[:, Ba:]) * s
    dmean, dlv = np.concatenate([dmean_r, dmean_s], 1), np.concatenate([dlv_r, dlv_s], 1)
    s1, s2 = _dsoftplus(c["y1"]), _dsoftplus(c["y2"])
    dl1 = dlv * s2
    g = {"max_logvar": (dl1 * (1 - s1)).sum(axis=(0, 1)) + SL_LOGVAR_COEF, "min_logvar": (dlv * (1 - s2)).sum(axis=(0, 1)) - SL_LOGVAR_COEF}
    dy = np.concatenate([dmean, dl1 * s1], -1).astype(T)
    L = orc.layers(st)
    for i in range(len(L) - 1, -1, -1):
        wn, bn = L[i]
        h = c["hs"][i]
        g[wn] = (np.einsum("ni,kno->kio", h, dy) if h.ndim == 2 else np.matmul(np.swapaxes(h, -1, -2), dy)).astype(T)
        g[bn] = dy.sum(axis=1, keepdims=True).astype(T)
        if i > 0:
            zz = c["zs"][i - 1]
            sg = _sig(zz)
            dy = (np.matmul(dy, np.swapaxes(st[wn], -1, -2)) * (sg * (1 + zz * (1 - sg)))).astype(T)
    decay = sum(float(wd) * 0.5 * float((st[wn].astype(np.float64) ** 2).sum()) for (wn, _), wd in zip(L, decays))
    sl = float((diff ** 2 * inv[:, Ba:]).mean(axis=(1, 2)).sum() + lv[:, Ba:].mean(axis=(1, 2)).sum()) + decay + \
        SL_LOGVAR_COEF * float(st["max_logvar"].sum()) - SL_LOGVAR_COEF * float(st["min_logvar"].sum())
    adv = float((log_prob * A.astype(np.float64)).mean())
    return dict(all_loss=adv_weight * adv + sl, sl_loss=sl, adv_loss=adv, adv_log_prob=float(log_prob.mean()), log_prob=log_prob), g


def with_decay(st, g, decays):
    """the gradient Adam sees: + wd_l W_l on the weights"""
    out = dict(g)
    for (w, _), wd in zip(orc.layers(st), decays):
        out[w] = (g[w] + np.float32(wd) * st[w]).astype(np.float32)
    return out


def step(st, opt, mu, std, rows, eps, model_idx, elites, advantage, adv_weight, decays, lr):
    """one fp32 dynamics_step_and_forward on ``st`` (updated in place through dyn_oracle.adam); returns (forward state, metrics, grads)"""
    f = step_forward(st, mu, std, rows, eps, model_idx)
    m, g = step_grads(f, elites, advantage, adv_weight, decays)
    g = {k: v.astype(np.float32) for k, v in g.items()}
    orc.adam(st, with_decay(st, g, decays), opt, lr)
    return f, m, g
