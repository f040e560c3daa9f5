"""Self-bounding float64 restatements of the dynamics ensemble's own kernels (csrc/dynamics.hip: gather / step / adversarial input,
Gaussian NLL head and its reduction, Adam with the folded decay term, the loss cells, validate's MSE, step()'s head, MOBILE's and RAMBO's
samplers, RAMBO's adversarial head, reduction and metrics), written from the formulas of the reference that the kernel comments cite
(modules/dynamics_module.py soft_clamp, dynamics/ensemble_dynamics.py step / sample_next_obss / learn / validate,
policy/model_based/rambo.py:129-207) -- not from the kernel code.  Built on ``row_refs.BV`` (value + first-order fp32 error bound); the
bar a caller holds a kernel to is ``row_refs.FACTOR`` x the propagated bound on every element, as derived in row_refs.py.

Operands read back from the engine are exact.  So is ONE correctly rounded fp32 operation on exact operands when numpy fp32 performs the
same operation (``mean + obs``, ``(x - mu) / std``): both sides round the same real number the same way, the
build uses no fast-math.  That is how the input kernels are held bit for bit, and it keeps the cancellation ``sample - mean`` of the
adversarial head from inflating its bound.

Sums: a column sum over (member, row) is one wave's 64-lane strided loop and 6-step shuffle tree, ``ceil(n / 64) + 6`` rounding steps
(``row_refs.wave_terms``, by the derivation of ``sum_terms``); a sum over the D dims by one thread is D - 1 sequential steps.
Double-precision accumulations (the penalty, the mixture's log-sum-exp, the adversarial means) contribute no rounding of their own at
fp32 scale: only their operands' errors and the final cast to fp32 enter.  Where softplus switches branch at 20 both branches agree to
2e-9, far inside the bound, so float64 may take either."""
import math

import numpy as np

import row_refs as rr
from row_refs import BV, U

f32 = np.float32
F64 = np.float64
SL_LOGVAR_COEF = 0.001          # rambo.py:194
MODES = ("aleatoric", "pairwise-diff", "ensemble_std")


def rup4(n):
    return (n + 3) // 4 * 4


# ---- the input kernels: bit for bit -------------------------------------------------------------------------------------------------
def scale_rows(x, mu, std):
    """StandardScaler.transform in fp32, zero pads up to a multiple of 4 columns"""
    x = np.asarray(x, f32)
    out = np.zeros(x.shape[:-1] + (rup4(x.shape[-1]),), f32)
    out[..., :x.shape[-1]] = (x - np.asarray(mu, f32)) / np.asarray(std, f32)
    return out


def gather(data_in, data_tg, idx, mu, std):
    """rows ``idx`` (any shape) of the dataset -> (X [..., pitch0] scaled with zero pads, T [..., D])"""
    idx = np.asarray(idx, np.int64)
    return scale_rows(np.asarray(data_in, f32)[idx], mu, std), np.asarray(data_tg, f32)[idx].copy()


def adv_input(obs, act, sl_obs, sl_act, sl_next, sl_rew, mu, std):
    """rambo.py:137-150: -> (X [Ba + Bs, pitch0], T [Bs, D] = [sl_next - sl_obs, sl_rew], the kept obs [Ba, od])"""
    x = np.concatenate([np.concatenate([obs, act], 1), np.concatenate([sl_obs, sl_act], 1)], 0).astype(f32)
    t = np.concatenate([np.asarray(sl_next, f32) - np.asarray(sl_obs, f32), np.asarray(sl_rew, f32).reshape(-1, 1)], 1)
    return scale_rows(x, mu, std), t, np.asarray(obs, f32).copy()


def same_bits(got, ref, tag):
    got, ref = np.ascontiguousarray(got, f32), np.ascontiguousarray(ref, f32)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    bad = got.view(np.uint32) != ref.view(np.uint32)
    assert not bad.any(), (tag, "bits differ at", np.argwhere(bad)[:4].tolist(), got[bad][:4], ref[bad][:4])


# ---- soft_clamp and the Gaussian NLL element ----------------------------------------------------------------------------------------
def log1p(x):
    x = BV.exact(x)
    return rr._lib(np.log1p(x.v), x.e / np.abs(1.0 + x.v))


def softplus(y):
    """torch.nn.functional.softplus (beta 1, threshold 20)"""
    y = BV.exact(y)
    yc = BV(np.minimum(y.v, 20.0), y.e)
    return rr.where(y.v > 20.0, y, log1p(rr.exp(yc)))


def dsoftplus(y):
    y = BV.exact(y)
    yc = BV(np.minimum(y.v, 20.0), y.e)
    return rr.where(y.v > 20.0, 1.0, 1.0 / (1.0 + rr.exp(-yc)))


def soft_clamp(raw, mx, mn):
    """dynamics_module.py:19-29: l1 = max - softplus(max - raw), lv = min + softplus(l1 - min); s1 = d l1 / d raw, s2 = d lv / d l1"""
    raw, mx, mn = np.asarray(raw, f32), np.asarray(mx, f32), np.asarray(mn, f32)
    y1 = BV.exact(mx) - BV.exact(raw)
    l1 = BV.exact(mx) - softplus(y1)
    y2 = l1 - BV.exact(mn)
    return BV.exact(mn) + softplus(y2), dsoftplus(y1), dsoftplus(y2)


def std_of(raw, mx, mn):
    """std = sqrt(exp(logvar)) as ensemble_dynamics.py:62 writes it"""
    return rr.sqrt(rr.exp(soft_clamp(raw, mx, mn)[0]))


def nll_elem(mean, raw, target, mx, mn, rows, D):
    """one element of mean over (rows, D) of [(mean - target)^2 exp(-lv) + lv] (ensemble_dynamics.py:199-203) and its gradient:
    -> dmean, draw, lterm, gmax, gmin (the element's shares of the max / min_logvar gradients)"""
    lv, s1, s2 = soft_clamp(raw, mx, mn)
    inv = rr.exp(-lv)
    diff = BV.exact(mean) - BV.exact(target)
    sq = diff * diff * inv
    scale = 1.0 / (BV.exact(float(rows)) * float(D))
    dlv = (1.0 - sq) * scale
    dl1 = dlv * s2
    return 2.0 * diff * inv * scale, dl1 * s1, sq + lv, dl1 * (1.0 - s1), dlv * (1.0 - s2)


def col_sums(a):
    """[K, rows, D] -> [D]: one wave per column over the K * rows (member, row) pairs"""
    a = BV.exact(a)
    return rr.sum_(a.reshape(-1, a.shape[-1]), axis=0, stride=64)


def logvar_term(mx, mn, coef):
    c = BV.exact(f32(coef))
    return c * rr.sum_(BV.exact(mx), sequential=True) - c * rr.sum_(BV.exact(mn), sequential=True)


def nll_reduce(lterm, gmax, gmin, mx, mn, coef, rows):
    """the loss without the decay term, sum_k mean_(rows, D) + coef (sum max_logvar - sum min_logvar), and the max / min_logvar gradients"""
    D = lterm.shape[-1]
    ls = rr.sum_(col_sums(lterm), sequential=True)
    nll = ls / (BV.exact(float(rows)) * float(D)) + logvar_term(mx, mn, coef)
    return nll, col_sums(gmax) + f32(coef), col_sums(gmin) - f32(coef)


def val_mse(out, target):
    """ensemble_dynamics.py:211-217: per member, mean over (row, dim) of (mean - target)^2.  out [K, H, 2D], target [H, D]"""
    D = np.asarray(target).shape[-1]
    d = BV.exact(np.asarray(out, f32)[..., :D]) - BV.exact(np.asarray(target, f32)[None])
    K = d.shape[0]
    return rr.sum_((d * d).reshape(K, -1), axis=1) / float(d.v[0].size)


# ---- the flat parameter block: decay loss, Adam -------------------------------------------------------------------------------------
def flat_layout(tensors, decays, P):
    """(wd [P]: the weight decay that applies to each float, trainable [P] bool) from the tensor table (name, offset, shape)"""
    wd, tr = np.zeros(P, f32), np.zeros(P, bool)
    for name, off, shape in tensors:
        n = int(np.prod(shape))
        if "saved_" in name:
            continue
        tr[off:off + n] = True
        if name.endswith(".weight"):
            l = len(decays) - 1 if name.startswith("output_layer") else int(name.split(".")[1])
            wd[off:off + n] = f32(decays[l])
    return wd, tr


def decay(flat, wd):
    """0.5 wd_l sum W_l^2 (dynamics_module.py get_decay_loss) per 1024-float block of the parameter block: four floats per thread added one
    after the other, scaled, then the 256 threads of the block.  -> BV [nblk]"""
    P = flat.size
    nblk = (P + 1023) // 1024
    w = np.zeros(nblk * 1024, f32)
    w[:P] = np.where(wd > 0, flat, 0)
    s = np.zeros(nblk * 1024, f32)
    s[:P] = wd
    w, s = BV.exact(w.reshape(-1, 4)), s.reshape(-1, 4)
    assert (s == s[:, :1]).all()                  # a thread's four floats share one tensor
    q = rr.sum_(w * w, axis=1, sequential=True) * (BV.exact(f32(0.5)) * BV.exact(s[:, 0]))
    return rr.sum_(q.reshape(nblk, 256), axis=1)


def adam(flat, m, v, G, wd, trainable, lr, b1, b2, eps, t, torch_scalars=False):
    """torch.optim.Adam on the gradient G + wd W (the decay loss's gradient) at step t; the floats outside ``trainable`` (saved_*, pads)
    keep their values with a zero bound.  -> (p, m, v) BV [P]"""
    g = BV.exact(G) + BV.exact(wd) * BV.exact(flat)
    g = rr.where(wd > 0, g, BV.exact(G))          # wd = 0: G + 0 * w is G exactly
    p2, m2, v2 = rr.adam(flat, m, v, g, lr, b1, b2, eps, t, torch_scalars=torch_scalars)
    return rr.where(trainable, p2, flat), rr.where(trainable, m2, m), rr.where(trainable, v2, v)


def loss_cell(nll, decay_part):
    """one minibatch's loss: nll + sum of the decay partial sums (all exact read-backs)"""
    return BV.exact(nll) + rr.sum_(BV.exact(decay_part))


# ---- step(): ensemble_dynamics.py:45-80 --------------------------------------------------------------------------------------------
def _means(out, obs, D):
    """mean[..., :od] += obs in fp32 (exact on exact operands): [K, n, D]"""
    mean = np.asarray(out, f32)[..., :D].copy()
    od = obs.shape[-1]
    mean[..., :od] += np.asarray(obs, f32)[None]
    return mean


def _sample(mean, eps, std):
    """mean + eps std evaluated wider than fp32, rounded once"""
    v = mean + eps * std.v
    return BV(v, np.abs(eps) * std.e + U * np.abs(v))


def head(out, obs, noise, midx, mx, mn, mode, coef):
    """out [K, n, 2D], obs [n, od], noise [K, n, D], midx [n] -> (next_obs [n, od], raw_reward [n], penalty [n], reward [n]).
    The penalty runs over ALL K members; the sample comes from member midx[i]."""
    out = np.asarray(out, f32)
    K, n, D = out.shape[0], out.shape[1], out.shape[2] // 2
    od = obs.shape[-1]
    mean = _means(out, obs, D).astype(F64)
    std = std_of(out[..., D:], mx, mn)
    i = np.arange(n)
    s = _sample(mean[midx, i], np.asarray(noise, f32)[midx, i].astype(F64), std[midx, i])
    if mode == "aleatoric":            # max over members of ||std||_2 over all out dims
        ss = BV((std.v ** 2).sum(-1), (2.0 * std.v * std.e).sum(-1))
        nk = BV(np.sqrt(ss.v), ss.e / (2.0 * np.sqrt(ss.v)))
        pen = BV(nk.v.max(0), nk.e.max(0))
    else:
        mo = mean[..., :od]
        mb = mo.mean(0)
        mb_e = U * np.abs(mb)          # held as fp32
        df = mo - mb[None]
        df_e = mb_e[None] + U * np.abs(df)
        if mode == "pairwise-diff":    # max over members of ||mean_k - mean of the means||_2 over the obs dims
            ss = (df ** 2).sum(-1)
            ss_e = (2.0 * np.abs(df) * df_e).sum(-1)
            with np.errstate(divide="ignore", invalid="ignore"):
                nk_e = np.where(ss > 0, ss_e / (2.0 * np.sqrt(np.where(ss > 0, ss, 1.0))), np.sqrt(ss_e))
            pen = BV(np.sqrt(ss).max(0), nk_e.max(0))
        else:                          # sqrt(mean over obs dims of the variance over members)
            vs = (df ** 2).mean(0).sum(-1) / od
            vs_e = (2.0 * np.abs(df) * df_e).mean(0).sum(-1) / od
            with np.errstate(divide="ignore", invalid="ignore"):
                pen = BV(np.sqrt(vs), np.where(vs > 0, vs_e / (2.0 * np.sqrt(np.where(vs > 0, vs, 1.0))), np.sqrt(vs_e)))
    pen = BV(pen.v, pen.e + U * np.abs(pen.v))          # the cast to fp32
    raw = s[:, od]
    return s[:, :od], raw, pen, raw - BV.exact(f32(coef)) * pen


def sample_next(out, obs, noise, elites, mx, mn):
    """ensemble_dynamics.py:82-99: out [K, n, 2D], noise [S, E, n, D] -> [S, E, n, od] = mean_e + (eps * std_e), two fp32 roundings"""
    out = np.asarray(out, f32)
    D, od = out.shape[2] // 2, obs.shape[-1]
    el = np.asarray(elites, np.int64)
    mean = _means(out, obs, D)[el][..., :od]
    std = std_of(out[el][..., D:D + od], mx[:od], mn[:od])
    eps = BV.exact(np.asarray(noise, f32)[..., :od])
    return BV.exact(mean[None]) + eps * BV(std.v[None], std.e[None])


def adv_sample(out, obs, noise, midx, mx, mn):
    """rambo.py:152-160 (Normal(mean, std).sample() of each row's member): out [K, N, 2D] (rollout rows first), noise [K, Ba, D] -> S [Ba, D]"""
    out = np.asarray(out, f32)
    Ba, D = obs.shape[0], out.shape[2] // 2
    i = np.arange(Ba)
    o = out[:, :Ba]
    mean = _means(o, obs, D)[midx, i]
    std = std_of(o[..., D:], mx, mn)[midx, i]
    return BV.exact(mean) + std * BV.exact(np.asarray(noise, f32)[midx, i])


# ---- RAMBO's adversarial update: rambo.py:162-207 -----------------------------------------------------------------------------------
def adv_head(out, obs, S, T, adv, elites, mx, mn, adv_weight):
    """out [K, Ba + Bs, 2D], obs [Ba, od], S [Ba, D] (the kept sample), T [Bs, D], adv [Ba] ->
    dict(rowlp [Ba] (double: compare hi + lo), dout [K, N, 2D], lterm, gmax, gmin [K, N, D]).
    Rollout rows: log_prob_i = logsumexp_{k in elites} sum_d Normal(mean_k, std_k).log_prob(s) - log(n_elites) and the gradient of
    adv_weight mean_i(A_i log_prob_i); dataset rows: the Gaussian NLL over the Bs rows (``nll_elem``)."""
    out = np.asarray(out, f32)
    K, N, D = out.shape[0], out.shape[1], out.shape[2] // 2
    Ba = obs.shape[0]
    Bs = N - Ba
    o = out[:, :Ba]
    mean = _means(o, obs, D)
    lv, s1, s2 = soft_clamp(o[..., D:], mx, mn)
    sd = rr.sqrt(rr.exp(lv))
    z = BV.exact(np.asarray(S, f32)[None]) - BV.exact(mean)
    lp = -(z * z) / (2.0 * (sd * sd)) - rr.log(sd) - rr.LOG_SQRT_2PI
    s = BV(lp.v.sum(-1), lp.e.sum(-1))                                  # [K, Ba], summed in double
    el = np.asarray(elites, np.int64)
    m = s.v[el].max(0)
    ex = np.zeros_like(s.v)
    ex[el] = np.exp(s.v[el] - m)
    w = ex / ex.sum(0)
    we = (w * s.e).sum(0)
    rowlp = BV(m + np.log(ex.sum(0)) - math.log(len(el)), we)
    wk = BV(w, w * (s.e + we[None]) + U * w)                            # softmax weight, cast to fp32
    c0 = BV.exact(f32(adv_weight)) * BV.exact(adv) / float(Ba)
    c = (c0.reshape(1, -1) * wk).reshape(K, Ba, 1)
    inv = rr.exp(-lv)
    dlv = c * 0.5 * (z * z * inv - 1.0)
    dl1 = dlv * s2
    r = (c * z * inv, dl1 * s1, BV(np.zeros((K, Ba, D))), dl1 * (1.0 - s1), dlv * (1.0 - s2))
    d = nll_elem(out[:, Ba:, :D], out[:, Ba:, D:], np.asarray(T, f32)[None], mx, mn, Bs, D)
    cat = [BV(np.concatenate([a.v, b.v], 1), np.concatenate([a.e, b.e], 1)) for a, b in zip(r, d)]
    dout = BV(np.concatenate([cat[0].v, cat[1].v], -1), np.concatenate([cat[0].e, cat[1].e], -1))
    return dict(rowlp=rowlp, dout=dout, lterm=cat[2], gmax=cat[3], gmin=cat[4])


def adv_reduce(lterm, gmax, gmin, rowlp, adv, mx, mn, Ba):
    """-> (sl loss without the decay term over the Bs dataset rows, max / min_logvar gradients over ALL rows (+- 0.001),
    advm = [mean_i(log_prob_i A_i), mean_i(log_prob_i)] held as fp32)"""
    lterm = BV.exact(lterm)
    Bs, D = lterm.shape[1] - Ba, lterm.shape[2]
    ls = rr.sum_(col_sums(lterm[:, Ba:]), sequential=True)
    nll = ls / (BV.exact(float(Bs)) * float(D)) + logvar_term(mx, mn, SL_LOGVAR_COEF)
    lp = np.asarray(rowlp, F64)
    a0, a1 = float((lp * np.asarray(adv, f32).astype(F64)).mean()), float(lp.mean())
    advm = BV(np.array([a0, a1]), U * np.abs(np.array([a0, a1])))
    return nll, col_sums(gmax) + f32(SL_LOGVAR_COEF), col_sums(gmin) - f32(SL_LOGVAR_COEF), advm


def adv_metrics(nll, decay_part, advm, adv_weight):
    """rambo.py:196-207: [all_loss, sl_loss, adv_loss, mean log_prob]"""
    sl = loss_cell(np.asarray(nll, f32).reshape(()), decay_part)
    a = BV.exact(np.asarray(advm, f32))
    return rr.stack([BV.exact(f32(adv_weight)) * a[0] + sl, sl, a[0], a[1]])


def split_hi_lo(pairs):
    """the (hi, lo) float pairs a double comes back as -> float64"""
    p = np.asarray(pairs, f32).astype(F64)
    return p[..., 0] + p[..., 1]
