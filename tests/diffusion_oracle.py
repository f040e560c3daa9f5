"""numpy oracle of DiffusionBC (reference: policy/others/diffusion.py + nets/unet.py at sequence length 1) for the tests.

The net is restated as what it is at length 1 -- the centre tap of every conv, GroupNorm + Mish, FiLM, residual paths and skip
concatenations -- with a hand-written backward; the schedules (squared-cosine betas, the DDPM update, the cosine learning rate with
warm-up, the EMA, Adam) are restated from DESIGN.md.  ``dtype`` float64 gives the comparison reference for gradient bounds."""
import math

import numpy as np


# ---- schedules -----------------------------------------------------------------------------------------------------------------
def betas(N):
    def abar(u):
        return math.cos((u + 0.008) / 1.008 * math.pi / 2) ** 2
    return np.array([min(1.0 - abar((i + 1) / N) / abar(i / N), 0.999) for i in range(N)], np.float64).astype(np.float32)


def alphas_cumprod(N):
    return np.cumprod(np.float32(1.0) - betas(N), dtype=np.float32)


def lr_at(k, T, warmup=500, lr_max=1e-4):
    if k < warmup:
        return lr_max * (k / warmup)
    return lr_max * max(0.0, 0.5 * (1.0 + math.cos(math.pi * (k - warmup) / max(1, T - warmup))))


def ema_decay(k):
    s = max(0, k - 1)
    return 0.0 if s <= 0 else min(1.0 - (1.0 + s) ** -0.75, 0.9999)


FINAL_GROUPS = 8      # final_conv's Conv1dBlock is built without n_groups: GroupNorm(8) whatever the blocks use


# ---- the net ---------------------------------------------------------------------------------------------------------------------
def block_plan(act_dim, down_dims):
    """[(module name, in, out, src block or -1, skip block or -1)] in execution order, and the index of the last block"""
    plan, level_out = [], []
    prev, cin = -1, act_dim
    for l, d in enumerate(down_dims):
        plan.append((f"down_modules.{l}.0", cin, d, prev, -1)); prev = len(plan) - 1
        plan.append((f"down_modules.{l}.1", d, d, prev, -1)); prev = len(plan) - 1
        level_out.append(prev)
        cin = d
    mid = down_dims[-1]
    for i in range(2):
        plan.append((f"mid_modules.{i}", mid, mid, prev, -1)); prev = len(plan) - 1
    for u in range(len(down_dims) - 1):
        l = len(down_dims) - 1 - u
        plan.append((f"up_modules.{u}.0", plan[prev][2] + down_dims[l], down_dims[l - 1], prev, level_out[l])); prev = len(plan) - 1
        plan.append((f"up_modules.{u}.1", down_dims[l - 1], down_dims[l - 1], prev, -1)); prev = len(plan) - 1
    return plan, prev


def _w(P, key, dt):
    w = P[key]
    if w.ndim == 3:
        w = w[:, :, w.shape[2] // 2]
    return w.astype(dt)


def softplus(x):
    return np.where(x > 20, x, np.log1p(np.exp(np.minimum(x, 20))))


def mish(x):
    return x * np.tanh(softplus(x))


def dmish(x):
    ts = np.tanh(softplus(x))
    return ts + x * (1.0 / (1.0 + np.exp(-x))) * (1.0 - ts * ts)


def gn_fwd(h, gamma, beta, G):
    B, C = h.shape
    hg = h.reshape(B, G, C // G)
    mean = hg.mean(axis=2, keepdims=True)
    var = ((hg - mean) ** 2).mean(axis=2, keepdims=True)
    rstd = 1.0 / np.sqrt(var + h.dtype.type(1e-5))
    xh = ((hg - mean) * rstd).reshape(B, C)
    return xh * gamma + beta, (xh, rstd)


def gn_bwd(du, gamma, cache, G):
    xh, rstd = cache
    B, C = du.shape
    dxh = (du * gamma).reshape(B, G, C // G)
    xg = xh.reshape(B, G, C // G)
    dh = rstd * (dxh - dxh.mean(axis=2, keepdims=True) - xg * (dxh * xg).mean(axis=2, keepdims=True))
    return dh.reshape(B, C), (du * xh).sum(axis=0), du.sum(axis=0)


def sinusoidal(t, dsed, dt):
    half = dsed // 2
    f = np.exp(np.arange(half, dtype=np.float32) * np.float32(-(math.log(10000) / (half - 1)))).astype(np.float32)
    arg = (np.asarray(t, np.float32)[:, None] * f[None, :]).astype(np.float32)
    return np.concatenate([np.sin(arg), np.cos(arg)], axis=1).astype(dt)


def forward(P, c, x, t, obs, dtype=np.float32, keep=False, e0=None):
    """x [B, act_dim], t [B], obs [B, obs_dim] -> the predicted noise [B, act_dim] (and the activations the backward reads);
    ``e0``: a given sinusoidal embedding [B, dsed] (an engine's own) in place of the one computed from t"""
    dt, G = dtype, c["n_groups"]
    plan, last = block_plan(c["act_dim"], c["down_dims"])
    x = x.astype(dt)
    e0 = sinusoidal(t, c["dsed"], dt) if e0 is None else np.asarray(e0).astype(dt)
    z1 = e0 @ _w(P, "diffusion_step_encoder.1.weight", dt).T + P["diffusion_step_encoder.1.bias"].astype(dt)
    m1 = mish(z1)
    emb = m1 @ _w(P, "diffusion_step_encoder.3.weight", dt).T + P["diffusion_step_encoder.3.bias"].astype(dt)
    gf = np.concatenate([emb, obs.astype(dt)], axis=1)
    mc = mish(gf)
    A = dict(e0=e0, z1=z1, m1=m1, gf=gf, mc=mc, blocks=[])
    outs = []
    for nm, cin, cout, src, skip in plan:
        X = x if src < 0 else outs[src]
        if skip >= 0:
            X = np.concatenate([X, outs[skip]], axis=1)
        film = mc @ _w(P, nm + ".cond_encoder.1.weight", dt).T + P[nm + ".cond_encoder.1.bias"].astype(dt)
        h1 = X @ _w(P, nm + ".blocks.0.block.0.weight", dt).T + P[nm + ".blocks.0.block.0.bias"].astype(dt)
        u1, c1 = gn_fwd(h1, P[nm + ".blocks.0.block.1.weight"].astype(dt), P[nm + ".blocks.0.block.1.bias"].astype(dt), G)
        y1 = film[:, :cout] * mish(u1) + film[:, cout:]
        h2 = y1 @ _w(P, nm + ".blocks.1.block.0.weight", dt).T + P[nm + ".blocks.1.block.0.bias"].astype(dt)
        u2, c2 = gn_fwd(h2, P[nm + ".blocks.1.block.1.weight"].astype(dt), P[nm + ".blocks.1.block.1.bias"].astype(dt), G)
        res = X @ _w(P, nm + ".residual_conv.weight", dt).T + P[nm + ".residual_conv.bias"].astype(dt) if cin != cout else X
        outs.append(mish(u2) + res)
        A["blocks"].append(dict(X=X, film=film, u1=u1, c1=c1, y1=y1, u2=u2, c2=c2))
    hf = outs[last] @ _w(P, "final_conv.0.block.0.weight", dt).T + P["final_conv.0.block.0.bias"].astype(dt)
    uf, cf = gn_fwd(hf, P["final_conv.0.block.1.weight"].astype(dt), P["final_conv.0.block.1.bias"].astype(dt), FINAL_GROUPS)
    yf = mish(uf)
    pred = yf @ _w(P, "final_conv.1.weight", dt).T + P["final_conv.1.bias"].astype(dt)
    A.update(outs=outs, uf=uf, cf=cf, yf=yf, gf=gf)
    return (pred, A) if keep else pred


def _set_grad(Gd, P, key, g):
    """the gradient of a centre tap into a zero tensor of the conv's full shape"""
    full = np.zeros(P[key].shape, g.dtype)
    if full.ndim == 3:
        full[:, :, full.shape[2] // 2] = g
    else:
        full[...] = g
    Gd[key] = full


def _skip_cols(dX, c1):
    """the skip half of the gradient of a concatenation [x | skip]: the columns from c1 on"""
    return dX[:, c1:]


def _clip_x0(x0):
    return np.clip(x0, -1.0, 1.0)


def loss_and_grads(P, c, act, t, eps, obs, dtype=np.float32, e0=None, keep=False):
    """one training batch -> (loss, pred, {state_dict key: gradient}, x_t) (and the forward's activations when ``keep``)"""
    dt, G = dtype, c["n_groups"]
    acp = alphas_cumprod(c["N"])
    xt = (np.sqrt(acp[t])[:, None] * act + np.sqrt(np.float32(1.0) - acp[t])[:, None] * eps).astype(np.float32)
    pred, A = forward(P, c, xt, t, obs, dtype, keep=True, e0=e0)
    B = len(t)
    diff = pred - eps.astype(dt)
    loss = (diff * diff).mean()
    dpred = 2.0 * diff / dt(B * c["act_dim"])
    plan, last = block_plan(c["act_dim"], c["down_dims"])
    Gd = {}
    _set_grad(Gd, P, "final_conv.1.weight", dpred.T @ A["yf"]); Gd["final_conv.1.bias"] = dpred.sum(axis=0)
    duf = dpred @ _w(P, "final_conv.1.weight", dt) * dmish(A["uf"])
    dhf, dg, db = gn_bwd(duf, P["final_conv.0.block.1.weight"].astype(dt), A["cf"], FINAL_GROUPS)
    Gd["final_conv.0.block.1.weight"], Gd["final_conv.0.block.1.bias"] = dg, db
    _set_grad(Gd, P, "final_conv.0.block.0.weight", dhf.T @ A["outs"][last]); Gd["final_conv.0.block.0.bias"] = dhf.sum(axis=0)
    douts = [None] * len(plan)
    douts[last] = dhf @ _w(P, "final_conv.0.block.0.weight", dt)
    dmc = np.zeros_like(A["mc"])
    for b in range(len(plan) - 1, -1, -1):
        nm, cin, cout, src, skip = plan[b]
        a = A["blocks"][b]
        dout = douts[b]
        dh2, dg, db = gn_bwd(dout * dmish(a["u2"]), P[nm + ".blocks.1.block.1.weight"].astype(dt), a["c2"], G)
        Gd[nm + ".blocks.1.block.1.weight"], Gd[nm + ".blocks.1.block.1.bias"] = dg, db
        _set_grad(Gd, P, nm + ".blocks.1.block.0.weight", dh2.T @ a["y1"]); Gd[nm + ".blocks.1.block.0.bias"] = dh2.sum(axis=0)
        dy1 = dh2 @ _w(P, nm + ".blocks.1.block.0.weight", dt)
        dfilm = np.concatenate([dy1 * mish(a["u1"]), dy1], axis=1)
        Gd[nm + ".cond_encoder.1.weight"] = dfilm.T @ A["mc"]; Gd[nm + ".cond_encoder.1.bias"] = dfilm.sum(axis=0)
        dmc = dmc + dfilm @ P[nm + ".cond_encoder.1.weight"].astype(dt)
        dh1, dg, db = gn_bwd(dy1 * a["film"][:, :cout] * dmish(a["u1"]), P[nm + ".blocks.0.block.1.weight"].astype(dt), a["c1"], G)
        Gd[nm + ".blocks.0.block.1.weight"], Gd[nm + ".blocks.0.block.1.bias"] = dg, db
        _set_grad(Gd, P, nm + ".blocks.0.block.0.weight", dh1.T @ a["X"]); Gd[nm + ".blocks.0.block.0.bias"] = dh1.sum(axis=0)
        dX = dh1 @ _w(P, nm + ".blocks.0.block.0.weight", dt)
        if cin != cout:
            _set_grad(Gd, P, nm + ".residual_conv.weight", dout.T @ a["X"]); Gd[nm + ".residual_conv.bias"] = dout.sum(axis=0)
            dX = dX + dout @ _w(P, nm + ".residual_conv.weight", dt)
        else:
            dX = dX + dout
        if src >= 0:
            c1 = plan[src][2]
            douts[src] = dX[:, :c1] if douts[src] is None else douts[src] + dX[:, :c1]
            if skip >= 0:
                douts[skip] = _skip_cols(dX, c1) if douts[skip] is None else douts[skip] + _skip_cols(dX, c1)
    dsed = c["dsed"]
    de = dmc[:, :dsed] * dmish(A["gf"][:, :dsed])
    Gd["diffusion_step_encoder.3.weight"] = de.T @ A["m1"]; Gd["diffusion_step_encoder.3.bias"] = de.sum(axis=0)
    dz1 = de @ P["diffusion_step_encoder.3.weight"].astype(dt) * dmish(A["z1"])
    Gd["diffusion_step_encoder.1.weight"] = dz1.T @ A["e0"]; Gd["diffusion_step_encoder.1.bias"] = dz1.sum(axis=0)
    return (loss, pred, Gd, xt, A) if keep else (loss, pred, Gd, xt)


def train(P, c, data, steps, total_steps):
    """Adam (lr of the schedule, no decay) + EMA over teacher-forced steps [(idx, t, eps)] -> (losses, final params, final EMA);
    the off-centre taps keep their values"""
    obs, act = data
    P = {k: v.copy() for k, v in P.items()}
    ema = {k: v.copy() for k, v in P.items()}
    m = {k: np.zeros_like(v) for k, v in P.items()}
    v_ = {k: np.zeros_like(v) for k, v in P.items()}
    losses = []
    f = np.float32
    for k, (idx, t, eps) in enumerate(steps):
        loss, _, Gd, _ = loss_and_grads(P, c, act[idx], t, eps, obs[idx])
        losses.append(float(loss))
        lr = lr_at(k, total_steps)
        bc1, bc2 = 1.0 - 0.9 ** (k + 1), 1.0 - 0.999 ** (k + 1)
        step, bc2s = f(lr / bc1), f(math.sqrt(bc2))
        d = ema_decay(k)
        for key in P:
            g = Gd[key].astype(f)
            m[key] = m[key] + (g - m[key]) * f(1.0 - 0.9)
            v_[key] = v_[key] * f(0.999) + f(1.0 - 0.999) * g * g
            P[key] = (P[key] - step * (m[key] / (np.sqrt(v_[key]) / bc2s + f(1e-8)))).astype(f)
            ema[key] = (ema[key] * f(d) + P[key] * f(1.0 - d)).astype(f)
    return np.array(losses, np.float64), P, ema


def sample(P, c, obs, init_noise, z, dtype=np.float32, trace=None):
    """select_action: x from init_noise [rows, 1, act_dim] through t = N-1 .. 0 with z[t] added for t > 0 -> [rows, act_dim].
    The five coefficients of a step are the fp32 table of ``policy/diffusion.py::ddpm_schedule`` whatever ``dtype`` is: float64 widens
    the net and the update, not the schedule.  ``trace``: a list that receives every step's x0 before the clip."""
    f, dt = np.float32, dtype
    acp = alphas_cumprod(c["N"])
    x = init_noise.reshape(len(obs), -1).astype(f).astype(dt)
    one = f(1.0)
    for t in range(c["N"] - 1, -1, -1):
        e = forward(P, c, x, np.full(len(obs), t), obs, dtype=dt)
        a, ap = acp[t], (acp[t - 1] if t > 0 else one)
        at = a / ap
        raw = (x - np.sqrt(one - a) * e) / np.sqrt(a)
        if trace is not None:
            trace.append(np.array(raw, np.float64))
        x0 = _clip_x0(raw).astype(dt)
        x = (np.sqrt(ap) * (one - at) / (one - a) * x0 + np.sqrt(at) * (one - ap) / (one - a) * x).astype(dt)
        if t > 0:
            x = (x + np.sqrt(max((one - ap) / (one - a) * (one - at), f(1e-20))) * z[t]).astype(dt)
    return x


# ---- the gradient norm of the checks --------------------------------------------------------------------------------------------
def grad_distance(a, b):
    """(relative, noise): over the tensors of the float64 gradient ``b`` whose scale exceeds 1e-9 of the largest tensor scale, the worst
    max |a - b| / max |b|; over the others -- structurally zero: everything upstream of a GroupNorm with one channel per group, whose
    output is its beta whatever it reads -- the largest |a|, which is fp32 cancellation noise"""
    top = max(float(np.abs(v).max()) for v in b.values())
    rel, noise = 0.0, 0.0
    for k, v in b.items():
        scale = float(np.abs(v).max())
        if scale > 1e-9 * top:
            rel = max(rel, float(np.abs(np.asarray(a[k], np.float64) - v).max() / scale))
        else:
            noise = max(noise, float(np.abs(a[k]).max()))
    return rel, noise


# ---- self-bounding float64 restatements (the bound type of tests/row_refs.py) ---------------------------------------------------
def sinusoidal_ref(t, dsed):
    """[sin(t f_j) | cos(t f_j)], f_j = exp(-j ln(1e4) / (half - 1)), in float64 with the first-order bound of an fp32 evaluation
    (u = 2^-24): one rounding each for the constant ln(1e4), the division by half - 1, the product with j and the product t f_j; a
    2 u library exp whose argument error the exponential turns into a relative one (so the constant's, the division's and the product's
    roundings arrive multiplied by j step = the argument itself); a 2 u library sin / cos on an argument that carries all of that,
    times |cos| / |sin|.  j = 0 is exact up to the sine: f_0 = exp(0) = 1 and the argument is the integer t.  -> a BV [len(t), dsed]"""
    import row_refs as rr
    half = dsed // 2
    j = np.arange(half, dtype=np.float64)
    const = rr.BV(np.array(math.log(10000.0)), rr.U * math.log(10000.0))             # what fp32 holds of ln(1e4): one rounding
    prod = rr.BV.exact(j) * (const / float(half - 1))
    f = rr.where(j == 0, 1.0, rr.exp(-prod))
    a = rr.BV.exact(np.asarray(t, np.float64)[:, None]) * rr.BV(f.v[None, :], f.e[None, :])
    a = rr.where(np.broadcast_to(j == 0, a.shape), rr.BV(a.v), a)                     # t * 1
    s, co = np.sin(a.v), np.cos(a.v)
    lib = lambda z, d: rr.BV(z, np.abs(d) * a.e + 2.0 * rr.U * np.abs(z) + rr.TINY)
    sn, cs = lib(s, co), lib(co, s)
    return rr.BV(np.concatenate([sn.v, cs.v], axis=1), np.concatenate([sn.e, cs.e], axis=1))


def adam_ema_f32(p, ema, m, v, g, lr, k, decay=None):
    """one step of ``train``'s update in fp32 numpy on flat arrays: Adam with the learning rate ``lr`` at optimizer step k (0-based),
    then the EMA with ``decay`` (``ema_decay(k)`` unless given) -> (p, ema, m, v)"""
    f = np.float32
    bc1, bc2 = 1.0 - float(f(0.9)) ** (k + 1), 1.0 - float(f(0.999)) ** (k + 1)
    step, bc2s = f(lr / bc1), f(math.sqrt(bc2))
    d = ema_decay(k) if decay is None else decay
    p, ema, m, v, g = (np.asarray(x, f) for x in (p, ema, m, v, g))
    m = m + (g - m) * (f(1.0) - f(0.9))
    v = v * f(0.999) + (f(1.0) - f(0.999)) * g * g
    p = (p - step * (m / (np.sqrt(v) / bc2s + f(1e-8)))).astype(f)
    ema = (ema * f(d) + p * f(1.0 - d)).astype(f)
    return p, ema, m, v


def adam_ema_ref(p, ema, m, v, g, lr, k, b1=0.9, b2=0.999, eps=1e-8):
    """the same step as value-with-bound arrays: torch.optim.Adam for the engine's fp32 betas (``row_refs.adam``'s formula and constants;
    the learning rate stays the double of the table, lr / (1 - b1^(k+1)) is rounded to fp32 once), then
    ema <- ema decay + p (1 - decay) with the two fp32 constants the launch receives: two products and one sum on top of p's own bound
    -> (p, ema, m, v) as BVs"""
    import row_refs as rr
    t = k + 1
    b1_, b2_ = float(np.float32(b1)), float(np.float32(b2))
    step, bc2s = float(lr) / (1.0 - b1_ ** t), math.sqrt(1.0 - b2_ ** t)
    step, bc2s = rr.BV(step, rr.U * abs(step)), rr.BV(bc2s, rr.U * abs(bc2s))
    p, ema, m, v, g = (rr.BV.exact(np.asarray(x, np.float32)) for x in (p, ema, m, v, g))
    m = m + (g - m) * rr.BV(1.0 - b1_)                      # 1 - b is exact in fp32 (Sterbenz)
    v = v * rr.BV.exact(b2_) + rr.BV(1.0 - b2_) * g * g
    p = p - step * (m / (rr.sqrt(v) / bc2s + rr.BV.exact(eps)))
    d = ema_decay(k)
    ema = ema * rr.BV.exact(np.float32(d)) + p * rr.BV.exact(np.float32(1.0 - d))
    return p, ema, m, v
