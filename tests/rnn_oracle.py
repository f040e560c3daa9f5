"""numpy restatement of RNNModel / RNNDynamics.learn (reference: nets/rnn.py, dynamics/rnn_dynamics.py) in float32 or float64: forward,
the masked MSE, the backward of every tensor and torch.optim.Adam.  Test infrastructure, as tests/diffusion_oracle.py is.

Arrays: x [B, T, in]; the tail works on the B * T rows in batch_first order (row b * T + t).  ``drop``: keep masks
[len(hidden), B * T, H] of 0 / 1 (entry 0 the input block, entry 1 + i residual block i) or None for eval mode; kept values are scaled
by 1 / (1 - p)."""
import numpy as np

EPS_LN = 1e-5


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def _cast(P, dtype):
    return {k: np.asarray(v, dtype) for k, v in P.items()}


def _ln(u, g, b):
    mean = u.mean(-1, keepdims=True)
    var = ((u - mean) ** 2).mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + u.dtype.type(EPS_LN))
    xh = (u - mean) * rstd
    return xh * g + b, (xh, rstd)


def _ln_bwd(dy, g, cache):
    xh, rstd = cache
    dg, db = (dy * xh).sum(0), dy.sum(0)
    dxh = dy * g
    du = rstd * (dxh - dxh.mean(-1, keepdims=True) - xh * (dxh * xh).mean(-1, keepdims=True))
    return du, dg, db


def forward(P, c, x, drop=None, dtype=np.float32):
    """-> (pred [B, T, out], cache); cache["taps"] holds gru.<l>, in, merge, block.<i> as [B * T, H]"""
    P = _cast(P, dtype)
    x = np.asarray(x, dtype)
    B, T, _ = x.shape
    H, L, nb = c["H"], c["L"], len(c["hidden"]) - 1
    one = dtype(1.0)
    scale = one / (one - dtype(c["p"])) if drop is not None else one
    cache = {"x": x, "gru": [], "taps": {}}
    seq = x
    for l in range(L):
        Wih, Whh = P[f"rnn_layer.weight_ih_l{l}"], P[f"rnn_layer.weight_hh_l{l}"]
        bih, bhh = P[f"rnn_layer.bias_ih_l{l}"], P[f"rnn_layer.bias_hh_l{l}"]
        GI = seq @ Wih.T + bih
        h = np.zeros((B, H), dtype)
        R, Z, N, HN, HP, HO = (np.zeros((B, T, H), dtype) for _ in range(6))
        for t in range(T):
            gh = h @ Whh.T + bhh
            r = _sig(GI[:, t, :H] + gh[:, :H])
            z = _sig(GI[:, t, H:2 * H] + gh[:, H:2 * H])
            n = np.tanh(GI[:, t, 2 * H:] + r * gh[:, 2 * H:])
            HP[:, t], R[:, t], Z[:, t], N[:, t], HN[:, t] = h, r, z, n, gh[:, 2 * H:]
            h = (one - z) * n + z * h
            HO[:, t] = h
        cache["gru"].append(dict(X=seq, R=R, Z=Z, N=N, HN=HN, HP=HP))
        cache["taps"][f"gru.{l}"] = HO.reshape(B * T, H)
        seq = HO
    x2 = x.reshape(B * T, -1)

    def block(inp, res, key, slot):
        zpre = inp @ P[key + ".linear.weight"].T + P[key + ".linear.bias"]
        s = zpre * _sig(zpre)
        m = None if drop is None else np.asarray(drop[slot], dtype) * scale
        u = s if m is None else s * m
        if res is not None:
            u = res + u
        y, lnc = _ln(u, P[key + ".layer_norm.weight"], P[key + ".layer_norm.bias"])
        return y, dict(inp=inp, zpre=zpre, m=m, ln=lnc, key=key, res=res is not None)

    yin, cin = block(x2, None, "input_layer", 0)
    cat = np.concatenate([yin, seq.reshape(B * T, H)], axis=-1)
    zm = cat @ P["merge_layer.weight"].T + P["merge_layer.bias"]
    y = zm * _sig(zm)
    cache["taps"]["in"], cache["taps"]["merge"] = yin, y
    cache.update(cin=cin, cat=cat, zm=zm, blocks=[])
    for i in range(nb):
        y, cb = block(y, y, f"backbones.{i}", 1 + i)
        cache["blocks"].append(cb)
        cache["taps"][f"block.{i}"] = y
    cache["last"] = y
    pred = y @ P["output_layer.weight"].T + P["output_layer.bias"]
    return pred.reshape(B, T, -1), cache


def loss_of(pred, targets, masks):
    return (((pred - targets) ** 2).mean(-1) * masks).mean()


def loss_and_grads(P, c, x, targets, masks, drop=None, dtype=np.float32):
    """-> (loss, pred [B, T, out], {tensor: gradient}, cache)"""
    Pd = _cast(P, dtype)
    pred, cache = forward(P, c, x, drop, dtype)
    targets, masks = np.asarray(targets, dtype), np.asarray(masks, dtype)
    B, T, od = pred.shape
    H, L, nb = c["H"], c["L"], len(c["hidden"]) - 1
    loss = loss_of(pred, targets, masks)
    G = {}
    dpred = (dtype(2.0) * (pred - targets) * masks[..., None] / dtype(od * B * T)).reshape(B * T, od)
    G["output_layer.weight"], G["output_layer.bias"] = dpred.T @ cache["last"], dpred.sum(0)
    dy = dpred @ Pd["output_layer.weight"]

    def block_bwd(dy, cb):
        key = cb["key"]
        du, G[key + ".layer_norm.weight"], G[key + ".layer_norm.bias"] = _ln_bwd(dy, Pd[key + ".layer_norm.weight"], cb["ln"])
        ds = du if cb["m"] is None else du * cb["m"]
        sg = _sig(cb["zpre"])
        dz = ds * sg * (1 + cb["zpre"] * (1 - sg))
        G[key + ".linear.weight"], G[key + ".linear.bias"] = dz.T @ cb["inp"], dz.sum(0)
        dinp = dz @ Pd[key + ".linear.weight"]
        return dinp + du if cb["res"] else dinp

    for i in range(nb - 1, -1, -1):
        dy = block_bwd(dy, cache["blocks"][i])
    sg = _sig(cache["zm"])
    dzm = dy * sg * (1 + cache["zm"] * (1 - sg))
    G["merge_layer.weight"], G["merge_layer.bias"] = dzm.T @ cache["cat"], dzm.sum(0)
    dcat = dzm @ Pd["merge_layer.weight"]
    block_bwd(dcat[:, :H], cache["cin"])
    dH = dcat[:, H:].reshape(B, T, H)
    one = dtype(1.0)
    for l in range(L - 1, -1, -1):
        g = cache["gru"][l]
        Whh, Wih = Pd[f"rnn_layer.weight_hh_l{l}"], Pd[f"rnn_layer.weight_ih_l{l}"]
        dGI, dGH = np.zeros((B, T, 3 * H), dtype), np.zeros((B, T, 3 * H), dtype)
        carry = np.zeros((B, H), dtype)
        for t in range(T - 1, -1, -1):
            dh = dH[:, t] + carry
            r, z, n, hn, hp = g["R"][:, t], g["Z"][:, t], g["N"][:, t], g["HN"][:, t], g["HP"][:, t]
            gn = dh * (one - z) * (one - n * n)
            gz = dh * (hp - n) * z * (one - z)
            gr = gn * hn * r * (one - r)
            dGI[:, t] = np.concatenate([gr, gz, gn], -1)
            dGH[:, t] = np.concatenate([gr, gz, gn * r], -1)
            carry = dh * z + dGH[:, t] @ Whh
        gi2, gh2 = dGI.reshape(B * T, 3 * H), dGH.reshape(B * T, 3 * H)
        G[f"rnn_layer.weight_hh_l{l}"], G[f"rnn_layer.bias_hh_l{l}"] = gh2.T @ g["HP"].reshape(B * T, H), gh2.sum(0)
        G[f"rnn_layer.weight_ih_l{l}"], G[f"rnn_layer.bias_ih_l{l}"] = gi2.T @ g["X"].reshape(B * T, -1), gi2.sum(0)
        dH = dGI @ Wih
    return loss, pred, G, cache


def adam_step(P, G, M, V, k, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam's step k + 1 (0-based k) in float32, in place"""
    f = np.float32
    bc1, bc2 = 1.0 - b1 ** (k + 1), 1.0 - b2 ** (k + 1)
    step, bc2s = f(lr / bc1), f(np.sqrt(bc2))
    for key in P:
        g = G[key].astype(f)
        M[key] = M[key] + (g - M[key]) * f(1.0 - b1)
        V[key] = V[key] * f(b2) + f(1.0 - b2) * g * g
        P[key] = P[key] - step * (M[key] / (np.sqrt(V[key]) / bc2s + f(eps)))


def train(P, c, data, steps, lr=1e-3):
    """the optimizer steps ``steps`` (row indices each) of RNNDynamics.learn in float32 -> (losses, final parameters, (exp_avg, exp_avg_sq) after step 1)"""
    inputs, targets, masks = data
    P = {k: v.astype(np.float32).copy() for k, v in P.items()}
    M = {k: np.zeros_like(v) for k, v in P.items()}
    V = {k: np.zeros_like(v) for k, v in P.items()}
    losses, first = [], None
    for k, idx in enumerate(steps):
        loss, _, G, _ = loss_and_grads(P, c, inputs[idx], targets[idx], masks[idx])
        adam_step(P, G, M, V, k, lr)
        losses.append(float(loss))
        if k == 0:
            first = ({a: b.copy() for a, b in M.items()}, {a: b.copy() for a, b in V.items()})
    return np.array(losses, np.float64), P, first
