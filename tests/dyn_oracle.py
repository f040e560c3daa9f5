"""numpy fp32 restatement of the dynamics ensemble's learn() / validate() (reference: dynamics/ensemble_dynamics.py:178-217,
modules/dynamics_module.py): forward with Swish, soft_clamp, the Gaussian NLL with decay and logvar terms, its backward, and
torch.optim.Adam.  Test infrastructure: pinned to tests/golden/dyn_*.npz (tests/test_dynamics_cpu.py)."""
import numpy as np

F = np.float32


def _sig(x):
    return (F(1) / (F(1) + np.exp(-x))).astype(F)


def _softplus(y):
    return np.where(y > 20, y, np.log1p(np.exp(np.minimum(y, 20)))).astype(F)


def _dsoftplus(y):
    return np.where(y > 20, F(1), _sig(y)).astype(F)


def layers(st):
    n = 0
    while f"backbones.{n}.weight" in st:
        n += 1
    return [(f"backbones.{i}.weight", f"backbones.{i}.bias") for i in range(n)] + [("output_layer.weight", "output_layer.bias")]


def forward(st, x):
    """x: (K, B, in) or (B, in); returns mean, logvar, and the cache of the backward"""
    hs, zs = [x.astype(F)], []
    h = x.astype(F)
    L = layers(st)
    for i, (w, b) in enumerate(L):
        z = (np.matmul(h, st[w]) + st[b]).astype(F)
        if i < len(L) - 1:
            zs.append(z)
            h = (z * _sig(z)).astype(F)
            hs.append(h)
        else:
            out = z
    D = out.shape[-1] // 2
    mean, raw = out[..., :D], out[..., D:]
    mx, mn = st["max_logvar"].astype(F), st["min_logvar"].astype(F)
    y1 = mx - raw
    l1 = mx - _softplus(y1)
    y2 = l1 - mn
    lv = mn + _softplus(y2)
    return mean, lv, dict(hs=hs, zs=zs, y1=y1, y2=y2)


def loss_and_grads(st, x, t, decays, coef):
    mean, lv, c = forward(st, x)
    K, B, D = mean.shape
    inv = np.exp(-lv).astype(F)
    diff = mean - t
    loss = ((diff ** 2 * inv).mean(axis=(1, 2)).sum() + lv.mean(axis=(1, 2)).sum()).astype(np.float64)
    L = layers(st)
    decay = sum(float(wd) * 0.5 * float((st[w].astype(np.float64) ** 2).sum()) for (w, _), wd in zip(L, decays))
    loss = loss + decay + coef * st["max_logvar"].sum() - coef * st["min_logvar"].sum()
    s = F(1) / F(B * D)
    dmean = 2 * diff * inv * s
    dlv = (1 - diff ** 2 * inv) * s
    s1, s2 = _dsoftplus(c["y1"]), _dsoftplus(c["y2"])
    dl1 = dlv * s2
    g = {"max_logvar": (dl1 * (1 - s1)).sum(axis=(0, 1)) + coef, "min_logvar": (dlv * (1 - s2)).sum(axis=(0, 1)) - coef}
    dy = np.concatenate([dmean, dl1 * s1], axis=-1).astype(F)
    for i in range(len(L) - 1, -1, -1):
        w, b = L[i]
        h = c["hs"][i]
        g[w] = (np.matmul(np.swapaxes(h, -1, -2), dy) + decays[i] * st[w]).astype(F)
        g[b] = dy.sum(axis=1, keepdims=True).astype(F)
        if i > 0:
            z = c["zs"][i - 1]
            sg = _sig(z)
            dy = (np.matmul(dy, np.swapaxes(st[w], -1, -2)) * (sg * (1 + z * (1 - sg)))).astype(F)
    return float(loss), g


def adam(st, g, opt, lr, b1=0.9, b2=0.999, eps=1e-8):
    opt["t"] = opt.get("t", 0) + 1
    t = opt["t"]
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    for k, gk in g.items():
        m = opt.setdefault(("m", k), np.zeros_like(gk))
        v = opt.setdefault(("v", k), np.zeros_like(gk))
        m += (gk - m) * F(1 - b1)
        v *= F(b2)
        v += F(1 - b2) * gk * gk
        st[k] = (st[k] - F(lr / bc1) * (m / (np.sqrt(v) / F(np.sqrt(bc2)) + F(eps)))).astype(F)


def learn(st, opt, x, t, batch, decays, coef, lr):
    """one learn() epoch on (K, T, ...) arrays; returns the mean minibatch loss and the last minibatch's gradients"""
    losses, g = [], None
    T = x.shape[1]
    for b in range(int(np.ceil(T / batch))):
        loss, g = loss_and_grads(st, x[:, b * batch:(b + 1) * batch], t[:, b * batch:(b + 1) * batch], decays, coef)
        adam(st, g, opt, lr)
        losses.append(loss)
    return float(np.mean(losses)), g


def validate(st, x, t):
    mean, _, _ = forward(st, x)
    return ((mean - t) ** 2).mean(axis=(1, 2))
