"""numpy fp32 restatement of the autoregressive behaviour policy (reference: policy/others/autoregressive.py:28-54 ``forward``, :64-96
``fit``, :98-124 ``learn``), its hand-derived gradient, PyTorch-semantics Adam and sequential sampling, with the row-validity mask of the
engine's ordered epoch.  Pinned to tests/golden/ar_*.npz by tests/test_autoreg_cpu.py.  Test infrastructure.

State: {"model": {model.{0, 2, ..., 2L}.{weight, bias}}, "opt": Adam state}.  Every Linear, the last one included, is followed by
LeakyReLU(0.01); the two activated outputs are (mean, logstd)."""
from collections import OrderedDict

import numpy as np

from oracle import nn
from oracle.nn import f32

SLOPE = f32(0.01)
HALF_LOG_2PI = f32(0.9189385332046727)
PREFIX = "model."


def init_state(net):
    st = OrderedDict(model=nn.copy_net(net))
    st["opt"] = nn.adam_init(st["model"])
    return st


def leaky(z):
    return np.where(z > 0, z, SLOPE * z).astype(f32)


def expand(obs, act):
    """-> (X [A * B, od + 2 A], target [A * B]); expanded row j * B + b = [obs_b | act_b[k] 1[k < j] | onehot_j], target act_b[j]"""
    obs, act = np.asarray(obs, f32), np.asarray(act, f32)
    B, A = act.shape
    eye = np.eye(A, dtype=f32)
    mask = (np.tril(np.ones((A, A), f32)) - eye).astype(f32)
    x = np.concatenate([np.tile(obs, (A, 1)), np.tile(act, (A, 1)) * np.repeat(mask, B, axis=0), np.repeat(eye, B, axis=0)], axis=1)
    return x.astype(f32), act.T.reshape(-1).copy()


def forward_rows(net, x):
    """-> (hs = [x, h_1, ..., h_L, out] every one post-activation, zs = the pre-activations)"""
    Ws, bs = nn.backbone_layers(net, PREFIX)
    hs, zs = [np.asarray(x, f32)], []
    for W, b in zip(Ws, bs):
        z = (nn.mm(hs[-1], W.T) + b).astype(f32)
        zs.append(z)
        hs.append(leaky(z))
    return hs, zs


def learn(state, cfg, batch, valid=None):
    """One step.  ``valid`` (bool [B], default all): batch rows that count -- a padding row invalidates its A expanded rows, which add
    nothing to the loss and get zero gradient rows; the mean divides by valid rows x A (the reference's partial last batch)."""
    net = state["model"]
    act = np.asarray(batch["actions"], f32)
    B, A = act.shape
    valid = np.ones(B, bool) if valid is None else np.asarray(valid, bool)
    v = np.tile(valid, A)
    x, t = expand(batch["observations"], act)
    hs, zs = forward_rows(net, x)
    out = hs[-1]
    mean, ls = out[:, 0], out[:, 1]
    cnt = f32(int(valid.sum()) * A)
    inv_std = np.exp(-ls).astype(f32)
    d = ((t - mean) * inv_std).astype(f32)
    nll = (ls + f32(0.5) * d * d + HALF_LOG_2PI).astype(f32)
    loss = f32(np.where(v, nll, f32(0)).sum(dtype=f32) / cnt)
    dout = np.stack([np.where(v, -d * inv_std / cnt, f32(0)), np.where(v, (f32(1) - d * d) / cnt, f32(0))], axis=1).astype(f32)
    Ws, _ = nn.backbone_layers(net, PREFIX)
    idx = nn.backbone_indices(net, PREFIX)
    grads = OrderedDict()
    dh = dout
    dz_tail = None
    for l in reversed(range(len(Ws))):
        dz = (dh * np.where(hs[l + 1] > 0, f32(1), SLOPE)).astype(f32)
        if dz_tail is None:
            dz_tail = dz
        grads[f"{PREFIX}{idx[l]}.weight"] = nn.mm(dz.T, hs[l])
        grads[f"{PREFIX}{idx[l]}.bias"] = dz.sum(axis=0, dtype=f32)
        if l > 0:
            dh = nn.mm(dz, Ws[l])
    grads = OrderedDict((k, grads[k]) for k in net)
    nn.adam_step(net, grads, state["opt"], cfg["lr"])
    return OrderedDict(loss=float(loss)), dict(x=x, target=t, out=out, mean=mean, logstd=ls, z_tail=zs[-1], zs=zs, hs=hs, grads=grads, dz_tail=dz_tail)


def sample(net, obs, eps):
    """``forward`` for any number of rows: a_j = mean + e^logstd eps[:, j] from the pass whose input holds a_<j and onehot_j (the
    reference's ``logstd.exp() == 0 -> mean`` is the same value)"""
    obs, eps = np.asarray(obs, f32), np.asarray(eps, f32)
    n, A = eps.shape
    act = np.zeros((n, A), f32)
    eye = np.eye(A, dtype=f32)
    for j in range(A):
        x = np.concatenate([obs, act, np.tile(eye[j], (n, 1))], axis=1)
        out = forward_rows(net, x)[0][-1]
        act[:, j] = (out[:, 0] + np.exp(out[:, 1]).astype(f32) * eps[:, j]).astype(f32)
    return act

