"""numpy fp32 restatement of Gaussian RCSL (reference: modules/rcsl_gauss_module.py:42-54 ``get_dist_params``, modules/dist_module.py:80-93,
policy/rcsl/rcsl_gauss.py:123-154 ``learn``) on the network pieces of oracle.nn, with the row-validity mask of the engine's ordered epoch.
Pinned to tests/golden/rcslg_*.npz by tests/test_rcsl_gauss_cpu.py.  Test infrastructure.

State: {"rcsl": {backbone.model.{0, 2, ..., 2L}.{weight, bias}, dist_net.{mu, sigma}.{weight, bias}}, "opt": Adam state}.  The last
backbone Linear yields the latent z (act_dim wide); the clamped sigma output is read as a log-variance, as the reference's loss reads it."""
from collections import OrderedDict

import numpy as np

from oracle import nn
from oracle.nn import f32

LO, HI = f32(-5.0), f32(2.0)


def init_state(net):
    st = OrderedDict(rcsl=nn.copy_net(net))
    st["opt"] = nn.adam_init(st["rcsl"])
    return st


def forward(net, obs, rtg):
    """-> (mu (B, A), logvar (B, A) post-clamp, cache)"""
    x = np.concatenate([np.asarray(obs, f32), np.asarray(rtg, f32).reshape(len(obs), 1)], axis=1)
    Ws, bs = nn.backbone_layers(net)
    hs = nn.mlp_fwd(x, Ws[:-1], bs[:-1])
    z = (nn.mm(hs[-1], Ws[-1].T) + bs[-1]).astype(f32)
    mu = (nn.mm(z, net["dist_net.mu.weight"].T) + net["dist_net.mu.bias"]).astype(f32)
    raw = (nn.mm(z, net["dist_net.sigma.weight"].T) + net["dist_net.sigma.bias"]).astype(f32)
    logvar = np.clip(raw, LO, HI).astype(f32)
    return mu, logvar, dict(x=x, hs=hs, z=z, raw=raw)


def learn(state, cfg, batch, valid=None):
    """One step.  ``valid`` (bool [B], default all): rows that count -- a padding row adds nothing to the loss, gets zero gradient rows,
    and both means divide by valid rows x act_dim (the reference's partial last batch is the valid rows alone)."""
    net = state["rcsl"]
    act = np.asarray(batch["actions"], f32)
    B, A = act.shape
    valid = np.ones(B, bool) if valid is None else np.asarray(valid, bool)
    v = valid[:, None]
    mu, logvar, c = forward(net, batch["observations"], batch["rtgs"])
    z, hs, raw = c["z"], c["hs"], c["raw"]
    cnt = f32(int(valid.sum()) * A)
    d = np.where(v, mu - act, f32(0)).astype(f32)
    iv = np.exp(-logvar).astype(f32)
    q = (d * d * iv).astype(f32)
    loss = f32(q.sum(dtype=f32) / cnt + np.where(v, logvar, f32(0)).sum(dtype=f32) / cnt)
    dmu = (f32(2) * d * iv / cnt).astype(f32)
    is_open = (raw >= LO) & (raw <= HI)                       # torch.clamp passes the gradient where lo <= x <= hi
    ds = np.where(v & is_open, (f32(1) - q) / cnt, f32(0)).astype(f32)
    grads = OrderedDict()
    grads["dist_net.mu.weight"] = nn.mm(dmu.T, z)
    grads["dist_net.mu.bias"] = dmu.sum(axis=0, dtype=f32)
    grads["dist_net.sigma.weight"] = nn.mm(ds.T, z)
    grads["dist_net.sigma.bias"] = ds.sum(axis=0, dtype=f32)
    dz = (nn.mm(dmu, net["dist_net.mu.weight"]) + nn.mm(ds, net["dist_net.sigma.weight"])).astype(f32)
    Ws, _ = nn.backbone_layers(net)
    idx = nn.backbone_indices(net)
    grads[f"backbone.model.{idx[-1]}.weight"] = nn.mm(dz.T, hs[-1])
    grads[f"backbone.model.{idx[-1]}.bias"] = dz.sum(axis=0, dtype=f32)
    dWs, dbs, _ = nn.mlp_bwd(hs, Ws[:-1], nn.mm(dz, Ws[-1]), need_dx=False)
    for i, dW, db in zip(idx[:-1], dWs, dbs):
        grads[f"backbone.model.{i}.weight"] = dW
        grads[f"backbone.model.{i}.bias"] = db
    nn.adam_step(net, grads, state["opt"], cfg["lr"])
    return OrderedDict(loss=float(loss)), dict(mu=mu, logvar=logvar, z=z, raw=raw, x=c["x"], grads=grads, dz=dz)
