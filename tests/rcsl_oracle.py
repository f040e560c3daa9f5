"""numpy fp32 restatement of RCSL (reference: modules/rcsl_module.py:22-33 ``forward``, policy/rcsl/rcsl.py:123-151 ``learn``) on the
network pieces of oracle.nn, with the row-validity mask of the engine's ordered epoch.  Pinned to tests/golden/rcsl_*.npz by
tests/test_rcsl_cpu.py.  Test infrastructure.

State: {"rcsl": {backbone.model.{0, 2, ..., 2L}.{weight, bias}}, "opt": Adam state}; the last Linear is the plain output layer."""
from collections import OrderedDict

import numpy as np

from oracle import nn
from oracle.nn import f32


def init_state(net):
    st = OrderedDict(rcsl=nn.copy_net(net))
    st["opt"] = nn.adam_init(st["rcsl"])
    return st


def forward(net, obs, rtg):
    """-> (pred (B, A), x (B, obs_dim + 1), [x, h1, ..., hL])"""
    x = np.concatenate([np.asarray(obs, f32), np.asarray(rtg, f32).reshape(len(obs), 1)], axis=1)
    Ws, bs = nn.backbone_layers(net)
    hs = nn.mlp_fwd(x, Ws[:-1], bs[:-1])
    pred = (nn.mm(hs[-1], Ws[-1].T) + bs[-1]).astype(f32)
    return pred, x, hs


def learn(state, cfg, batch, valid=None):
    """One step.  ``valid`` (bool [B], default all): rows that count -- a padding row adds nothing to the loss, gets a zero gradient row,
    and the mean divides by valid rows x act_dim (the reference's partial last batch is the valid rows alone)."""
    net = state["rcsl"]
    act = np.asarray(batch["actions"], f32)
    B, A = act.shape
    valid = np.ones(B, bool) if valid is None else np.asarray(valid, bool)
    pred, x, hs = forward(net, batch["observations"], batch["rtgs"])
    d = np.where(valid[:, None], pred - act, f32(0)).astype(f32)
    cnt = f32(int(valid.sum()) * A)
    loss = f32((d * d).sum(dtype=f32) / cnt)
    dpred = (f32(2) * d / cnt).astype(f32)
    Ws, _ = nn.backbone_layers(net)
    idx = nn.backbone_indices(net)
    grads = OrderedDict()
    grads[f"backbone.model.{idx[-1]}.weight"] = nn.mm(dpred.T, hs[-1])
    grads[f"backbone.model.{idx[-1]}.bias"] = dpred.sum(axis=0, dtype=f32)
    dWs, dbs, _ = nn.mlp_bwd(hs, Ws[:-1], nn.mm(dpred, Ws[-1]), need_dx=False)
    for i, dW, db in zip(idx[:-1], dWs, dbs):
        grads[f"backbone.model.{i}.weight"] = dW
        grads[f"backbone.model.{i}.bias"] = db
    nn.adam_step(net, grads, state["opt"], cfg["lr"])
    return OrderedDict(loss=float(loss)), dict(pred=pred, x=x, grads=grads, dpred=dpred)
