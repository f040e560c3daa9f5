#!/usr/bin/env python3
"""Golden vectors for RNNDynamics from the REAL reference, run on the CPU.  Usage: make_rnn_golden.py <reference root>.

The reference's own code: ``RNNModel`` (offlinerlkit/nets/rnn.py) and ``RNNDynamics`` (offlinerlkit/dynamics/rnn_dynamics.py), loaded
from the reference tree as they are.  The reference's ``offlinerlkit.dynamics`` package pulls in gym / mujoco and its logger pulls in
tensorboard: both are replaced by stubs (a package holding only ``BaseDynamics`` and a logger that records what it is given), the
approach of make_dyn_golden.py.  Inputs come from rnn_cases.py; only the reference's outputs are stored.

Dropout: every ``ResBlock.dropout`` of the loaded reference model is replaced by a module that draws the keep mask itself
(``torch.rand >= p``), applies ``x * keep / (1 - p)`` as ``nn.Dropout`` does and records the mask; the float64 run replays the masks.
The float64 gradients come from the project's own ``offlinerlkit.nets.RNNModel`` (the reference's forward casts its input to float32),
which tests/test_rnn_cpu.py holds to this fixture in float32.

Per single-step fixture: pred, loss, the taps the reference exposes (the last GRU layer's output, the input block, the merge layer,
every residual block), the float64 autograd gradient of every tensor (rnn_default: DIGEST seeded entries and the
scale of every tensor), ``grad_f32_vs_f64`` = the distance of the reference's own fp32 gradient from it in the norm of
diffusion_oracle.grad_distance, ``grad_zero_noise`` = the fp32 noise on structurally zero tensors (rnn_t1: W_hh at T = 1), and the
packed keep masks.  The script asserts what the tests rely on and prints the measured distances."""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True
import rnn_cases as rc  # noqa: E402
import rnn_oracle as orc  # noqa: E402
from diffusion_oracle import grad_distance  # noqa: E402


def _load_file(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


class StubLogger:
    def __init__(self, model_dir):
        self.model_dir = model_dir
        self.rows, self._sum, self._cnt, self.calls = [], {}, {}, []

    def logkv_mean(self, k, v):
        self.calls.append((k, float(v)))
        self._sum[k] = self._sum.get(k, 0.0) + float(v)
        self._cnt[k] = self._cnt.get(k, 0) + 1

    def set_timestep(self, t):
        self._t = t

    def dumpkvs(self, exclude=None):
        self.exclude = exclude
        row = {k: self._sum[k] / self._cnt[k] for k in self._sum}
        row["timestep"] = self._t
        self.rows.append(row)
        self._sum, self._cnt = {}, {}


def import_reference(root):
    """-> (the reference's RNNModel, RNNDynamics, StandardScaler)"""
    rnn = _load_file("ref_rnn", os.path.join(root, "offlinerlkit", "nets", "rnn.py"))
    saved = {k: sys.modules.get(k) for k in list(sys.modules) if k == "offlinerlkit" or k.startswith("offlinerlkit.")}
    for k in saved:
        del sys.modules[k]
    for pkg in ("offlinerlkit", "offlinerlkit.dynamics", "offlinerlkit.utils"):
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    bd = _load_file("offlinerlkit.dynamics.base_dynamics", os.path.join(root, "offlinerlkit/dynamics/base_dynamics.py"))
    sys.modules["offlinerlkit.dynamics"].BaseDynamics = bd.BaseDynamics
    sc = _load_file("offlinerlkit.utils.scaler", os.path.join(root, "offlinerlkit/utils/scaler.py"))
    lg = types.ModuleType("offlinerlkit.utils.logger")
    lg.Logger = StubLogger
    sys.modules["offlinerlkit.utils.logger"] = lg
    rd = _load_file("offlinerlkit.dynamics.rnn_dynamics", os.path.join(root, "offlinerlkit/dynamics/rnn_dynamics.py"))
    for k in [k for k in sys.modules if k == "offlinerlkit" or k.startswith("offlinerlkit.")]:
        del sys.modules[k]
    sys.modules.update({k: v for k, v in saved.items() if v is not None})
    return rnn.RNNModel, rd.RNNDynamics, sc.StandardScaler


class RecordingDropout(nn.Module):
    """nn.Dropout(p) that draws its keep mask in the open and records it, or replays the masks it is given"""

    def __init__(self, p, gen=None, replay=None):
        super().__init__()
        self.p, self.gen, self.replay, self.masks = p, gen, replay, []

    def forward(self, x):
        if not self.training:
            return x
        if self.replay is not None:
            keep = torch.from_numpy(self.replay).to(x.dtype)
        else:
            keep = (torch.rand(x.shape, generator=self.gen) >= self.p).to(x.dtype)
            self.masks.append(keep.numpy().copy())
        return x * keep / (1.0 - self.p)


def blocks_of(model):
    return [model.input_layer] + list(model.backbones)


def build(Model, c, P, dtype=torch.float32, replay=None, gen=None):
    m = Model(c["input_dim"], c["output_dim"], hidden_dims=list(c["hidden"]), rnn_num_layers=c["L"], dropout_rate=c["p"])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()}, strict=True)
    m = m.to(dtype)
    if c["p"] > 0:
        for s, b in enumerate(blocks_of(m)):
            b.dropout = RecordingDropout(c["p"], gen=gen, replay=None if replay is None else replay[s])
    return m


def loss_fn(preds, targets, masks):
    return (((preds - targets) ** 2).mean(-1) * masks).mean()


def single_step(Ref, Ours, c):
    P = rc.make_params(c)
    x, tg, mk = rc.make_data(c)
    idx = np.arange(c["B"])
    gen = torch.Generator()
    gen.manual_seed(c["seed"])
    ref = build(Ref, c, P, gen=gen)
    ref.train()
    taps = {}
    hooks = [ref.input_layer.register_forward_hook(lambda m, i, o: taps.__setitem__("in", o.detach().numpy().copy())),
             ref.activation.register_forward_hook(lambda m, i, o: taps.__setitem__("merge", o.detach().numpy().copy())),
             ref.rnn_layer.register_forward_hook(lambda m, i, o: taps.__setitem__(f"gru.{c['L'] - 1}", o[0].detach().numpy().reshape(-1, c["H"]).copy()))]
    for i, b in enumerate(ref.backbones):
        hooks.append(b.register_forward_hook(lambda m, inp, o, i=i: taps.__setitem__(f"block.{i}", o.detach().numpy().copy())))
    pred, _ = ref(torch.from_numpy(x[idx]))
    loss = loss_fn(pred, torch.from_numpy(tg[idx]), torch.from_numpy(mk[idx]))
    loss.backward()
    for h in hooks:
        h.remove()
    g32 = {k: p.grad.numpy().copy() for k, p in ref.named_parameters()}
    drop = None
    if c["p"] > 0:
        drop = np.stack([b.dropout.masks[0] for b in blocks_of(ref)])
        assert all(len(b.dropout.masks) == 1 for b in blocks_of(ref))
    ours = build(Ours, c, P, torch.float64, replay=drop)
    ours.train()
    pred64, _ = ours(torch.from_numpy(x[idx]).double())
    loss64 = loss_fn(pred64, torch.from_numpy(tg[idx]).double(), torch.from_numpy(mk[idx]).double())
    loss64.backward()
    g64 = {k: p.grad.numpy().copy() for k, p in ours.named_parameters()}
    dist, noise = grad_distance(g32, g64)
    # the numpy oracle: float64 equals float64 autograd, float32 sits inside the bar with room
    ol64, _, og64, _ = orc.loss_and_grads(P, c, x[idx], tg[idx], mk[idx], drop, np.float64)
    worst64 = max(float(np.abs(og64[k] - g64[k]).max() / max(np.abs(g64[k]).max(), 1e-300)) for k in g64 if np.abs(g64[k]).max() > 0)
    ol32, op32, og32, oc32 = orc.loss_and_grads(P, c, x[idx], tg[idx], mk[idx], drop, np.float32)
    od, on = grad_distance(og32, g64)
    print(f"{c['name']}: loss {loss.item():.6f}; fp32 vs float64 autograd, worst tensor {dist:.3e} (noise on zero tensors {noise:.3e}); "
          f"oracle64 vs autograd64 {worst64:.2e}; oracle32: pred {np.abs(op32 - pred.detach().numpy()).max():.2e} grads {od:.3e} / {on:.3e}")
    assert worst64 < 1e-10 and abs(ol64 - loss64.item()) < 1e-12
    assert od <= 4 * dist and on <= 4 * noise and dist > 0
    out = {"loss": np.float64(loss.item()), "loss64": np.float64(loss64.item()), "grad_f32_vs_f64": np.float64(dist),
           "grad_zero_noise": np.float64(noise)}
    if drop is not None:
        out["drop_masks"] = rc.pack_masks(drop)
        print(f"    keep rate {drop.mean():.4f}")
    if c["name"] == "rnn_default":
        out["pred"] = pred.detach().numpy()[:, list(rc.PRED_STEPS)]
        for k, v in g64.items():
            pos = rc.digest_positions(c, k, v.size)
            out[f"grad64/{k}"] = v.ravel()[pos]
            out[f"gscale/{k}"] = np.float64(np.abs(v).max())
            d = float(np.abs(g32[k].ravel()[pos] - v.ravel()[pos]).max() / np.abs(v).max())
            assert d <= dist
    else:
        out["pred"] = pred.detach().numpy()
        out.update({f"tap/{k}": v for k, v in taps.items()})
        out.update({f"grad64/{k}": v for k, v in g64.items()})
    np.savez_compressed(os.path.join(HERE, c["name"] + ".npz"), **out)


def run_traj(Ref, RefDyn, c, P):
    x, tg, mk = rc.make_data(c)
    model = build(Ref, c, P)
    model.train()
    optim = torch.optim.Adam(model.parameters(), lr=c["lr"])
    dyn = RefDyn(model, optim, None, None)
    losses, first = [], None
    for k, idx in enumerate(rc.make_steps(c)):
        losses.append(dyn.learn((torch.from_numpy(x[idx]), torch.from_numpy(tg[idx]), torch.from_numpy(mk[idx]))))
        if k == 0:
            first = ({n: optim.state[p]["exp_avg"].numpy().copy() for n, p in model.named_parameters()},
                     {n: optim.state[p]["exp_avg_sq"].numpy().copy() for n, p in model.named_parameters()})
    return np.array(losses, np.float64), {k: v.detach().numpy().copy() for k, v in model.named_parameters()}, first


def traj(Ref, RefDyn, c):
    P = rc.make_params(c)
    losses, fin, (m1, v1) = run_traj(Ref, RefDyn, c, P)
    twin = {k: np.nextafter(v, np.float32(np.inf)).astype(np.float32) for k, v in P.items()}
    tl, tfin, _ = run_traj(Ref, RefDyn, c, twin)
    ol, ofin, _ = orc.train(P, c, rc.make_data(c), rc.make_steps(c), c["lr"])
    assert {len(s) for s in rc.make_steps(c)} == {16, 8}
    print(f"rnn_traj: losses {losses[0]:.5f} .. {losses[-1]:.5f}; twin max |dloss| {np.abs(tl - losses).max():.2e}; oracle {np.abs(ol - losses).max():.2e}; "
          f"params: twin {max(np.abs(tfin[k] - fin[k]).max() for k in fin):.2e} oracle {max(np.abs(ofin[k] - fin[k]).max() for k in fin):.2e}")
    out = {"losses": losses, "losses_twin": tl}
    for k in fin:
        out[f"final/{k}"], out[f"final_twin/{k}"], out[f"m1/{k}"], out[f"v1/{k}"] = fin[k], tfin[k], m1[k], v1[k]
    np.savez_compressed(os.path.join(HERE, "rnn_traj.npz"), **out)


class RecordingData:
    """a map-style data set of (inputs, targets, masks) that records the order its items are fetched in"""

    def __init__(self, x, tg, mk):
        self.x, self.tg, self.mk, self.fetched = x, tg, mk, []

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        self.fetched.append(int(i))
        return self.x[i], self.tg[i], self.mk[i]


def trace(Ref, RefDyn, Scaler, c):
    P = rc.make_params(c)
    x, tg, mk = rc.make_data(c)
    obss, actions, mu, std = rc.make_windows(c)
    model = build(Ref, c, P)
    optim = torch.optim.Adam(model.parameters(), lr=c["lr"])
    dyn = RefDyn(model, optim, Scaler(mu, std), rc.terminal_fn)
    data = RecordingData(x, tg, mk)
    with tempfile.TemporaryDirectory() as tmp:
        logger = StubLogger(tmp)
        torch.manual_seed(c["torch_seed"])
        dyn.train(data, c["B"], c["epochs"], logger)
        files = sorted(os.listdir(tmp))
        keys = list(torch.load(os.path.join(tmp, "dynamics.pth")).keys())
    orders = np.array(data.fetched, np.int64).reshape(c["epochs"], c["n"])
    assert all(sorted(o) == list(range(c["n"])) for o in orders.tolist())
    assert not model.training and logger.exclude == ["policy_training_progress"]
    nxt, rew, term, info = dyn.step(obss, actions)
    margin = np.abs(np.abs(nxt).max(-1) - rc.TERMINAL_AT).min()
    print(f"rnn_trace: files {files}; epoch losses {[r['loss/model'] for r in logger.rows]}; terminals {term.ravel().astype(int)}; "
          f"nearest |next_obs| to the terminal threshold {margin:.3f}")
    assert margin > 1e-2 and term.any() and not term.all() and info == {}
    assert files == ["dynamics.pth", "mu.npy", "std.npy"]
    out = {"orders": orders, "batch_losses": np.array([v for _, v in logger.calls], np.float64),
           "epoch_losses": np.array([r["loss/model"] for r in logger.rows], np.float64),
           "timesteps": np.array([r["timestep"] for r in logger.rows], np.int64), "logger_keys": np.array(sorted(logger.rows[0].keys())),
           "state_dict_keys": np.array(keys), "next_obss": nxt.astype(np.float32), "rewards": rew.astype(np.float32),
           "terminals": term.astype(np.bool_)}
    out.update({f"final/{k}": v.detach().numpy().copy() for k, v in model.named_parameters()})
    np.savez_compressed(os.path.join(HERE, "rnn_trace.npz"), **out)


def main(root):
    torch.set_num_threads(1)
    Ref, RefDyn, Scaler = import_reference(root)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "offlinerl-kit_amd"))
    from offlinerlkit.nets import RNNModel as Ours
    for name in ("rnn_tiny", "rnn_t1", "rnn_odd", "rnn_default"):
        single_step(Ref, Ours, rc.CASES[name])
    traj(Ref, RefDyn, rc.CASES["rnn_traj"])
    trace(Ref, RefDyn, Scaler, rc.CASES["rnn_trace"])
    for name in rc.CASES:
        size = os.path.getsize(os.path.join(HERE, name + ".npz"))
        print(f"{name}.npz", size, "bytes")
        assert size < 600 * 1024


if __name__ == "__main__":
    main(sys.argv[1])
