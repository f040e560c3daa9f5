#!/usr/bin/env python3
"""Golden vectors for the dynamics ensemble (offlinerlkit.dynamics, csrc/dynamics.hip) from the REAL reference's
``EnsembleDynamics`` (dynamics/ensemble_dynamics.py) and ``EnsembleDynamicsModel`` (modules/dynamics_module.py), run on the CPU.

The reference's ``offlinerlkit.dynamics`` package pulls in gym / mujoco and its logger pulls in tensorboard: both are replaced by
stubs (a package holding only ``BaseDynamics`` and a logger that records the key-values it is given); every other file is loaded
from the reference tree as it is.  Usage: make_dyn_golden.py <reference root>.

Fixtures:
  dyn_tiny.npz     obs 3, act 2, [32, 32], 3 members, 2 elites, nonzero decays: three teacher-forced learn() epochs (150 rows,
                   batch 64: a partial last batch), the losses, full parameters after every epoch and the max / min_logvar gradients
                   of the last minibatch; validate(); step() in the three penalty modes with its recorded noise and model indices
  dyn_mopo.npz     17 / 6, [200] x 4, 7 members, the launcher's decays: one learn() epoch of 600 rows, losses and parameter digests
  dyn_trace.npz    whole train() on a synthetic set (500 rows) under fixed seeds: split, bootstrap and shuffle indices, per-epoch
                   train / holdout losses, stop epoch, elites; the script asserts that every improvement and elite decision has a
                   margin far above fp32 noise
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
import synth  # noqa: E402

TINY = dict(obs_dim=3, act_dim=2, hidden=[32, 32], K=3, elites=2, decays=[1e-4, 2.5e-4, 5e-4], T=150, B=64, epochs=3, H=40, N=40,
            seed=31, coef=0.01, lr=1e-3)
MOPO = dict(obs_dim=17, act_dim=6, hidden=[200, 200, 200, 200], K=7, elites=5, decays=[2.5e-5, 5e-5, 7.5e-5, 7.5e-5, 1e-4], T=600,
            B=256, epochs=1, seed=32, coef=0.01, lr=1e-3)
TRACE = dict(obs_dim=3, act_dim=2, hidden=[32, 32], K=3, elites=2, decays=[1e-4, 2.5e-4, 5e-4], n=500, B=64, seed=35, lr=3e-3,
             max_epochs=60)


def _load_file(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


class StubLogger:
    def __init__(self, model_dir):
        self.model_dir = model_dir
        self.rows, self._kv = [], {}

    def log(self, s):
        pass

    def logkv(self, k, v):
        self._kv[k] = float(v)

    def set_timestep(self, t):
        self._kv["timestep"] = t

    def dumpkvs(self, exclude=None):
        self.rows.append(dict(self._kv))
        self._kv = {}


def import_reference(root):
    for pkg in ("offlinerlkit", "offlinerlkit.nets", "offlinerlkit.modules", "offlinerlkit.dynamics", "offlinerlkit.utils"):
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    el = _load_file("offlinerlkit.nets.ensemble_linear", os.path.join(root, "offlinerlkit/nets/ensemble_linear.py"))
    sys.modules["offlinerlkit.nets"].EnsembleLinear = el.EnsembleLinear
    dm = _load_file("offlinerlkit.modules.dynamics_module", os.path.join(root, "offlinerlkit/modules/dynamics_module.py"))
    bd = _load_file("offlinerlkit.dynamics.base_dynamics", os.path.join(root, "offlinerlkit/dynamics/base_dynamics.py"))
    sys.modules["offlinerlkit.dynamics"].BaseDynamics = bd.BaseDynamics
    sc = _load_file("offlinerlkit.utils.scaler", os.path.join(root, "offlinerlkit/utils/scaler.py"))
    lg = types.ModuleType("offlinerlkit.utils.logger")
    lg.Logger = StubLogger
    sys.modules["offlinerlkit.utils.logger"] = lg
    ed = _load_file("offlinerlkit.dynamics.ensemble_dynamics", os.path.join(root, "offlinerlkit/dynamics/ensemble_dynamics.py"))
    return dm, sc, ed


def build(ref, c):
    dm, sc, ed = ref
    torch.manual_seed(c["seed"])
    model = dm.EnsembleDynamicsModel(c["obs_dim"], c["act_dim"], c["hidden"], c["K"], c["elites"], weight_decays=c["decays"])
    optim = torch.optim.Adam(model.parameters(), lr=c["lr"])
    dyn = ed.EnsembleDynamics(model, optim, sc.StandardScaler(), lambda o, a, n: np.zeros((len(o), 1), bool), penalty_coef=2.5)
    return model, dyn


def state(model):
    return {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}


def put_state(out, tag, st, full):
    for k, v in st.items():
        out[f"{tag}/{k}/digest"] = synth.digest(v)
        if full:
            out[f"{tag}/{k}/full"] = v


def synthetic(rng, n, od, ad):
    obs = rng.normal(size=(n, od)).astype(np.float32)
    act = rng.uniform(-1, 1, size=(n, ad)).astype(np.float32)
    A = rng.normal(size=(od + ad, od)) * 0.5
    nxt = (obs + 0.3 * np.tanh(np.concatenate([obs, act], 1) @ A) + 0.02 * rng.normal(size=(n, od))).astype(np.float32)
    rew = (np.sin(obs[:, :1]) + 0.5 * act[:, :1] ** 2 + 0.02 * rng.normal(size=(n, 1))).astype(np.float32)
    return {"observations": obs, "actions": act, "next_observations": nxt, "rewards": rew}


def gen_learn(ref, c, full, out):
    model, dyn = build(ref, c)
    rng = np.random.default_rng(c["seed"])
    od, ad, K, T = c["obs_dim"], c["act_dim"], c["K"], c["T"]
    D = od + 1
    x = rng.normal(size=(K, T, od + ad)).astype(np.float32)
    t = (0.5 * rng.normal(size=(K, T, D))).astype(np.float32)
    out["inputs"], out["targets"] = x, t
    put_state(out, "init", state(model), full)
    for e in range(c["epochs"]):
        loss = dyn.learn(x, t, c["B"], c["coef"])
        out[f"epoch{e}/loss"] = np.float64(loss)
        put_state(out, f"epoch{e}", state(model), full)
        out[f"epoch{e}/grad_max_logvar"] = model.max_logvar.grad.numpy().copy()
        out[f"epoch{e}/grad_min_logvar"] = model.min_logvar.grad.numpy().copy()
    return model, dyn


def gen_tiny(ref, path):
    c = TINY
    out = {}
    model, dyn = gen_learn(ref, c, True, out)
    rng = np.random.default_rng(c["seed"] + 1)
    od, ad, K, H, N = c["obs_dim"], c["act_dim"], c["K"], c["H"], c["N"]
    vx = rng.normal(size=(H, od + ad)).astype(np.float32)
    vt = (0.5 * rng.normal(size=(H, od + 1))).astype(np.float32)
    out["val_inputs"], out["val_targets"] = vx, vt
    out["val_loss"] = np.asarray(dyn.validate(vx, vt), np.float64)
    # step(): a fitted scaler, elites [2, 0], recorded draws
    fit = rng.normal(size=(300, od + ad)).astype(np.float32) * 2 + 0.5
    dyn.scaler.fit(fit)
    out["scaler_mu"], out["scaler_std"] = dyn.scaler.mu, dyn.scaler.std
    model.set_elites([2, 0])
    obs = rng.normal(size=(N, od)).astype(np.float32)
    act = rng.uniform(-1, 1, size=(N, ad)).astype(np.float32)
    out["step_obs"], out["step_act"] = obs, act
    put_state(out, "step_state", state(model), True)
    for mode in ("aleatoric", "pairwise-diff", "ensemble_std"):
        dyn._uncertainty_mode = mode
        np.random.seed(7)
        nxt, rew, term, info = dyn.step(obs, act)
        np.random.seed(7)
        noise = np.random.normal(size=(K, N, od + 1))
        idx = np.random.choice(np.array([2, 0]), size=N)
        out[f"step/{mode}/noise"], out[f"step/{mode}/model_idx"] = noise.astype(np.float32), idx
        out[f"step/{mode}/next_obs"], out[f"step/{mode}/reward"] = nxt, rew
        out[f"step/{mode}/raw_reward"], out[f"step/{mode}/penalty"] = info["raw_reward"], info["penalty"]
    # a reference-written checkpoint of this state (state_dict tensors + scaler) for the load test
    out["penalty_coef"] = np.float64(2.5)
    np.savez_compressed(path, **out)


def gen_mopo(ref, path):
    out = {}
    gen_learn(ref, MOPO, False, out)
    out.pop("inputs"); out.pop("targets")       # regenerated by the test from the seed (synthetic_learn_inputs)
    np.savez_compressed(path, **out)


def learn_inputs(c):
    """the inputs / targets gen_learn draws (the MOPO fixture does not store them)"""
    rng = np.random.default_rng(c["seed"])
    od, ad, K, T = c["obs_dim"], c["act_dim"], c["K"], c["T"]
    x = rng.normal(size=(K, T, od + ad)).astype(np.float32)
    t = (0.5 * rng.normal(size=(K, T, od + 1))).astype(np.float32)
    return x, t


def gen_trace(ref, path):
    c = TRACE
    model, dyn = build(ref, c)
    data = synthetic(np.random.default_rng(c["seed"]), c["n"], c["obs_dim"], c["act_dim"])
    torch.manual_seed(c["seed"] + 1)
    np.random.seed(c["seed"] + 2)
    # record the indices the reference draws by replaying its RNG calls
    torch_state, np_state = torch.get_rng_state(), np.random.get_state()
    with tempfile.TemporaryDirectory() as d:
        log = StubLogger(d)
        dyn.train(data, log, max_epochs=c["max_epochs"], batch_size=c["B"])
    elites = model.elites.detach().numpy().copy()
    epochs = len(log.rows)
    torch.set_rng_state(torch_state); np.random.set_state(np_state)
    n = c["n"]
    hs = min(int(n * 0.2), 1000)
    tr, ho = torch.utils.data.random_split(range(n), (n - hs, hs))
    boot = np.random.randint(n - hs, size=[c["K"], n - hs])
    shuf = [np.argsort(np.random.uniform(size=boot.shape), axis=-1) for _ in range(epochs)]
    out = {k: v for k, v in data.items()}
    out["train_idx"], out["holdout_idx"] = np.asarray(tr.indices), np.asarray(ho.indices)
    out["bootstrap"] = boot
    out["shuffle"] = np.stack(shuf)
    out["train_loss"] = np.array([r["loss/dynamics_train_loss"] for r in log.rows])
    out["holdout_loss"] = np.array([r["loss/dynamics_holdout_loss"] for r in log.rows])
    out["stop_epoch"] = np.int64(epochs)
    out["elites"] = elites
    out["seeds"] = np.array([c["seed"] + 1, c["seed"] + 2])
    np.savez_compressed(path, **out)
    return out


def check_trace_margins(path, member_losses):
    """every 1 % improvement decision and the elite order have a margin far above fp32 noise"""
    hist = [1e10] * member_losses.shape[1]
    worst = np.inf
    for e in range(member_losses.shape[0]):
        for i, v in enumerate(member_losses[e]):
            imp = (hist[i] - v) / hist[i]
            worst = min(worst, abs(imp - 0.01))
            if imp > 0.01:
                hist[i] = v
    s = np.sort(hist)
    gaps = np.diff(s) / s[1:]
    return worst, gaps.min() if gaps.size else np.inf


if __name__ == "__main__":
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("OFFLINERLKIT_REF", "")
    ref = import_reference(root)
    gen_tiny(ref, os.path.join(HERE, "dyn_tiny.npz"))
    gen_mopo(ref, os.path.join(HERE, "dyn_mopo.npz"))
    # the trace: per-member holdout losses for the margin check come from a second, instrumented run
    _, _, ed = ref
    rec = []
    orig = ed.EnsembleDynamics.validate

    def validate(self, x, t):
        v = orig(self, x, t)
        rec.append(np.asarray(v, np.float64))
        return v
    ed.EnsembleDynamics.validate = validate
    out = gen_trace(ref, os.path.join(HERE, "dyn_trace.npz"))
    ed.EnsembleDynamics.validate = orig
    ml = np.stack(rec)
    worst, gap = check_trace_margins(None, ml)
    print("trace: stop epoch", int(out["stop_epoch"]), "elites", out["elites"], "improvement margin", worst, "elite gap", gap)
    assert worst > 2e-3 and gap > 1e-3, (worst, gap)
    g = dict(np.load(os.path.join(HERE, "dyn_trace.npz")))
    g["member_holdout_loss"] = ml
    np.savez_compressed(os.path.join(HERE, "dyn_trace.npz"), **g)
    for f in ("dyn_tiny.npz", "dyn_mopo.npz", "dyn_trace.npz"):
        print(f, os.path.getsize(os.path.join(HERE, f)))
