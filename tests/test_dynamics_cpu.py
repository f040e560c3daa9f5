"""CPU: the dynamics ensemble's host side and its numpy restatement against fixtures from the reference (tests/golden/dyn_*.npz,
make_dyn_golden.py): the numpy oracle's learn / validate, train()'s control flow and RNG order with a numpy device stand-in, the
model's state_dict inventory and initialisation, and the dynamics entries of the C ABI."""
import os
import tempfile

import numpy as np
import pytest
import torch

import dyn_oracle as orc
import make_dyn_golden as mk

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _g(name):
    return np.load(os.path.join(GOLD, name))


def _state(g, tag):
    keys = sorted({k.split("/")[1] for k in g.files if k.startswith(tag + "/") and k.endswith("/full")})
    return {k: g[f"{tag}/{k}/full"].copy() for k in keys}


def _model(c):
    from offlinerlkit.modules import EnsembleDynamicsModel
    torch.manual_seed(c["seed"])
    return EnsembleDynamicsModel(c["obs_dim"], c["act_dim"], c["hidden"], c["K"], c["elites"], weight_decays=c["decays"])


def test_oracle_learn_tiny():
    g, c = _g("dyn_tiny.npz"), mk.TINY
    st = {k: v for k, v in _state(g, "init").items() if k != "elites"}
    opt = {}
    for e in range(c["epochs"]):
        loss, grads = orc.learn(st, opt, g["inputs"], g["targets"], c["B"], c["decays"], c["coef"], c["lr"])
        assert abs(loss - float(g[f"epoch{e}/loss"])) <= 2e-5 * abs(float(g[f"epoch{e}/loss"]))
        ref = _state(g, f"epoch{e}")
        for k in ("backbones.0.weight", "output_layer.bias", "max_logvar", "min_logvar"):
            assert np.abs(st[k] - ref[k]).max() <= 1e-5 + 1e-4 * np.abs(ref[k]).max(), (e, k)
        for k in ("max_logvar", "min_logvar"):
            assert np.allclose(grads[k], g[f"epoch{e}/grad_{k}"], rtol=1e-4, atol=1e-7), k


def test_oracle_validate_tiny():
    g = _g("dyn_tiny.npz")
    st = _state(g, f"epoch{mk.TINY['epochs'] - 1}")
    v = orc.validate(st, g["val_inputs"], g["val_targets"])
    assert np.abs(v - g["val_loss"]).max() <= 2e-5 * np.abs(g["val_loss"]).max()


def test_oracle_learn_mopo_shape():
    import synth
    g, c = _g("dyn_mopo.npz"), mk.MOPO
    m = _model(c)
    st = {k: v.detach().numpy().copy() for k, v in m.state_dict().items() if k != "elites"}
    for k, v in st.items():               # the constructor reproduces the reference's initial parameters
        assert np.allclose(synth.digest(v), g[f"init/{k}/digest"], rtol=1e-6, atol=1e-6), k
    x, t = mk.learn_inputs(c)
    loss, _ = orc.learn(st, {}, x, t, c["B"], c["decays"], c["coef"], c["lr"])
    assert abs(loss - float(g["epoch0/loss"])) <= 2e-5 * abs(float(g["epoch0/loss"]))
    for k, v in st.items():
        d, ref = synth.digest(v), g[f"epoch0/{k}/digest"]
        assert np.abs(d[2:] - ref[2:]).max() <= 1e-5 + 1e-4 * np.abs(ref[2:]).max(), k


def test_state_dict_inventory_and_init():
    g, c = _g("dyn_tiny.npz"), mk.TINY
    m = _model(c)
    sd = m.state_dict()
    ref = _state(g, "init")
    ref_keys = [k.split("/")[1] for k in g.files if k.startswith("init/") and k.endswith("/full")]
    assert list(sd.keys()) == ["max_logvar", "min_logvar", "elites"] + [k for k in sd.keys() if "." in k]
    assert set(sd.keys()) == set(ref_keys)
    for k, v in sd.items():
        assert tuple(v.shape) == ref[k].shape, k
        assert np.array_equal(v.numpy(), ref[k]), k


class _NumpyDyn:
    """device stand-in: orl_dyn_* restated with dyn_oracle on the host (run 0 only)"""

    def __init__(self, model, c):
        self.st = {k: v.detach().numpy().copy() for k, v in model.state_dict().items() if k != "elites"}
        self.saved = None
        self.opt, self.c = {}, c
        self.tensors = [(k, 0, v.shape) for k, v in self.st.items()]
        self.elites = np.arange(c["elites"])

    def load_data(self, x, t):
        self.x, self.t = x, t

    def set_scaler(self, r, mu, std):
        self.mu, self.std = mu, std

    def learn_epoch(self, rows, active):
        x = ((self.x[rows[0]] - self.mu) / self.std).astype(np.float32)
        loss, _ = orc.learn(self.st, self.opt, x, self.t[rows[0]], self.c["B"], self.c["decays"], 0.01, self.c["lr"])
        return np.array([loss], np.float32)

    def validate(self, hold):
        x = ((self.x[hold[0]] - self.mu) / self.std).astype(np.float32)
        return orc.validate(self.st, x, self.t[hold[0]])[None]

    def update_save(self, r, mask):
        pass

    def load_save(self, r):
        pass

    def set_elites(self, r, el):
        self.elites = np.asarray(el)

    def get_elites(self, r):
        return self.elites

    def sync(self):
        pass


def test_train_control_flow_matches_reference_trace():
    from offlinerlkit.dynamics import EnsembleDynamics
    from offlinerlkit.utils.scaler import StandardScaler
    g, c = _g("dyn_trace.npz"), mk.TRACE
    m = _model(c)
    optim = torch.optim.Adam(m.parameters(), lr=c["lr"])
    dyn = EnsembleDynamics(m, optim, StandardScaler(), lambda o, a, n: np.zeros((len(o), 1), bool))
    dyn._eng = _NumpyDyn(m, c)
    dyn._shape = (c["B"], 0.01)
    dyn._bind = lambda *a, **k: None
    dyn._sync_torch = lambda: None
    dyn.select_run = lambda r: None
    dyn.save = lambda p: None
    data = {k: g[k] for k in ("observations", "actions", "next_observations", "rewards")}
    torch.manual_seed(int(g["seeds"][0]))
    np.random.seed(int(g["seeds"][1]))
    logs = mk.StubLogger(tempfile.mkdtemp())
    dyn.train(data, logs, max_epochs=c["max_epochs"], batch_size=c["B"])
    tr = dyn.train_trace
    assert np.array_equal(tr["train_idx"][0], g["train_idx"]) and np.array_equal(tr["holdout_idx"][0], g["holdout_idx"])
    assert np.array_equal(tr["data_idxes"][0][0], g["bootstrap"])
    boot = g["bootstrap"]
    for e in range(1, len(tr["data_idxes"])):       # each epoch's order = the previous one shuffled by the reference's draw
        boot = boot[np.arange(boot.shape[0])[:, None], g["shuffle"][e - 1]]
        assert np.array_equal(tr["data_idxes"][e][0], boot), e
    assert tr["stop_epoch"][0] == int(g["stop_epoch"])
    assert list(tr["elites"][0]) == list(g["elites"])
    tl = np.array([r["loss/dynamics_train_loss"] for r in logs.rows])
    assert np.allclose(tl, g["train_loss"], rtol=1e-4)


def test_dynamics_abi_symbols():
    from offlinerlkit import _engine
    lib = _engine.load_library()
    dyn = [s for s in _engine.ABI_SYMBOLS if s.startswith("orl_dyn_")]
    assert len(dyn) == 24 and "orl_dyn_debug_read" in dyn
    for s in dyn:
        assert hasattr(lib, s), s
    cfg = _engine.default_dyn_config()
    assert cfg.num_ensemble == 7 and cfg.num_elites == 5 and list(cfg.hidden) == [200] * 4 and cfg.batch_size == 256
    assert np.allclose(list(cfg.weight_decay), [2.5e-5, 5e-5, 7.5e-5, 7.5e-5, 1e-4])
    # parameter block: every tensor of the reference's state_dict except elites, 16-B aligned
    c = _engine.default_dyn_config(obs_dim=3, act_dim=2, hidden=[32, 32], num_ensemble=3, num_elites=2)
    n = sum(((int(np.prod(v.shape)) + 3) // 4) * 4 for k, v in _model(mk.TINY).state_dict().items() if k != "elites")
    assert lib.orl_dyn_config_floats(c) == n


def test_dynamics_create_refuses_without_gpu_or_precision():
    from offlinerlkit import _engine
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="HIP device|precision"):
        _engine.Dynamics(_engine.default_dyn_config())
