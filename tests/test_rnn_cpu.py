"""CPU: RNNDynamics without a GPU -- the numpy oracle (tests/rnn_oracle.py) against the reference fixtures of
tests/golden/make_rnn_golden.py, the project's torch ``RNNModel`` against the same fixtures, the epoch order of ``train``, and the refusals.

Bars: pred and taps 1e-4 of scale, loss 1e-4 (rel_err with floor 1e-2), the float32 oracle's gradients 4 x the fixture's
``grad_f32_vs_f64``, the float64 oracle's gradients 1e-10 of each tensor's scale."""
import numpy as np
import pytest
import torch

import rnn_cases as rc
import rnn_oracle as orc
from diffusion_oracle import grad_distance
from helpers import load_golden, rel_err, scale_err

SINGLE = ["rnn_tiny", "rnn_t1", "rnn_odd", "rnn_default"]


def fixture_grads(g, c, G):
    """(the fixture's float64 gradients, ``G`` cut to the same entries): whole tensors, or rnn_default's seeded entries"""
    want = {k[len("grad64/"):]: g[k] for k in g.files if k.startswith("grad64/")}
    if c["name"] != "rnn_default":
        return want, {k: np.asarray(G[k]) for k in want}
    return want, {k: np.asarray(G[k]).ravel()[rc.digest_positions(c, k, np.asarray(G[k]).size)] for k in want}


def grad_ratio(g, c, G):
    """the worst per-tensor max |G - g64| / scale(g64) over the bar 4 x grad_f32_vs_f64; structurally zero tensors must stay inside
    4 x the recorded noise"""
    want, got = fixture_grads(g, c, G)
    worst = 0.0
    for k, v in want.items():
        scale = float(g[f"gscale/{k}"]) if c["name"] == "rnn_default" else float(np.abs(v).max())
        if scale == 0.0:
            assert float(np.abs(got[k]).max()) <= 4 * float(g["grad_zero_noise"]), k
            continue
        worst = max(worst, float(np.abs(got[k].astype(np.float64) - v).max() / scale))
    return worst / (4 * float(g["grad_f32_vs_f64"]))


def drop_of(g, c):
    return rc.unpack_masks(g["drop_masks"], c, c["B"] * c["T"]) if c["p"] > 0 else None


@pytest.mark.parametrize("name", SINGLE)
def test_oracle_reproduces_the_fixture(name):
    c, g = rc.CASES[name], load_golden(name)
    P = rc.make_params(c)
    x, tg, mk = rc.make_data(c)
    drop = drop_of(g, c)
    loss, pred, G, cache = orc.loss_and_grads(P, c, x, tg, mk, drop, np.float32)
    want_pred = g["pred"]
    got_pred = pred[:, list(rc.PRED_STEPS)] if name == "rnn_default" else pred
    assert scale_err(got_pred, want_pred) < 1e-4
    assert rel_err(loss, g["loss"], floor=1e-2) < 1e-4
    for k in g.files:
        if k.startswith("tap/"):
            assert scale_err(cache["taps"][k[4:]], g[k]) < 1e-4, k
    ratio = grad_ratio(g, c, G)
    print(f"{name}: float32 oracle gradients at {ratio:.2f} of the bar (grad_f32_vs_f64 = {float(g['grad_f32_vs_f64']):.3e})")
    assert ratio <= 1.0
    loss64, _, G64, _ = orc.loss_and_grads(P, c, x, tg, mk, drop, np.float64)
    want, got = fixture_grads(g, c, G64)
    for k, v in want.items():
        scale = float(g[f"gscale/{k}"]) if name == "rnn_default" else float(np.abs(v).max())
        assert float(np.abs(got[k] - v).max()) <= 1e-10 * scale, k
    assert abs(loss64 - float(g["loss64"])) < 1e-12


def test_t1_has_no_recurrent_weight_gradient():
    g = load_golden("rnn_t1")
    for l in range(rc.CASES["rnn_t1"]["L"]):
        assert not g[f"grad64/rnn_layer.weight_hh_l{l}"].any()
        assert g[f"grad64/rnn_layer.bias_hh_l{l}"].any()


def test_odd_masks_have_zero_entries_and_a_zero_row():
    _, _, mk = rc.make_data(rc.CASES["rnn_odd"])
    assert not mk[11].any() and (mk == 0).sum() > mk.shape[1] and mk.any(axis=1).sum() == mk.shape[0] - 1


def test_oracle_trajectory_stays_inside_the_twin_envelope():
    import long_horizon as lh
    c, g = rc.CASES["rnn_traj"], load_golden("rnn_traj")
    losses, fin, (m1, v1) = orc.train(rc.make_params(c), c, rc.make_data(c), rc.make_steps(c), c["lr"])
    ref, twin = g["losses"][:, None], g["losses_twin"][:, None]
    d = np.maximum.accumulate(lh.deviation(losses[:, None], ref))
    env = lh.envelope(ref, [twin])
    assert d[-1] <= lh.K_ENVELOPE * env[-1] and d[-1] < 1e-4
    for k in fin:
        assert scale_err(m1[k], g[f"m1/{k}"]) < 1e-5 and scale_err(v1[k], g[f"v1/{k}"]) < 1e-5


def _model(c, P=None, **over):
    from offlinerlkit.nets import RNNModel
    m = RNNModel(c["input_dim"], c["output_dim"], hidden_dims=list(c["hidden"]), rnn_num_layers=c["L"], dropout_rate=c["p"], **over)
    if P is not None:
        m.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()}, strict=True)
    return m


def test_module_has_the_reference_signature_keys_and_shapes():
    import inspect
    from offlinerlkit.nets import RNNModel, ResBlock, Swish, soft_clamp  # noqa: F401
    sig = inspect.signature(RNNModel.__init__)
    assert list(sig.parameters) == ["self", "input_dim", "output_dim", "hidden_dims", "rnn_num_layers", "dropout_rate", "device"]
    assert list(sig.parameters["hidden_dims"].default) == [200] * 4 and sig.parameters["rnn_num_layers"].default == 3
    assert sig.parameters["dropout_rate"].default == 0.1 and sig.parameters["device"].default == "cpu"
    assert list(inspect.signature(RNNModel.forward).parameters) == ["self", "input", "h_state"]
    for name in rc.CASES:
        c = rc.CASES[name]
        sd = _model(c).state_dict()
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == rc.shapes(c)
    g = load_golden("rnn_trace")
    assert [str(k) for k in g["state_dict_keys"]] == [k for k, _ in rc.shapes(rc.CASES["rnn_trace"])]


@pytest.mark.parametrize("name", ["rnn_tiny", "rnn_t1"])
def test_module_forward_matches_the_reference_in_eval_mode(name):
    c, g = rc.CASES[name], load_golden(name)
    m = _model(c, rc.make_params(c)).eval()
    x, _, _ = rc.make_data(c)
    with torch.no_grad():
        pred, h = m(x)
    assert pred.shape == (c["B"], c["T"], c["output_dim"]) and h.shape == (c["L"], c["B"], c["H"])
    assert scale_err(pred.numpy(), g["pred"]) < 1e-5


def test_module_loads_the_trained_reference_tensors_and_steps_like_it():
    c, g = rc.CASES["rnn_trace"], load_golden("rnn_trace")
    m = _model(c)
    m.load_state_dict({k[len("final/"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("final/")}, strict=True)
    m.eval()
    obss, actions, mu, std = rc.make_windows(c)
    with torch.no_grad():
        pred, _ = m((np.concatenate([obss, actions], -1) - mu) / std)
    last = pred[:, -1].numpy()
    nxt = last[:, :-1] + obss[:, -1]
    assert scale_err(nxt, g["next_obss"]) < 1e-5 and scale_err(last[:, -1:], g["rewards"]) < 1e-5
    assert np.array_equal(rc.terminal_fn(obss[:, -1], actions[:, -1], nxt), g["terminals"])


def test_module_dropout_follows_train_and_eval():
    c = rc.CASES["rnn_odd"]
    m = _model(c, rc.make_params(c))
    x, _, _ = rc.make_data(c)
    with torch.no_grad():
        m.eval()
        a, b = m(x)[0], m(x)[0]
        m.train()
        torch.manual_seed(0)
        d = m(x)[0]
    assert torch.equal(a, b) and not torch.equal(a, d)


def test_epoch_order_reproduces_the_reference_loader():
    from offlinerlkit.dynamics import rnn_epoch_order
    c, g = rc.CASES["rnn_trace"], load_golden("rnn_trace")
    torch.manual_seed(c["torch_seed"])
    for want in g["orders"]:
        got = rnn_epoch_order(c["n"])
        assert got.dtype == np.int64 and np.array_equal(got, want)


def test_epoch_order_equals_a_live_loader_and_takes_a_generator():
    from torch.utils.data import DataLoader
    from offlinerlkit.dynamics import rnn_epoch_order
    torch.manual_seed(77)
    loader = DataLoader(list(range(13)), shuffle=True, batch_size=5)
    want = [np.concatenate([b.numpy() for b in loader]) for _ in range(2)]
    torch.manual_seed(77)
    assert all(np.array_equal(rnn_epoch_order(13), w) for w in want)
    g1, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    before = torch.get_rng_state()
    assert np.array_equal(rnn_epoch_order(9, g1), rnn_epoch_order(9, g2))
    assert torch.equal(torch.get_rng_state(), before)


def _dynamics(model, optim=None, **kw):
    from offlinerlkit.dynamics import RNNDynamics
    from offlinerlkit.utils.scaler import StandardScaler
    optim = optim if optim is not None else torch.optim.Adam(model.parameters(), lr=1e-3, **kw)
    return RNNDynamics(model, optim, StandardScaler(np.zeros((1, 5), np.float32), np.ones((1, 5), np.float32)), rc.terminal_fn)


def test_exports():
    import offlinerlkit.dynamics as dyn
    assert {"BaseDynamics", "EnsembleDynamics", "RNNDynamics"} <= set(dyn.__all__)
    assert issubclass(dyn.RNNDynamics, dyn.BaseDynamics)


def test_dynamics_refusals():
    from offlinerlkit.nets import MLP, RNNModel
    ok = RNNModel(5, 4, [24, 24], 1, 0.0)
    _dynamics(ok)
    with pytest.raises(NotImplementedError, match="equal hidden_dims"):
        _dynamics(RNNModel(5, 4, [24, 32], 1, 0.0))
    with pytest.raises(NotImplementedError, match="multiple of 4"):
        _dynamics(RNNModel(5, 4, [30, 30], 1, 0.0))
    with pytest.raises(NotImplementedError, match="multiple of 4"):
        _dynamics(RNNModel(5, 4, [516, 516], 1, 0.0))
    with pytest.raises(NotImplementedError, match="GRU layers"):
        _dynamics(RNNModel(5, 4, [24, 24], 5, 0.0))
    with pytest.raises(NotImplementedError, match="hidden_dims"):
        _dynamics(RNNModel(5, 4, [24] * 6, 1, 0.0))
    with pytest.raises(NotImplementedError, match="hidden_dims"):
        _dynamics(RNNModel(5, 4, [24], 1, 0.0))
    with pytest.raises(NotImplementedError, match="RNNModel"):
        _dynamics(MLP(5, [24, 24], 4), optim=torch.optim.Adam(ok.parameters()))
    with pytest.raises(NotImplementedError, match="Adam only"):
        _dynamics(ok, optim=torch.optim.AdamW(ok.parameters()))
    with pytest.raises(NotImplementedError, match="Adam only"):
        _dynamics(ok, optim=torch.optim.SGD(ok.parameters(), lr=0.1))
    with pytest.raises(NotImplementedError, match="weight_decay"):
        _dynamics(ok, weight_decay=1e-4)
    with pytest.raises(NotImplementedError, match="amsgrad"):
        _dynamics(ok, amsgrad=True)
    drop = _dynamics(RNNModel(5, 4, [24, 24], 1, 0.1))
    drop.model.eval()                                     # the engine's training step always applies the dropout
    with pytest.raises(NotImplementedError, match="eval mode"):
        drop.learn(rc.make_data(rc.CASES["rnn_tiny"]))


def test_engine_config_refusals():
    """orl_rnn_config_floats applies orl_rnn_create's refusals and needs no device"""
    from offlinerlkit import _engine
    assert _engine.rnn_config_floats(_engine.default_rnn_config()) > 0
    c = rc.CASES["rnn_tiny"]
    want = sum(-(-int(np.prod(s)) // 4) * 4 for _, s in rc.shapes(c))             # every tensor on a 16-byte boundary
    assert _engine.rnn_config_floats(_engine.default_rnn_config(input_dim=5, output_dim=4, hidden=[24, 24], rnn_num_layers=1)) == want
    for over, word in ((dict(hidden=[24, 32]), "equal"), (dict(hidden=[30, 30]), "multiple of 4"), (dict(hidden=[4, 4]), "multiple of 4"),
                       (dict(hidden=[516, 516]), "multiple of 4"), (dict(hidden=[24]), "hidden_dims"), (dict(rnn_num_layers=0), "rnn_num_layers"),
                       (dict(rnn_num_layers=5), "rnn_num_layers"), (dict(dropout_rate=1.0), "dropout_rate"), (dict(dropout_rate=-0.1), "dropout_rate"),
                       (dict(input_dim=0), "input_dim"), (dict(output_dim=0), "output_dim"), (dict(n_runs=2), "one run"),
                       (dict(precision=1), "precision 0"), (dict(batch_size=0), "batch_size"), (dict(max_seq_len=0), "max_seq_len")):
        with pytest.raises(RuntimeError, match=word):
            _engine.rnn_config_floats(_engine.default_rnn_config(**over))
    with pytest.raises(NotImplementedError, match="hidden_dims"):
        _engine.default_rnn_config(hidden=[24] * 6)
    with pytest.raises(KeyError):
        _engine.default_rnn_config(no_such_field=1)


def test_dynamics_without_a_device_raises(monkeypatch):
    from offlinerlkit.nets import RNNModel
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    dyn = _dynamics(RNNModel(5, 4, [24, 24], 1, 0.0))
    x, tg, mk = rc.make_data(rc.CASES["rnn_tiny"])
    with pytest.raises(RuntimeError, match="no HIP device"):
        dyn.learn((x, tg, mk))
    with pytest.raises(RuntimeError, match="no HIP device"):
        dyn.step(x[:, :, :3], x[:, :, 3:])
