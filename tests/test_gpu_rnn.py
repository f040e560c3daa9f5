"""GPU: RNNDynamics on the engine (orl_rnn_*) against the reference fixtures of tests/golden/make_rnn_golden.py, the numpy oracle in
float64 on the engine's own operands, and the ``RNNDynamics`` class on top of it.

Bars: pred and the taps 1e-4 of scale, loss 1e-4 (rel_err with floor 1e-2, the project's gate); gradients per tensor 4 x the distance
the reference's fp32 autograd shows from float64 autograd on the same batch (``grad_f32_vs_f64``, stored in the fixture; for the shapes
outside the fixtures measured here with the project's torch module, which tests/test_rnn_cpu.py holds to the reference), in the norm
of diffusion_oracle.grad_distance -- the 4 covers another summation order; the 20-step trajectory and its final parameters K = 4 x the
reference's own one-ulp twin (tests/long_horizon.py's rule)."""
import numpy as np
import pytest
import torch
from scipy import stats

import long_horizon as lh
import rnn_cases as rc
import rnn_oracle as orc
from diffusion_oracle import grad_distance
from helpers import load_golden, rel_err, scale_err
from test_rnn_cpu import drop_of, grad_ratio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make_engine(c, B=None, T=None, seed=0, P=None, p=None):
    from offlinerlkit import _engine
    cfg = _engine.default_rnn_config(input_dim=c["input_dim"], output_dim=c["output_dim"], hidden=c["hidden"], rnn_num_layers=c["L"],
                                     dropout_rate=c["p"] if p is None else p, batch_size=B or c["B"], max_seq_len=T or c["T"],
                                     lr=c.get("lr", 1e-3), seed=seed)
    eng = _engine.RnnDynamicsEngine(cfg)
    P = P if P is not None else rc.make_params(c)
    eng.set_params(P)
    return eng, P


def grads_of(eng):
    from offlinerlkit import _engine
    return _engine._unflatten(eng.tensors(), eng.debug_grads())


def tap(eng, name, cols):
    return eng.debug_read(name).reshape(-1, cols)


# ---- 1. one step against every single-step fixture -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rnn_tiny", "rnn_t1", "rnn_odd", "rnn_default"])
def test_step_matches_the_reference_fixture(name):
    c, g = rc.CASES[name], load_golden(name)
    x, tg, mk = rc.make_data(c)
    eng, P = make_engine(c)
    try:
        assert [(k, s) for k, _, s in eng.tensors()] == rc.shapes(c) and all(off % 4 == 0 for _, off, _ in eng.tensors())
        eng.load_data(x, tg, mk)
        loss = eng.step(np.arange(c["B"]), drop_of(g, c))
        pred = tap(eng, "pred", c["output_dim"]).reshape(c["B"], c["T"], -1)
        got = pred[:, list(rc.PRED_STEPS)] if name == "rnn_default" else pred
        e_pred, e_loss = scale_err(got, g["pred"]), rel_err(loss, g["loss"], floor=1e-2)
        e_taps = {k[4:]: scale_err(tap(eng, k[4:], c["H"]), g[k]) for k in g.files if k.startswith("tap/")}
        ratio = grad_ratio(g, c, grads_of(eng))
        print(f"{name}: pred {e_pred:.2e} loss {e_loss:.2e} taps {max(e_taps.values(), default=0.0):.2e}; gradients at {ratio:.2f} of the bar "
              f"(4 x {float(g['grad_f32_vs_f64']):.3e})")
        assert e_pred < 1e-4 and e_loss < 1e-4 and abs(float(eng.debug_read("loss")[0]) - loss) == 0
        assert all(v < 1e-4 for v in e_taps.values()), e_taps
        assert ratio <= 1.0
        assert eng.step_count == 1 and not np.array_equal(eng.get(eng.PARAMS), _flat(eng, P))
    finally:
        eng.close()


def _flat(eng, P):
    from offlinerlkit import _engine
    return _engine._flatten(eng.tensors(), P, eng.floats)


@pytest.mark.parametrize("name", ["rnn_tiny", "rnn_t1", "rnn_odd"])
def test_forward_matches_the_fixture_and_the_oracle(name):
    """eval mode: the fixture's pred where the case has no dropout, the oracle's eval forward (every layer's tap) everywhere"""
    c, g = rc.CASES[name], load_golden(name)
    x, _, _ = rc.make_data(c)
    eng, P = make_engine(c)
    try:
        last, every = eng.forward(x, want_all=True)
        want, cache = orc.forward(P, c, x, None, np.float64)
        assert np.array_equal(last, every[:, -1]) and scale_err(every, want) < 1e-4
        if c["p"] == 0:
            assert scale_err(every, g["pred"]) < 1e-4
        for k, v in cache["taps"].items():
            assert scale_err(tap(eng, k, c["H"]), v) < 1e-4, k
        dlast, devery = eng.forward(torch.as_tensor(x, device=DEV), want_all=True)
        assert np.array_equal(dlast.cpu().numpy(), last) and np.array_equal(devery.cpu().numpy(), every)
        assert np.array_equal(eng.forward(x[:2, :1]), eng.forward(x[:2, :1], want_all=True)[1][:, 0])      # fewer rows and steps than before
        assert scale_err(eng.forward(x[:2, :1]), orc.forward(P, c, x[:2, :1], None, np.float64)[0][:, 0]) < 1e-4
    finally:
        eng.close()


# ---- 2. the trajectory ---------------------------------------------------------------------------------------------------------------------
def _param_dev(x, ref):
    return max(float((np.abs(x[k].astype(np.float64) - ref[k]) / np.maximum(np.abs(ref[k]), 1e-2 * np.abs(ref[k]).max())).max()) for k in ref)


def test_trajectory_stays_inside_the_twin_envelope():
    c, g = rc.CASES["rnn_traj"], load_golden("rnn_traj")
    steps = rc.make_steps(c)
    assert {len(s) for s in steps} == {16, 8}
    eng, P = make_engine(c)
    try:
        eng.load_data(*rc.make_data(c))
        losses = []
        for k, idx in enumerate(steps):
            losses.append(eng.step(idx))
            if k == 0:
                from offlinerlkit import _engine
                m1, v1 = (_engine._unflatten(eng.tensors(), eng.get(w)) for w in (eng.EXP_AVG, eng.EXP_AVG_SQ))
                e_m = max(scale_err(m1[n], g[f"m1/{n}"]) for n in P)
                e_v = max(scale_err(v1[n], g[f"v1/{n}"]) for n in P)
                print(f"Adam moments after step 1: exp_avg {e_m:.2e} exp_avg_sq {e_v:.2e}")
                assert e_m < 1e-6 and e_v < 1e-6
        losses = np.array(losses, np.float64)
        ref, twin = g["losses"][:, None], g["losses_twin"][:, None]
        d = np.maximum.accumulate(lh.deviation(losses[:, None], ref))
        env = lh.envelope(ref, [twin])
        for T in (5, 10, c["steps"]):
            print(f"loss deviation by step {T}: {d[T - 1]:.2e} (twin envelope {env[T - 1]:.2e})")
            assert d[T - 1] <= lh.K_ENVELOPE * env[T - 1], (T, d[T - 1], env[T - 1])
        assert d[-1] < 1e-4
        got = eng.get_params()
        want = {k[len("final/"):]: g[k] for k in g.files if k.startswith("final/")}
        tw = {k[len("final_twin/"):]: g[k] for k in g.files if k.startswith("final_twin/")}
        dev, env_p = _param_dev(got, want), _param_dev(tw, want)
        print(f"final parameters: deviation {dev:.2e} (twin {env_p:.2e})")
        assert dev <= lh.K_ENVELOPE * env_p, (dev, env_p)
    finally:
        eng.close()


# ---- 3. float64 backward error at shapes outside the fixtures ------------------------------------------------------------------------------
# (H, B, T, L, in, out, blocks, p): H in {8, 72, 512}, B in {1, 16, 17}, T in {1, 2, 9}, L in {1, 4}, in = 1, out = 1; H = 512 takes the
# scan backward past 64 KB of LDS and 8 unit groups, B = 17 a second row block of one row, H = 8 half a unit tile
SHAPES = [(8, 1, 1, 1, 1, 1, 2, 0.0), (8, 17, 9, 4, 3, 2, 2, 0.0), (72, 16, 2, 1, 1, 3, 3, 0.0), (72, 17, 9, 4, 6, 1, 2, 0.25),
          (512, 16, 2, 1, 5, 4, 2, 0.0), (512, 17, 9, 1, 4, 3, 2, 0.0), (72, 1, 9, 4, 2, 2, 5, 0.0)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "H{}_B{}_T{}_L{}_in{}_out{}_n{}_p{}".format(*s))
def test_float64_backward_error_outside_the_fixtures(shape):
    H, B, T, L, nin, nout, nh, p = shape
    c = dict(name="shape", input_dim=nin, output_dim=nout, hidden=[H] * nh, H=H, L=L, B=B, T=T, p=p, n=B, seed=900 + H + B + T, lengths=T > 1)
    P = rc.make_params(c)
    x, tg, mk = rc.make_data(c)
    drop = (np.random.RandomState(3).uniform(size=(nh, B * T, H)) >= p).astype(np.float32) if p > 0 else None
    loss64, pred64, G64, cache = orc.loss_and_grads(P, c, x, tg, mk, drop, np.float64)
    # the bar: fp32 autograd of the project's torch module against the float64 oracle on the same batch
    from offlinerlkit.nets import RNNModel
    m = RNNModel(nin, nout, [H] * nh, L, 0.0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
    if drop is not None:
        class Forced(torch.nn.Module):
            def __init__(self, keep):
                super().__init__()
                self.keep = torch.from_numpy(keep)

            def forward(self, v):
                return v * self.keep / (1.0 - p)
        for s, b in enumerate([m.input_layer] + list(m.backbones)):
            b.dropout = Forced(drop[s])
    pr, _ = m(torch.from_numpy(x))
    (((pr - torch.from_numpy(tg)) ** 2).mean(-1) * torch.from_numpy(mk)).mean().backward()
    g32 = {k: v.grad.numpy() for k, v in m.named_parameters()}
    dist, noise = grad_distance(g32, G64)
    eng, _ = make_engine(c, P=P)
    try:
        eng.load_data(x, tg, mk)
        loss = eng.step(np.arange(B), drop)
        e_pred = scale_err(tap(eng, "pred", nout), pred64.reshape(-1, nout))
        e_loss = rel_err(loss, loss64, floor=1e-2)
        e_taps = max(scale_err(tap(eng, k, H), v) for k, v in cache["taps"].items())
        got, n_got = grad_distance(grads_of(eng), G64)
        print(f"{shape}: pred {e_pred:.2e} loss {e_loss:.2e} taps {e_taps:.2e}; gradients {got:.3e} against 4 x {dist:.3e} "
              f"({got / (4 * dist):.2f} of the bar); zero tensors {n_got:.1e} (fp32 autograd {noise:.1e})")
        assert e_pred < 1e-4 and e_loss < 1e-4 and e_taps < 1e-4
        assert got <= 4 * dist and n_got <= 4 * noise
    finally:
        eng.close()


# ---- 4. no stale rows or time steps; bitwise repeatability -----------------------------------------------------------------------------------
def _state(eng):
    return [eng.get(w) for w in (eng.PARAMS, eng.EXP_AVG, eng.EXP_AVG_SQ)]


def test_short_batch_after_a_full_one_reads_nothing_stale():
    c = rc.CASES["rnn_traj"]
    data = rc.make_data(c)
    a, P = make_engine(c)
    b, _ = make_engine(c)
    try:
        a.load_data(*data)
        b.load_data(*data)
        a.step(np.arange(16))
        for w, v in zip((b.PARAMS, b.EXP_AVG, b.EXP_AVG_SQ), _state(a)):
            b.set(w, v)
        b.step_count = 1
        short = np.array([33, 2, 17], np.int64)
        la, lb = a.step(short), b.step(short)
        assert la == lb and np.array_equal(a.debug_grads(), b.debug_grads())
        assert all(np.array_equal(u, v) for u, v in zip(_state(a), _state(b)))
        assert np.array_equal(a.debug_read("pred"), b.debug_read("pred")) and a.debug_read("pred").size == 3 * c["T"] * c["output_dim"]
        # fewer time steps after more: a forward of 2 steps after one of 5
        x = data[0]
        a.forward(x[:16])
        assert np.array_equal(a.forward(x[:3, :2]), b.forward(x[:3, :2]))
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("name", ["rnn_odd", "rnn_traj"])
def test_identical_steps_give_identical_bits(name):
    c = rc.CASES[name]
    data = rc.make_data(c)
    a, _ = make_engine(c, seed=4)
    b, _ = make_engine(c, seed=4)
    try:
        out = []
        for e in (a, b):
            e.load_data(*data)
            idx = np.arange(c["B"])
            out.append(([e.step(idx), e.step(idx[::-1].copy())], e.debug_grads(), _state(e)))
        assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1])
        assert all(np.array_equal(u, v) for u, v in zip(out[0][2], out[1][2]))
    finally:
        a.close(); b.close()


def test_epoch_equals_its_steps():
    c = rc.CASES["rnn_traj"]
    order = np.random.RandomState(5).permutation(c["n"]).astype(np.int64)
    a, P = make_engine(c)
    b, _ = make_engine(c)
    try:
        a.load_data(*rc.make_data(c))
        b.load_data(*rc.make_data(c))
        la = np.concatenate([a.learn_epoch(order), a.learn_epoch(torch.as_tensor(order[::-1].copy(), device=DEV))])
        lb = [b.step(o[s:s + c["B"]]) for o in (order, order[::-1]) for s in range(0, c["n"], c["B"])]
        assert la.shape == (6,) and np.array_equal(la, np.array(lb, np.float32)) and a.step_count == b.step_count == 6
        assert all(np.array_equal(u, v) for u, v in zip(_state(a), _state(b)))
    finally:
        a.close(); b.close()


# ---- 5. the device dropout -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_philox_dropout(p):
    """4096 x 40 elements per mask: the keep rate inside the two-sided binomial interval at 1e-6, masks differ between step counts and
    between dropouts, the same seed and step count reproduce them, kept activations carry 1 / (1 - p)"""
    c = dict(name="drop", input_dim=3, output_dim=2, hidden=[40, 40], H=40, L=1, B=256, T=16, p=p, n=256, seed=77, lengths=False)
    data = rc.make_data(c)
    n = 4096 * 40
    lo, hi = stats.binom.ppf(5e-7, n, 1 - p), stats.binom.ppf(1 - 5e-7, n, 1 - p)
    a, _ = make_engine(c, seed=12)
    b, _ = make_engine(c, seed=12)
    d, _ = make_engine(c, seed=13)
    try:
        for e in (a, b, d):
            e.load_data(*data)
        idx = np.arange(256)
        a.step(idx)
        m0, m1 = a.debug_read("mask.0"), a.debug_read("mask.1")
        assert m0.size == n and set(np.unique(m0)) == {0.0, 1.0}
        for m in (m0, m1):
            print(f"p = {p}: kept {int(m.sum())} of {n} (interval {lo:.0f} .. {hi:.0f})")
            assert lo <= m.sum() <= hi
        assert not np.array_equal(m0, m1)
        act, dropped = a.debug_read("act.0"), a.debug_read("drop.0")
        assert np.allclose(dropped, act * m0 / (1 - p), rtol=1e-6, atol=0) and (dropped[m0 == 0] == 0).all()
        res = a.debug_read("merge")                               # the residual block adds its input to the dropped activation
        assert np.allclose(a.debug_read("drop.1"), res + a.debug_read("act.1") * m1 / (1 - p), rtol=1e-5, atol=1e-6)
        b.step(idx)
        assert np.array_equal(b.debug_read("mask.0"), m0) and np.array_equal(b.debug_read("mask.1"), m1)
        d.step(idx)
        assert not np.array_equal(d.debug_read("mask.0"), m0)     # another seed
        a.step(idx)
        assert not np.array_equal(a.debug_read("mask.0"), m0)     # another step count
        b.step_count = 0
        b.step(idx)
        assert np.array_equal(b.debug_read("mask.0"), m0)
        with pytest.raises(RuntimeError, match="no dropout mask"):
            a.forward(data[0][:4])
            a.debug_read("mask.0")
    finally:
        a.close(); b.close(); d.close()


def test_engine_refusals():
    from offlinerlkit import _engine
    with pytest.raises(RuntimeError, match="equal"):
        _engine.RnnDynamicsEngine(_engine.default_rnn_config(hidden=[24, 32]))
    c = rc.CASES["rnn_tiny"]
    eng, _ = make_engine(c)
    try:
        x, tg, mk = rc.make_data(c)
        with pytest.raises(RuntimeError, match="no data loaded"):
            eng.step(np.arange(2))
        with pytest.raises(RuntimeError, match="max_seq_len"):
            eng.load_data(np.zeros((2, c["T"] + 1, 5), np.float32), np.zeros((2, c["T"] + 1, 4), np.float32), np.ones((2, c["T"] + 1), np.float32))
        eng.load_data(x, tg, mk)
        with pytest.raises(RuntimeError, match="row index out of range"):
            eng.step(np.array([c["n"]], np.int64))
        with pytest.raises(RuntimeError, match="batch_size"):
            eng.step(np.zeros(c["B"] + 1, np.int64))
        with pytest.raises(RuntimeError, match="max_seq_len"):
            eng.forward(np.zeros((1, c["T"] + 1, 5), np.float32))
        with pytest.raises(RuntimeError, match="unknown tap"):
            eng.debug_read("gru.7")
        assert eng.step_count == 0
    finally:
        eng.close()


def test_step_profile_reports_its_phases():
    c = rc.CASES["rnn_traj"]
    eng, _ = make_engine(c)
    try:
        eng.load_data(*rc.make_data(c))
        eng.step(np.arange(16))
        with pytest.raises(RuntimeError, match="no timed step"):
            eng.profile_read()
        eng.profile(True)
        eng.step(np.arange(16))
        ms = eng.profile_read()
        assert set(ms) == {"step", "forward", "forward_scan", "backward", "backward_scan", "adam"} and all(v > 0 for v in ms.values())
        assert ms["forward_scan"] < ms["forward"] and ms["backward_scan"] < ms["backward"]
        assert ms["forward"] + ms["backward"] + ms["adam"] <= ms["step"] * 1.001
        eng.profile(False)
        eng.step(np.arange(16))
        with pytest.raises(RuntimeError, match="no timed step"):
            eng.profile_read()
    finally:
        eng.close()


# ---- 6. the RNNDynamics class ------------------------------------------------------------------------------------------------------------------
class _Logger:
    def __init__(self, model_dir):
        self.model_dir, self.rows, self._kv, self.excluded = str(model_dir), [], {}, None

    def logkv_mean(self, k, v):
        self._kv.setdefault(k, []).append(float(v))

    def set_timestep(self, t):
        self._t = t

    def dumpkvs(self, exclude=None):
        self.excluded = exclude
        row = {k: float(np.mean(v)) for k, v in self._kv.items()}
        row["timestep"] = self._t
        self.rows.append(row)
        self._kv = {}


def _dynamics(c, P=None, mu=None, std=None):
    from offlinerlkit.dynamics import RNNDynamics
    from offlinerlkit.nets import RNNModel
    from offlinerlkit.utils.scaler import StandardScaler
    m = RNNModel(c["input_dim"], c["output_dim"], list(c["hidden"]), c["L"], c["p"])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in (P if P is not None else rc.make_params(c)).items()})
    return RNNDynamics(m, torch.optim.Adam(m.parameters(), lr=c.get("lr", 1e-3)), StandardScaler(mu, std), rc.terminal_fn)


def test_dynamics_learn_equals_the_engine_path():
    c, g = rc.CASES["rnn_tiny"], load_golden("rnn_tiny")
    x, tg, mk = rc.make_data(c)
    dyn = _dynamics(c)
    eng, _ = make_engine(c)
    try:
        eng.load_data(x, tg, mk)
        want = eng.step(np.arange(c["B"]))
        got = dyn.learn((torch.from_numpy(x), torch.from_numpy(tg), torch.from_numpy(mk)))
        assert got == want and rel_err(got, g["loss"], floor=1e-2) < 1e-4
        sd = dyn.model.state_dict()
        after = eng.get_params()
        assert all(np.array_equal(sd[k].cpu().numpy(), after[k]) for k in after)      # the module shows what the engine trained
        assert not np.array_equal(after["output_layer.bias"], rc.make_params(c)["output_layer.bias"])
        assert dyn.learn((x[:2], tg[:2], mk[:2])) == eng.step(np.arange(2))           # host arrays, a shorter batch
    finally:
        eng.close()


def test_dynamics_train_step_save_and_load_follow_the_reference_trace(tmp_path):
    c, g = rc.CASES["rnn_trace"], load_golden("rnn_trace")
    x, tg, mk = rc.make_data(c)
    obss, actions, mu, std = rc.make_windows(c)
    dyn = _dynamics(c, mu=mu, std=std)
    logger = _Logger(tmp_path)
    torch.manual_seed(c["torch_seed"])
    dyn.train([(x[i], tg[i], mk[i]) for i in range(c["n"])], c["B"], c["epochs"], logger)
    got = np.array([r["loss/model"] for r in logger.rows])
    print(f"epoch losses {got} (reference {g['epoch_losses']})")
    assert rel_err(got, g["epoch_losses"]) < 1e-4
    assert sorted(logger.rows[0].keys()) == [str(k) for k in g["logger_keys"]] and [r["timestep"] for r in logger.rows] == list(g["timesteps"])
    assert logger.excluded == ["policy_training_progress"] and not dyn.model.training
    saved = torch.load(str(tmp_path / "dynamics.pth"))
    assert list(saved.keys()) == [str(k) for k in g["state_dict_keys"]]
    nxt, rew, term, info = dyn.step(obss, actions)
    assert scale_err(nxt, g["next_obss"]) < 1e-4 and scale_err(rew, g["rewards"]) < 1e-4
    assert np.array_equal(term, g["terminals"]) and info == {}
    fresh = _dynamics(c, P=rc.make_params(c, seed_offset=50), mu=mu * 0, std=std * 0 + 1)
    assert not np.array_equal(fresh.step(obss, actions)[0], nxt)
    fresh.load(str(tmp_path))
    n2, r2, t2, _ = fresh.step(obss, actions)
    assert np.array_equal(n2, nxt) and np.array_equal(r2, rew) and np.array_equal(t2, term)
