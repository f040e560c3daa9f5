"""GPU: RNNDynamics' window forward at eval precision 1 (csrc/rnn_fused.hip: k_rnn_pack_planes + k_rnn_fused_fwd under forward /
forward_runs / state_prime).

``pred`` and the top layer's ``gru.<L-1>`` of every run against a float64 numpy forward of the engine's own ``x0``.  Bar (DESIGN.md
4.x10b): scale_err(got, o64) <= SPLIT x BAR x D32 = 16 x D32, D32 = scale_err(o32, o64) of the same forward in numpy fp32, each over a
run's whole [rows * T] matrix.  Cases, one edge each (columns H, in, L, T, rows, R): row tails of the 16-row tile; 8197 and 16389 rows
(the 32- and 64-row tiles: 257 workgroups each on 256 CUs, a ragged last tile); T = 1 and T = max_seq_len; H = 8 (half a unit tile,
k < 32) and 36 (partial tile, k tail); the workload (13 unit tiles, k tail 200 -> 224, three layers, 20 steps); H = 256 (two full tiles
per wave); H = 512 with 4 layers (four tiles per wave, 133 KB of LDS); in = 1, 33, 65 (one, two, three x k-steps); 4 layers; two runs on
shared inputs, on their own, and run 1 alone.  Every case prints its err / D32 (MI355X: profiles/rnn_eval_split_accuracy.json).
"""
import numpy as np
import pytest

import rnn_cases as rc
from helpers import scale_err

pytestmark = pytest.mark.gpu
f32 = np.float32
BAR = 16.0                                  # SPLIT (4) x BAR (4) of tests/diffusion_split_cases.py
ROWS = [("n%d" % n, 24, 5, 1, 3, n, 1) for n in (1, 15, 16, 17, 33)]
CASES = ROWS + [
    ("rt32", 8, 5, 1, 3, 8197, 1), ("rt64", 8, 5, 1, 3, 16389, 1), ("T1", 24, 5, 1, 1, 17, 1), ("Tmax", 24, 5, 1, 5, 17, 1),
    ("h8", 8, 5, 1, 3, 17, 1), ("h36", 36, 5, 1, 3, 17, 1), ("work", 200, 14, 3, 20, 17, 1), ("h256", 256, 5, 1, 3, 17, 1),
    ("h512", 512, 5, 4, 3, 17, 1), ("in1", 24, 1, 1, 3, 17, 1), ("in33", 24, 33, 1, 3, 17, 1), ("in65", 24, 65, 1, 3, 17, 1),
    ("L4", 24, 5, 4, 3, 17, 1), ("R2_shared", 24, 5, 2, 3, 17, 2), ("R2_own", 24, 5, 2, 3, 17, 2), ("R2_run1", 24, 5, 2, 3, 17, 2),
]


def case(H=24, nin=5, L=1, T=3, R=1, nout=4):
    return dict(name="fused", input_dim=nin, output_dim=nout, hidden=[H, H], H=H, L=L, T=T, R=R, seed=8100 + H + nin + L)


def make(c, prec=1, max_T=5):
    """an engine of c["R"] runs (run r: rc.make_params(c, r)) at eval precision ``prec`` -> (engine, [parameters of run r])"""
    from offlinerlkit import _engine
    cfg = _engine.default_rnn_config(input_dim=c["input_dim"], output_dim=c["output_dim"], hidden=c["hidden"], rnn_num_layers=c["L"],
                                     dropout_rate=0.0, batch_size=4, max_seq_len=max(c["T"], max_T), n_runs=c["R"])
    eng, Ps = _engine.RnnDynamicsEngine(cfg), [rc.make_params(c, r) for r in range(c["R"])]
    for r, P in enumerate(Ps):
        eng.set_params(P, r)
    eng.set_eval_precision(prec)
    assert eng.eval_precision == prec
    return eng, Ps


def forward(x0, P, c, T, dt):
    """RNNModel's eval forward of the rows x0 [rows * T, in] in dtype dt -> (top layer's h_t, pred, [h_{T-1} of every layer])"""
    P = {k: v.astype(dt) for k, v in P.items()}
    H, x0 = c["H"], np.asarray(x0, dt)
    B = x0.shape[0] // T
    sig = lambda v: 1 / (1 + np.exp(-v))
    lin = lambda v, key: v @ P[key + "weight"].T + P[key + "bias"]
    X, last = x0.reshape(B, T, -1), []
    for l in range(c["L"]):
        h, hs = np.zeros((B, H), dt), []
        for t in range(T):
            gi = X[:, t] @ P[f"rnn_layer.weight_ih_l{l}"].T + P[f"rnn_layer.bias_ih_l{l}"]
            gh = h @ P[f"rnn_layer.weight_hh_l{l}"].T + P[f"rnn_layer.bias_hh_l{l}"]
            r, z = sig(gi[:, :H] + gh[:, :H]), sig(gi[:, H:2 * H] + gh[:, H:2 * H])
            h = (1 - z) * np.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:]) + z * h
            hs.append(h)
        X = np.stack(hs, 1)
        last.append(h)

    def block(v, res, key):
        zp = lin(v, key + ".linear.")
        u = res + zp * sig(zp)
        mu, var = u.mean(1, keepdims=True), u.var(1, keepdims=True)
        return (u - mu) / np.sqrt(var + dt(1e-5)) * P[key + ".layer_norm.weight"] + P[key + ".layer_norm.bias"]
    top = X.reshape(B * T, H)
    zm = lin(np.concatenate([block(x0, dt(0), "input_layer"), top], 1), "merge_layer.")
    y = zm * sig(zm)
    for i in range(len(c["hidden"]) - 1):
        y = block(y, y, f"backbones.{i}")
    pred = lin(y, "output_layer.")
    assert pred.dtype == dt
    return top, pred, last


def refs(x0, P, c, T):
    return forward(x0, P, c, T, np.float64), forward(x0, P, c, T, f32)


def ratio(got, o64, o32, tag):
    """err / D32 of ``got`` against the float64 forward's o64, D32 from the same forward in fp32"""
    d32 = scale_err(o32, o64)
    assert d32 > 0.0 and got.shape == o64.shape, tag
    r = scale_err(got, o64) / d32
    print(f"{tag}: err / D32 {r:.2f} (bar {BAR:.0f})")
    return r


@pytest.mark.parametrize("cid,H,nin,L,T,rows,R", CASES, ids=[t[0] for t in CASES])
def test_pred_and_top_h_vs_float64(cid, H, nin, L, T, rows, R):
    c = case(H, nin, L, T, R)
    eng, Ps = make(c)
    x = np.random.default_rng(rows + H).standard_normal((R, rows, T, nin)).astype(f32)
    if cid == "R2_own":
        eng.forward_runs(x, run=-1)
    elif R == 2:
        eng.forward_runs(x[0], run=1 if cid == "R2_run1" else -1)
    else:
        eng.forward(x[0])
    for r in ([1] if cid == "R2_run1" else range(R)):
        xr = x[r if cid == "R2_own" else 0].reshape(rows * T, nin)
        x0 = eng.debug_read("x0", run=0 if cid == "R2_shared" else r).reshape(rows * T, nin)      # (shared inputs live in run 0's slot)
        assert np.array_equal(x0, xr)
        top, pred = eng.debug_read(f"gru.{L - 1}", run=r).reshape(-1, H), eng.debug_read("pred", run=r).reshape(rows * T, -1)
        o64, o32 = refs(x0, Ps[r], c, T)
        assert ratio(top, o64[0], o32[0], (cid, r, "gru")) <= BAR
        assert ratio(pred, o64[1], o32[1], (cid, r, "pred")) <= BAR
    eng.close()


def test_state_prime():
    """n < n_traj windows: every layer's slots 0 .. n - 1 hold h_{T-1}, the other slots keep their planted bits"""
    c = case(H=36, L=3, T=4)
    eng, (P,) = make(c)
    n, n_traj = 19, 23
    rng = np.random.default_rng(4)
    x, planted = rng.standard_normal((n, 4, 5)).astype(f32), rng.uniform(-1, 1, size=(n_traj, 36)).astype(f32)
    eng.state_reset(n_traj)
    for l in range(3):
        eng.state_set(l, planted)
    eng.state_prime(x)
    o64, o32 = refs(x.reshape(n * 4, 5), P, c, 4)
    for l in range(3):
        st = eng.state_get(l)
        assert np.array_equal(st[n:], planted[n:])
        assert ratio(st[:n], o64[2][l], o32[2][l], ("state_prime", l)) <= BAR
    eng.close()


def test_option_does_not_leak():
    """a training step and a state step are the fp32 arithmetic at either setting, bit for bit; only the window forward differs"""
    c = dict(case(T=3), B=4, n=4, lengths=False)
    out = []
    for prec in (0, 1):
        eng, _ = make(c, prec)
        eng.load_data(*rc.make_data(c))
        loss = eng.step(np.arange(4))
        eng.set_scaler(np.zeros(5, f32), np.ones(5, f32))
        eng.state_reset(4)
        x = np.random.default_rng(2).standard_normal((4, 3, 5)).astype(f32)
        nxt, rew = eng.state_step(x[:, 0, :3], x[:, 0, 3:])
        out.append((np.concatenate([[loss], eng.get(eng.PARAMS), nxt.ravel(), rew, eng.state_get(0).ravel()]).astype(f32), eng.forward(x)))
        eng.close()
    assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32))
    assert (out[0][1].view(np.uint32) != out[1][1].view(np.uint32)).any()


def test_refusals_and_range_flags():
    c = case()
    eng, (P,) = make(c)
    with pytest.raises(RuntimeError, match="must be 0 .* or 1"):
        eng.set_eval_precision(2)
    x = np.random.default_rng(1).standard_normal((17, 3, 5)).astype(f32)
    good = eng.forward(x)
    with pytest.raises(RuntimeError, match="gi.0"):
        eng.debug_read("gi.0")
    bad = x.copy()
    bad[3, 1, 2] = 1e5
    with pytest.raises(RuntimeError, match="range flag.*activation"):
        eng.forward(bad)
    assert np.array_equal(eng.forward(x).view(np.uint32), good.view(np.uint32))
    W = {k: v.copy() for k, v in P.items()}
    W["rnn_layer.weight_hh_l0"][-1, -1] = 2000.0
    eng.set_params(W)
    for _ in range(2):                               # raised again by every call's pack launch for as long as the weight stays
        with pytest.raises(RuntimeError, match="range flag.*weight"):
            eng.forward(x)
    eng.set_params(P)
    assert np.array_equal(eng.forward(x).view(np.uint32), good.view(np.uint32))
    eng.close()


def test_rnn_dynamics_option():
    """RNNDynamics.set_eval_precision(1), before or after binding: step() is the precision-1 engine's forward on the scaled windows"""
    import torch
    from offlinerlkit.dynamics import RNNDynamics
    from offlinerlkit.nets import RNNModel
    from offlinerlkit.utils.scaler import StandardScaler
    c = case(nin=5, nout=4)
    P = rc.make_params(c)
    rng = np.random.default_rng(6)
    obss, acts = rng.standard_normal((6, 3, 3)).astype(f32), rng.standard_normal((6, 3, 2)).astype(f32)
    sc = StandardScaler((0.2 * rng.standard_normal((1, 5))).astype(f32), (0.8 + 0.4 * rng.uniform(size=(1, 5))).astype(f32))
    got = {}
    for when in ("never", "before", "after"):
        model = RNNModel(5, 4, c["hidden"], 1, 0.0, "cuda:0")
        model.load_state_dict({k: torch.tensor(v) for k, v in P.items()})
        dyn = RNNDynamics(model, torch.optim.Adam(model.parameters(), lr=1e-3), sc, rc.terminal_fn)
        if when == "before":
            dyn.set_eval_precision(1)
        nxt, rew, _, _ = dyn.step(obss, acts)
        if when == "after":
            dyn.set_eval_precision(1)
            nxt, rew, _, _ = dyn.step(obss, acts)
        assert dyn._eng.eval_precision == (when != "never")
        got[when] = np.concatenate([nxt, rew], 1).astype(f32)
    eng, _ = make(c)
    pred = eng.forward(sc.transform(np.concatenate([obss, acts], -1)).astype(f32))
    want = np.concatenate([pred[:, :-1] + obss[:, -1], pred[:, -1:]], 1).astype(f32)
    assert np.array_equal(got["before"], want) and np.array_equal(got["after"], want) and (got["never"] != want).any()
    eng.close()
