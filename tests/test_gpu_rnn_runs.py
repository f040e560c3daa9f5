"""GPU: RNNDynamics objects of several runs (``orl_rnn_config::n_runs`` = R): run r of an R-run engine against a one-run engine with
seed ``seed + r`` on the same operands, bit for bit -- the one-run side is held to float64 by tests/test_gpu_rnn.py at the same
dimensions -- plus one float64 guard of its own at the last run, and the ``RNNDynamics`` class on top.

Why equality and not a tolerance: every launch gets the runs as a batch dimension only.  The tile configuration and the split-K slab
count of each matrix product are functions of the per-run shape, the scans and the row kernels add ``blockIdx.y * stride`` to their
base pointers, and nothing accumulates with atomics, so the reduction order of every output element is the one-run order."""
import os
import shutil

import numpy as np
import pytest
import torch

import rnn_cases as rc
import rnn_oracle as orc
from diffusion_oracle import grad_distance
from helpers import rel_err, scale_err
from test_gpu_rnn import _Logger, _dynamics

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BLOCKS = (0, 1, 2)      # PARAMS, EXP_AVG, EXP_AVG_SQ


def case_of(H, B, T, L, nin, nout, nh, p):
    return dict(name="shape", input_dim=nin, output_dim=nout, hidden=[H] * nh, H=H, L=L, B=B, T=T, p=p, n=B, seed=900 + H + B + T, lengths=T > 1)


def make_engine(c, R=1, seed=0, params=None, B=None, T=None, p=None):
    """an engine of R runs; params: one dict per run (default: rc.make_params(c, seed_offset=10 * r))"""
    from offlinerlkit import _engine
    cfg = _engine.default_rnn_config(input_dim=c["input_dim"], output_dim=c["output_dim"], hidden=c["hidden"], rnn_num_layers=c["L"],
                                     dropout_rate=c["p"] if p is None else p, batch_size=B or c["B"], max_seq_len=T or c["T"],
                                     lr=c.get("lr", 1e-3), seed=seed, n_runs=R)
    eng = _engine.RnnDynamicsEngine(cfg)
    for r in range(R):
        eng.set_params(params[r] if params is not None else rc.make_params(c, seed_offset=10 * r), run=r)
    return eng


def state(eng, run=0):
    return [eng.get(w, run) for w in BLOCKS]


def same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


def run_indices(c, R, rows, salt):
    """[R, rows]: other rows for every run, in no order, the second a repeat of the first"""
    idx = np.stack([np.random.RandomState(salt + r).randint(0, c["n"], size=rows) for r in range(R)]).astype(np.int64)
    if rows > 1:
        idx[:, 1] = idx[:, 0]
    return idx


# ---- 2. run r equals a one-run engine, bit for bit ---------------------------------------------------------------------------------------------
# (H, B, T, L, in, out, blocks, p, R): R = 9 crosses the 8-problem groups of the z-major GEMM mapping, B = 17 is a second row block of one
# row, H = 8 half a unit tile; Philox masks at an odd R; H = 512 takes the backward scan past 64 KB of LDS and 8 unit groups
RUN_CASES = [(8, 17, 9, 4, 3, 2, 2, 0.0, 9), (72, 16, 2, 1, 1, 3, 3, 0.25, 3), (512, 17, 9, 1, 4, 3, 2, 0.0, 2)]


@pytest.mark.parametrize("case", RUN_CASES, ids=lambda s: "H{}_B{}_T{}_L{}_in{}_out{}_n{}_p{}_R{}".format(*s))
def test_run_r_equals_a_one_run_engine(case):
    *shape, R = case
    c = case_of(*shape)
    p, seed = c["p"], 21
    data = rc.make_data(c)
    steps = [run_indices(c, R, c["B"], 40), run_indices(c, R, max(1, c["B"] // 2), 70)]      # the second step is shorter: no stale rows
    eng = make_engine(c, R, seed)
    try:
        eng.load_data(*data)
        losses = [eng.step_runs(idx) for idx in steps]
        assert eng.step_count == 2
        for r in range(R):
            one = make_engine(c, 1, seed + r, params=[rc.make_params(c, seed_offset=10 * r)])
            try:
                one.load_data(*data)
                want = [np.float32(one.step(idx[r])) for idx in steps]
                assert [l[r] for l in losses] == want, (r, losses, want)
                assert np.array_equal(eng.debug_grads(run=r), one.debug_grads()), r
                assert same(state(eng, r), state(one)), r
                assert np.array_equal(eng.debug_read("pred", run=r), one.debug_read("pred")), r
                assert eng.debug_read("pred", run=r).size == steps[1].shape[1] * c["T"] * c["output_dim"]
                assert float(eng.debug_read("loss", run=r)[0]) == float(want[1])
                if p > 0:
                    assert np.array_equal(eng.debug_read("mask.0", run=r), one.debug_read("mask.0")), r
            finally:
                one.close()
    finally:
        eng.close()


# ---- 3. an independent guard at the last run ---------------------------------------------------------------------------------------------------
def test_last_run_against_the_float64_oracle():
    """case 1 with teacher-forced masks at p = 0.25, another mask per run: run R - 1's loss, pred and gradients against the numpy oracle in
    float64 on that run's operands, at the bars of test_float64_backward_error_outside_the_fixtures (1e-4 of scale on pred and loss,
    gradients at most 4 x the distance fp32 autograd shows from float64 on the same batch)"""
    *shape, R = RUN_CASES[0]
    c = case_of(*shape)
    c["p"] = p = 0.25
    H, B, T, nh, nout = c["H"], c["B"], c["T"], len(c["hidden"]), c["output_dim"]
    x, tg, mk = rc.make_data(c)
    idx = run_indices(c, R, B, 40)
    drop = (np.random.RandomState(3).uniform(size=(R, nh, B * T, H)) >= p).astype(np.float32)
    r = R - 1
    P = rc.make_params(c, seed_offset=10 * r)
    xr, tr, mr = x[idx[r]], tg[idx[r]], mk[idx[r]]
    loss64, pred64, G64, _ = orc.loss_and_grads(P, c, xr, tr, mr, drop[r], np.float64)
    from offlinerlkit.nets import RNNModel
    m = RNNModel(c["input_dim"], nout, [H] * nh, c["L"], 0.0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})

    class Forced(torch.nn.Module):
        def __init__(self, keep):
            super().__init__()
            self.keep = torch.from_numpy(keep)

        def forward(self, v):
            return v * self.keep / (1.0 - p)
    for s, b in enumerate([m.input_layer] + list(m.backbones)):
        b.dropout = Forced(drop[r][s])
    pr, _ = m(torch.from_numpy(xr))
    (((pr - torch.from_numpy(tr)) ** 2).mean(-1) * torch.from_numpy(mr)).mean().backward()
    dist, noise = grad_distance({k: v.grad.numpy() for k, v in m.named_parameters()}, G64)
    from offlinerlkit import _engine
    eng = make_engine(c, R, 0)
    try:
        eng.load_data(x, tg, mk)
        loss = eng.step_runs(idx, drop)[r]
        e_pred = scale_err(eng.debug_read("pred", run=r).reshape(-1, nout), pred64.reshape(-1, nout))
        e_loss = rel_err(float(loss), loss64, floor=1e-2)
        got, n_got = grad_distance(_engine._unflatten(eng.tensors(), eng.debug_grads(run=r)), G64)
        print(f"run {r} of {R}: pred {e_pred:.2e} loss {e_loss:.2e}; gradients {got:.3e} against 4 x {dist:.3e} ({got / (4 * dist):.2f} of the bar); "
              f"zero tensors {n_got:.1e} (fp32 autograd {noise:.1e})")
        assert np.array_equal(eng.debug_read("mask.0", run=r), drop[r][0].ravel())
        assert e_pred < 1e-4 and e_loss < 1e-4
        assert got <= 4 * dist and n_got <= 4 * noise
    finally:
        eng.close()


# ---- 4. runs do not touch each other -----------------------------------------------------------------------------------------------------------
def test_runs_do_not_touch_each_other():
    c = case_of(24, 17, 5, 2, 3, 2, 3, 0.25)
    R, nh = 3, len(c["hidden"])
    data = rc.make_data(c)
    out = []
    for other in (0, 1):                # the two engines differ in run 1 only: parameters, indices and forced masks
        params = [rc.make_params(c, seed_offset=10 * r + (100 * other if r == 1 else 0)) for r in range(R)]
        eng = make_engine(c, R, 3, params=params)
        try:
            eng.load_data(*data)
            losses = []
            for k, rows in enumerate((17, 6)):
                idx = run_indices(c, R, rows, 40 + 30 * k)
                drop = (np.random.RandomState(9 + k).uniform(size=(R, nh, rows * c["T"], c["H"])) >= c["p"]).astype(np.float32)
                if other:
                    idx[1] = idx[1][::-1] + 1 - 2 * (idx[1][::-1] == c["n"] - 1)
                    drop[1] = 1.0 - drop[1]
                losses.append(eng.step_runs(idx, drop))
            out.append((np.array(losses), [state(eng, r) for r in range(R)], [eng.debug_grads(run=r) for r in range(R)]))
        finally:
            eng.close()
    (la, sa, ga), (lb, sb, gb) = out
    for r in (0, 2):
        assert np.array_equal(la[:, r], lb[:, r]) and same(sa[r], sb[r]) and np.array_equal(ga[r], gb[r]), r
    assert not np.array_equal(la[:, 1], lb[:, 1]) and not np.array_equal(ga[1], gb[1])


# ---- 5. learn_epoch_runs equals its steps ------------------------------------------------------------------------------------------------------
def test_epoch_of_runs_equals_its_steps():
    c = rc.CASES["rnn_traj"]
    R, n, B = 3, c["n"], c["B"]
    data = rc.make_data(c)
    a, b = make_engine(c, R), make_engine(c, R)
    try:
        a.load_data(*data)
        b.load_data(*data)
        for k, device in enumerate((False, True)):
            orders = np.stack([np.random.RandomState(5 + 10 * k + r).permutation(n) for r in range(R)]).astype(np.int64)
            la = a.learn_epoch_runs(torch.as_tensor(orders, device=DEV) if device else orders)
            lb = np.stack([b.step_runs(np.ascontiguousarray(orders[:, s:s + B])) for s in range(0, n, B)])
            assert la.shape == (3, R) and n % B and np.array_equal(la, lb), (device, la, lb)      # (the last step is short)
            assert a.step_count == b.step_count == 3 * (k + 1)
            assert all(same(state(a, r), state(b, r)) for r in range(R)), device
        assert not same(state(a, 0), state(a, 1))
    finally:
        a.close(); b.close()


# ---- 6. forward_runs ---------------------------------------------------------------------------------------------------------------------------
def test_forward_runs_against_one_run_engines():
    c = case_of(24, 4, 9, 2, 3, 2, 3, 0.0)
    R, n, T = 3, 33, c["T"]
    x = np.random.RandomState(8).standard_normal((R, n, T, c["input_dim"])).astype(np.float32)
    eng = make_engine(c, R)
    ones = [make_engine(c, 1, params=[rc.make_params(c, seed_offset=10 * r)]) for r in range(R)]
    try:
        last, every = eng.forward_runs(x, want_all=True)                                    # per-run inputs
        assert last.shape == (R, n, c["output_dim"]) and every.shape == (R, n, T, c["output_dim"])
        assert np.array_equal(every[:, :, -1], last)
        want = [o.forward(x[r], want_all=True) for r, o in enumerate(ones)]
        assert all(np.array_equal(last[r], want[r][0]) and np.array_equal(every[r], want[r][1]) for r in range(R))
        assert np.array_equal(eng.debug_read("gru.1", run=2), ones[2].debug_read("gru.1"))
        assert not np.array_equal(last[0], last[1])
        shared = eng.forward_runs(x[0])                                                      # the same inputs for every run
        assert shared.shape == (R, n, c["output_dim"])
        assert all(np.array_equal(shared[r], o.forward(x[0])) for r, o in enumerate(ones))
        single = eng.forward_runs(x[1], run=1, want_all=True)                                # one selected run
        assert np.array_equal(single[0], want[1][0]) and np.array_equal(single[1], want[1][1])
        assert np.array_equal(eng.debug_read("pred", run=1), want[1][1].ravel())               # (the tap is the selected run's)
        with pytest.raises(RuntimeError, match="did not compute run 0"):
            eng.debug_read("pred", run=0)
        small = np.ascontiguousarray(x[:, :5, :2])                                           # fewer rows and steps than before
        ls, es = eng.forward_runs(small, want_all=True)
        assert np.array_equal(es[:, :, -1], ls)
        assert all(np.array_equal(ls[r], o.forward(small[r])) for r, o in enumerate(ones))
        for inp, run in ((x, -1), (x[0], -1), (x[2], 2), (small, -1)):                       # device tensors against host arrays
            dl, de = eng.forward_runs(torch.as_tensor(inp, device=DEV), run=run, want_all=True)
            hl, he = eng.forward_runs(inp, run=run, want_all=True)
            assert np.array_equal(dl.cpu().numpy(), hl) and np.array_equal(de.cpu().numpy(), he)
    finally:
        eng.close()
        for o in ones:
            o.close()


# ---- 7. mask keying ----------------------------------------------------------------------------------------------------------------------------
def test_run_r_draws_the_stream_of_seed_plus_r():
    c = case_of(40, 16, 4, 1, 3, 2, 2, 0.5)
    data = rc.make_data(c)
    idx = np.arange(16)
    eng = make_engine(c, 2, seed=12)
    ones = [make_engine(c, 1, seed=12 + r) for r in range(2)]
    try:
        eng.load_data(*data)
        for o in ones:
            o.load_data(*data)
        for _ in range(2):                  # at step counts 0 and 1
            eng.step_runs(np.stack([idx, idx]))
            masks = [eng.debug_read(f"mask.{s}", run=r) for r in range(2) for s in range(2)]
            for o in ones:
                o.step(idx)
            assert all(np.array_equal(masks[2 * r + s], ones[r].debug_read(f"mask.{s}")) for r in range(2) for s in range(2))
            assert not np.array_equal(masks[0], masks[2]) and set(np.unique(masks[0])) == {0.0, 1.0}
    finally:
        eng.close()
        for o in ones:
            o.close()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_one_run_entry_points_and_bad_indices_are_refused():
    from offlinerlkit import _engine
    c = rc.CASES["rnn_tiny"]
    x, tg, mk = rc.make_data(c)
    eng = make_engine(c, 2)
    try:
        eng.load_data(x, tg, mk)
        with pytest.raises(RuntimeError, match="orl_rnn_step_runs"):
            eng.step(np.arange(2))
        flat = np.empty(eng.floats, np.float32)
        assert eng.lib.orl_rnn_get(eng._h, 0, flat.ctypes.data, flat.size) < 0 and "orl_rnn_get_run" in _engine.last_error()
        assert eng.lib.orl_rnn_set(eng._h, 0, flat.ctypes.data, flat.size) < 0 and "orl_rnn_set_run" in _engine.last_error()
        with pytest.raises(RuntimeError, match="orl_rnn_forward_runs"):
            eng.forward(x)
        with pytest.raises(RuntimeError, match="orl_rnn_learn_epoch_runs"):
            eng.learn_epoch(np.arange(c["n"]))
        assert eng.lib.orl_rnn_debug_grads(eng._h, flat.ctypes.data, flat.size) < 0 and "orl_rnn_debug_grads_run" in _engine.last_error()
        assert eng.lib.orl_rnn_debug_read(eng._h, b"pred", flat.ctypes.data, flat.size) < 0 and "orl_rnn_debug_read_run" in _engine.last_error()
        with pytest.raises(RuntimeError, match="run out of range"):
            eng.get(0, run=2)
        with pytest.raises(RuntimeError, match="row index out of range"):
            eng.step_runs(np.array([[0, 1], [0, c["n"]]], np.int64))                        # in run 1 only
        with pytest.raises(RuntimeError, match="row index out of range"):
            eng.learn_epoch_runs(np.array([[0, 1], [-1, 1]], np.int64))
        with pytest.raises(RuntimeError, match="batch_size"):
            eng.step_runs(np.zeros((2, c["B"] + 1), np.int64))
        assert eng.step_count == 0
        assert eng.step_runs(np.array([[0, 1], [2, 3]], np.int64)).shape == (2,) and eng.step_count == 1
    finally:
        eng.close()
    with pytest.raises(RuntimeError, match="n_runs must be in"):
        make_engine(c, 65)


# ---- 9. the class ------------------------------------------------------------------------------------------------------------------------------
def test_dynamics_class_with_three_runs(tmp_path):
    c = rc.CASES["rnn_trace"]
    x, tg, mk = rc.make_data(c)
    obss, actions, mu, std = rc.make_windows(c)
    data = [(x[i], tg[i], mk[i]) for i in range(c["n"])]
    (tmp_path / "one").mkdir(); (tmp_path / "three").mkdir(); (tmp_path / "run2").mkdir()
    one = _dynamics(c, mu=mu, std=std)
    log1 = _Logger(tmp_path / "one")
    torch.manual_seed(c["torch_seed"])
    one.train(data, c["B"], c["epochs"], log1)
    dyn = _dynamics(c, mu=mu, std=std)
    dyn.set_engine_options(n_runs=3, seed=5)
    log3 = _Logger(tmp_path / "three")
    torch.manual_seed(c["torch_seed"])
    dyn.train(data, c["B"], c["epochs"], log3)
    assert sorted(log3.rows[0]) == ["loss/model", "run0/loss/model", "run1/loss/model", "run2/loss/model", "timestep"]
    assert sorted(log1.rows[0]) == ["loss/model", "timestep"]
    for row in log3.rows:
        assert row["loss/model"] == pytest.approx(np.mean([row[f"run{r}/loss/model"] for r in range(3)]), rel=1e-12)
    # run 0 follows the one-run trace exactly (dropout 0: no device stream enters)
    assert [r["run0/loss/model"] for r in log3.rows] == [r["loss/model"] for r in log1.rows]
    assert len({tuple(r[f"run{k}/loss/model"] for r in log3.rows) for k in range(3)}) == 3
    assert sorted(os.listdir(tmp_path / "three"))[:3] == ["dynamics.pth", "dynamics_run1.pth", "dynamics_run2.pth"]
    # the module and step() follow select_run
    every = dyn.step(np.broadcast_to(obss, (3,) + obss.shape), np.broadcast_to(actions, (3,) + actions.shape))
    assert every[0].shape == (3,) + obss.shape[:1] + obss.shape[2:] and every[2].shape == (3, obss.shape[0], 1) and every[3] == {}
    n0 = dyn.step(obss, actions)
    assert all(np.array_equal(n0[k], every[k][0]) for k in range(3))
    assert all(np.array_equal(n0[k], one.step(obss, actions)[k]) for k in range(3))
    dyn.select_run(2)
    sd, want = dyn.model.state_dict(), dyn._eng.get_params(run=2)
    assert all(np.array_equal(sd[k].cpu().numpy(), want[k]) for k in want)
    n2 = dyn.step(obss, actions)
    assert all(np.array_equal(n2[k], every[k][2]) for k in range(3)) and not np.array_equal(n2[0], n0[0])
    assert np.array_equal(every[2][1], rc.terminal_fn(obss[:, -1], actions[:, -1], every[0][1]))      # terminal_fn per run
    # the saved runs load into one-run objects
    fresh = _dynamics(c, P=rc.make_params(c, seed_offset=50), mu=mu * 0, std=std * 0 + 1)
    fresh.load(str(tmp_path / "three"))
    assert all(np.array_equal(fresh.step(obss, actions)[k], n0[k]) for k in range(3))
    shutil.copy(tmp_path / "three" / "dynamics_run2.pth", tmp_path / "run2" / "dynamics.pth")
    dyn.scaler.save_scaler(str(tmp_path / "run2"))
    fresh2 = _dynamics(c, P=rc.make_params(c, seed_offset=50), mu=mu * 0, std=std * 0 + 1)
    fresh2.load(str(tmp_path / "run2"))
    assert all(np.array_equal(fresh2.step(obss, actions)[k], n2[k]) for k in range(3))
    # learn steps every run; a rebuilt engine (more rows than before) carries all of them
    before = [dyn._eng.get(0, r) for r in range(3)]
    k0 = dyn._eng.step_count
    dyn.model.train()
    losses = dyn.learn_runs((x[:12], tg[:12], mk[:12]))
    assert losses.shape == (3,) and dyn._eng.step_count == k0 + 1 and dyn._cur_run == 2
    assert all(not np.array_equal(dyn._eng.get(0, r), before[r]) for r in range(3))
    assert np.isfinite(dyn.learn((x[:12], tg[:12], mk[:12]))) and dyn._eng.step_count == k0 + 2      # (the selected run's loss)
    sd = dyn.model.state_dict()
    assert all(np.array_equal(sd[k].cpu().numpy(), v) for k, v in dyn._eng.get_params(run=2).items())


def test_dynamics_runs_start_from_their_own_seeds():
    from offlinerlkit.nets import RNNModel
    c = rc.CASES["rnn_trace"]
    obss, actions, mu, std = rc.make_windows(c)
    dyn = _dynamics(c, mu=mu, std=std)
    dyn.set_engine_options(n_runs=3, seed=5)
    dyn.step(obss, actions)                         # builds the engine
    run0 = dyn._eng.get_params(run=0)
    assert all(np.array_equal(run0[k], v) for k, v in rc.make_params(c).items())
    for r in (1, 2):
        torch.manual_seed(5 + r)
        want = RNNModel(c["input_dim"], c["output_dim"], list(c["hidden"]), c["L"], c["p"]).state_dict()
        got = dyn._eng.get_params(run=r)
        assert all(np.array_equal(got[k], want[k].numpy()) for k in want), r
