"""GPU: RNNDynamics' one-step path -- the carried GRU state in HBM, k_rnn_roll_in, k_rnn_cell, the tail on n rows, k_rnn_roll_head
(csrc/rnn_dynamics.hip; orl_rnn_state_*) -- and the rollouts through it.

1. Per element: state planted with ``state_set``, one step under a scrambled index, every stage read back through the taps and held to
   the float64 restatement of the same stage on the engine's own operands (tests/rnn_roll_refs.py), |got - f64| <= 4 x the propagated
   fp32 bound on EVERY element; the new h in its slot, the reward column and every slot the index does not name bit for bit.  The
   restatements are tied to the oracle and shown to catch eight planted defects in tests/test_rnn_roll_cpu.py.
2. Carried steps equal the window forward: both within the 1e-4 gate of the float64 oracle, from zero and from a primed state.
3. A trajectory's bits do not depend on which others are stepped beside it; identical sequences give identical bits; run r of a
   two-run object is a one-run object bit for bit.
4. ``RcslPolicy.rollout`` through ``step_state`` and ``rollout_device`` through ``step_device`` agree bit for bit on every key.

Worst err / bound per check over the five shapes (bar: 4), measured on an MI355X: k_rnn_roll_in.x 0.88, k_rnn_cell.h 0.13 (0.134 at
H = 8, 0.007 at H = 200, 0.003 at H = 512: the any-order bound of a product grows with its depth), tail.act 0.33, tail.drop 1.00,
tail.norm 0.16, tail.merge 0.08, tail.pred 0.08, k_rnn_roll_head.next_obs 1.00 (one rounding against a bound of one rounding); the
bit-for-bit checks (the slot is the new h, the untouched slots, the reward column) hold.  Carried against the float64 oracle 7.2e-7
of the output scale, the window forward 6.5e-7, carried against window 4.5e-7 (from zero) and 3.3e-7 (primed)."""
import numpy as np
import pytest

import rcsl_rollout_ref as ref
import rnn_cases as rc
import rnn_oracle as orc
import rnn_refs as rf
import rnn_roll_refs as rl
from helpers import scale_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _figures():
    yield
    print("\nworst |got - f64| / bound per check of the one-step path:", {k: round(v, 4) for k, v in sorted(WORST.items())})


def make_engine(c, runs=1, seed=5, T=1, p=0.0, rows=None, offsets=None):
    """an engine at a case's shape; run r holds rc.make_params(c, 50 * r) (``offsets``: other seed offsets) -> (engine, [parameters])"""
    from offlinerlkit import _engine
    assert "orl_rnn_state_step" in _engine.ABI_SYMBOLS and hasattr(_engine.RnnDynamicsEngine, "state_step"), \
        "this build has no orl_rnn_state_step: nothing here can be checked"          # before any device object exists
    cfg = _engine.default_rnn_config(input_dim=c["input_dim"], output_dim=c["output_dim"], hidden=c["hidden"], rnn_num_layers=c["L"],
                                     dropout_rate=p, batch_size=rows or c["n_traj"], max_seq_len=T, seed=seed, n_runs=runs)
    eng = _engine.RnnDynamicsEngine(cfg)
    Ps = [rc.make_params(c, seed_offset=o) for o in (offsets or [50 * r for r in range(runs)])]
    for r, P in enumerate(Ps):
        eng.set_params(P, r)
    return eng, Ps


def plant(eng, states):
    """states [R][L, n_traj, H] into the engine"""
    for r, st in enumerate(states):
        for l in range(st.shape[0]):
            eng.state_set(l, st[l], run=r)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. every stage of one step, per element ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rl.CASES))
def test_one_step_holds_per_element(name):
    c = rl.case(name)
    R, n, n_traj = c["runs"], c["rows"], c["n_traj"]
    eng, Ps = make_engine(c, runs=R)
    try:
        ins = [rl.make_inputs(c, seed=r) for r in range(R)]
        _, _, _, index, mu, std = ins[0]                                     # the index and the scaler are shared by the runs
        before = [i[0] for i in ins]
        obs, act = np.stack([i[1] for i in ins]), np.stack([i[2] for i in ins])
        eng.set_scaler(mu, std)
        eng.state_reset(n_traj)
        assert all(not eng.state_get(l, r).any() for r in range(R) for l in range(c["L"]))
        plant(eng, before)
        if R == 1:
            nxt, rew = eng.state_step(obs[0], act[0], index)
            nxt, rew = nxt[None], rew[None]
        else:
            nxt, rew = eng.state_step(obs, act, index, run=-1)
        assert nxt.shape == (R, n, c["obs_dim"]) and rew.shape == (R, n)
        rec = rf.Rec()
        kept = []
        for r in range(R):
            def rd(nm, r=r):
                return eng.state_get(int(nm[6:]), r) if nm.startswith("state.") else eng.debug_read(nm, run=r).reshape(n, -1)
            rl.check_step(rd, Ps[r], c, before[r], obs[r], act[r], index, mu, std, nxt[r], rew[r], rec)
            kept.append([eng.state_get(l, r) for l in range(c["L"])])
        for k, v in rec.worst.items():
            WORST[k] = max(WORST.get(k, 0.0), v)
        print(f"case {name}: worst err / bound per check", {k: round(v, 3) for k, v in sorted(rec.worst.items())})
        rec.finish()
        with pytest.raises(RuntimeError, match="no input projections"):
            eng.debug_read("gi.0", run=R - 1)
        # the same step on device tensors, and (two runs) of the last run alone: the same bits, the other run untouched
        import torch
        plant(eng, before)
        t = lambda a, dt=torch.float32: torch.tensor(a, dtype=dt, device=DEV)
        if R == 1:
            n2, r2 = eng.state_step(t(obs[0]), t(act[0]), t(index, torch.int64))
            assert np.array_equal(bits(n2.cpu().numpy()), bits(nxt[0])) and np.array_equal(bits(r2.cpu().numpy()), bits(rew[0]))
        else:
            n2, r2 = eng.state_step(t(obs[R - 1]), t(act[R - 1]), t(index, torch.int64), run=R - 1)
            assert np.array_equal(bits(n2.cpu().numpy()), bits(nxt[R - 1])) and np.array_equal(bits(r2.cpu().numpy()), bits(rew[R - 1]))
            for l in range(c["L"]):
                assert np.array_equal(bits(eng.state_get(l, 0)), bits(before[0][l])), l
            with pytest.raises(RuntimeError, match="did not compute run 0"):
                eng.debug_read("roll.pred", run=0)
        for l in range(c["L"]):
            assert np.array_equal(bits(eng.state_get(l, R - 1)), bits(kept[R - 1][l])), l
    finally:
        eng.close()


# ---- 2. carried steps equal the window forward ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T0", [0, 3])
def test_carried_steps_equal_the_window_forward(T0):
    """8 teacher-forced steps of 37 trajectories at 14 / 12 / 200 / 3 (the last 5 carried after a window of 3 when primed): pred of the
    carried step t and forward(want_all)[:, t] are both within the 1e-4 gate of the float64 oracle.  The engine's dropout rate is 0.1:
    the eval paths apply none"""
    c = rl.case("default")
    n, T = c["n_traj"], 8
    eng, (P,) = make_engine(c, T=T, p=0.1)
    try:
        rng = np.random.RandomState(c["seed"] + 11)
        obs = rng.standard_normal((n, T, c["obs_dim"])).astype(np.float32)
        act = np.tanh(rng.standard_normal((n, T, c["act_dim"]))).astype(np.float32)
        _, _, _, _, mu, std = rl.make_inputs(c)
        xs = ((np.concatenate([obs, act], -1) - mu).astype(np.float32) / std).astype(np.float32)      # StandardScaler.transform in fp32
        want = orc.forward(P, c, xs, None, np.float64)[0]
        _, window = eng.forward(xs, want_all=True)
        eng.set_scaler(mu, std)
        eng.state_reset(n)
        if T0:
            eng.state_prime(xs[:, :T0])
        got = []
        for t in range(T0, T):
            nxt, rew = eng.state_step(obs[:, t], act[:, t])
            pred = eng.debug_read("roll.pred").reshape(n, -1)
            assert np.array_equal(bits(eng.debug_read("roll.x").reshape(n, -1)), bits(xs[:, t]))
            assert np.array_equal(bits(rew), bits(pred[:, -1])) and np.array_equal(bits(nxt), bits(pred[:, :-1] + obs[:, t]))
            got.append(pred)
        got = np.stack(got, 1)
        e_c, e_w = scale_err(got, want[:, T0:]), scale_err(window, want)
        print(f"T0 = {T0}: carried vs float64 {e_c:.3e}, window vs float64 {e_w:.3e}, carried vs window {scale_err(got, window[:, T0:]):.3e}")
        assert e_c < 1e-4 and e_w < 1e-4
    finally:
        eng.close()


# ---- 3. independence and determinism ---------------------------------------------------------------------------------------------------------
def _sequence(eng, c, obs, act, live):
    """steps t = 0 .. on the trajectories live[t] (None: all, no index) -> (state of every layer after the last step, outputs per step)"""
    eng.state_reset(c["n_traj"])
    outs = []
    for t, ix in enumerate(live):
        o, a = (obs[:, t], act[:, t]) if ix is None else (obs[ix, t], act[ix, t])
        outs.append(eng.state_step(o, a, ix))
    return [eng.state_get(l) for l in range(c["L"])], outs


def test_a_trajectory_does_not_depend_on_its_neighbours_and_sequences_repeat():
    c = rl.case("default")
    n = c["n_traj"]
    eng, _ = make_engine(c)
    try:
        rng = np.random.RandomState(c["seed"] + 12)
        obs = rng.standard_normal((n, 4, c["obs_dim"])).astype(np.float32)
        act = np.tanh(rng.standard_normal((n, 4, c["act_dim"]))).astype(np.float32)
        _, _, _, _, mu, std = rl.make_inputs(c)
        eng.set_scaler(mu, std)
        s1 = np.sort(rng.permutation(n)[:21]).astype(np.int64)                # thinned at step 1 ...
        s2 = s1[np.sort(rng.permutation(21)[:9])]                            # ... and again at step 2: other tiles, other row positions
        full, fo = _sequence(eng, c, obs, act, [None, None, None, None])
        thin, to = _sequence(eng, c, obs, act, [None, s1, s2, s2])
        again, ao = _sequence(eng, c, obs, act, [None, s1, s2, s2])
        for l in range(c["L"]):
            assert np.array_equal(bits(full[l][s2]), bits(thin[l][s2])), l
            assert np.array_equal(bits(thin[l]), bits(again[l])), l
            assert full[l][s2].any()
        for t, ix in enumerate([np.arange(n), s1, s2, s2]):
            for k in (0, 1):
                assert np.array_equal(bits(fo[t][k][ix]), bits(to[t][k])), (t, k)
                assert np.array_equal(bits(to[t][k]), bits(ao[t][k])), (t, k)
        # a trajectory the thinned sequence dropped after step 0 kept that step's h
        gone = np.setdiff1d(np.arange(n), s1)
        eng.state_reset(n)
        eng.state_step(obs[:, 0], act[:, 0])
        for l in range(c["L"]):
            assert np.array_equal(bits(eng.state_get(l)[gone]), bits(thin[l][gone])), l
        # refusals by name
        with pytest.raises(RuntimeError, match="twice in one step"):
            eng.state_step(obs[:2, 0], act[:2, 0], np.array([3, 3]))
        with pytest.raises(RuntimeError, match="out of range"):
            eng.state_step(obs[:2, 0], act[:2, 0], np.array([3, n]))
        eng.state_reset(4)
        with pytest.raises(RuntimeError, match="state of 4 trajectories"):
            eng.state_step(obs[:5, 0], act[:5, 0])
        with pytest.raises(RuntimeError, match="unknown tap"):
            eng.debug_read("state.3")
        with pytest.raises(RuntimeError, match="unknown tap"):
            eng.debug_read("roll.h.3")
    finally:
        eng.close()


def test_a_run_of_two_is_a_one_run_object_bit_for_bit():
    c = rl.case("runs")
    n = c["n_traj"]
    two, _ = make_engine(c, runs=2, seed=9, T=3)
    ones = [make_engine(c, runs=1, seed=9 + r, T=3, offsets=[50 * r])[0] for r in range(2)]
    try:
        rng = np.random.RandomState(c["seed"] + 13)
        hist = rng.standard_normal((2, n, 3, c["input_dim"])).astype(np.float32)
        obs = rng.standard_normal((2, n, 2, c["obs_dim"])).astype(np.float32)
        act = np.tanh(rng.standard_normal((2, n, 2, c["act_dim"]))).astype(np.float32)
        _, _, _, index, mu, std = rl.make_inputs(c)
        for e in [two] + ones:
            e.set_scaler(mu, std)
            e.state_reset(n)
        two.state_prime(hist)
        outs = [two.state_step(obs[:, :, 0], act[:, :, 0], run=-1), two.state_step(obs[:, index, 1], act[:, index, 1], index, run=-1)]
        for r, e in enumerate(ones):
            e.state_prime(hist[r])
            alone = [e.state_step(obs[r, :, 0], act[r, :, 0]), e.state_step(obs[r, index, 1], act[r, index, 1], index)]
            for t in (0, 1):
                for k in (0, 1):
                    assert np.array_equal(bits(outs[t][k][r]), bits(alone[t][k])), (r, t, k)
            for l in range(c["L"]):
                assert np.array_equal(bits(two.state_get(l, r)), bits(e.state_get(l))), (r, l)
    finally:
        for e in [two] + ones:
            e.close()


# ---- 4. the rollouts -------------------------------------------------------------------------------------------------------------------------
N_TRAJ, LENGTH, OD, AD = 48, 6, 3, 2


def _dynamics(terminal_fn):
    """an RNNDynamics (H 32, 2 GRU layers) with fixed parameters: a head that moves x0 up by about 0.1 a step, so that with
    termination_fn_ant's 0.2 <= x0 <= 1 the start decides the step a trajectory ends at, whatever the (untrained) policy does"""
    import torch
    from offlinerlkit.dynamics import RNNDynamics
    from offlinerlkit.nets import RNNModel
    from offlinerlkit.utils.scaler import StandardScaler
    c = dict(input_dim=OD + AD, output_dim=OD + 1, hidden=[32, 32, 32], H=32, L=2, seed=8800)
    P = rc.make_params(c)
    P["output_layer.weight"] = (P["output_layer.weight"] * np.float32(0.02)).astype(np.float32)
    P["output_layer.bias"] = np.array([0.1, 0.0, 0.0, 0.5], np.float32)
    model = RNNModel(c["input_dim"], c["output_dim"], c["hidden"], c["L"], 0.1, DEV)
    model.load_state_dict({k: torch.tensor(v) for k, v in P.items()})
    model.eval()
    rng = np.random.RandomState(c["seed"] + 2)
    sc = StandardScaler((0.2 * rng.standard_normal((1, OD + AD))).astype(np.float32), (0.8 + 0.4 * rng.uniform(size=(1, OD + AD))).astype(np.float32))
    return RNNDynamics(model, torch.optim.Adam(model.parameters(), lr=1e-3), sc, terminal_fn)


def test_rollout_device_matches_the_host_rollout_bit_for_bit():
    """two RNNDynamics with the same parameters and scaler, one untrained AutoregressivePolicy, the same torch seed: the host rollout
    through ``step_state`` and the device rollout through ``step_device`` agree on every key"""
    import torch
    from offlinerlkit.modules import RcslModule
    from offlinerlkit.nets import MLP
    from offlinerlkit.policy import AutoregressivePolicy, RcslPolicy
    from offlinerlkit.utils import termination_fns as tf
    dyn_a, dyn_b = _dynamics(tf.termination_fn_ant), _dynamics(tf.termination_fn_ant)
    assert dyn_b.term_kind == tf.TERM_ANT and dyn_b.stateful
    torch.manual_seed(0)
    ar = AutoregressivePolicy(OD, AD, [32, 32], 1e-3, DEV)
    mod = RcslModule(MLP(input_dim=OD + 1, hidden_dims=[32, 32], output_dim=AD), DEV)
    pol = RcslPolicy(dyn_a, ar, mod, torch.optim.Adam(mod.parameters(), lr=1e-3), DEV)
    rng = np.random.RandomState(1)
    init = np.concatenate([rng.permutation(np.linspace(0.25, 0.95, N_TRAJ))[:, None], rng.uniform(-1.0, 1.0, (N_TRAJ, OD - 1))], 1).astype(np.float32)
    torch.manual_seed(123)
    host, hinfo = pol.rollout(init, LENGTH)
    # not vacuous (on the HOST rollout): some but not all trajectories end in each of the first two steps, one at least reaches the last
    term = host["terminals"].ravel()
    n1 = int((~term[:N_TRAJ]).sum())
    n2 = int((~term[N_TRAJ:N_TRAJ + n1]).sum())
    per_traj = np.bincount(host["traj_idxs"], minlength=N_TRAJ)
    print(f"host rollout: {len(term)} transitions, survivors {N_TRAJ} -> {n1} -> {n2}, {int((per_traj == LENGTH).sum())} of full length")
    assert 0 < n1 < N_TRAJ and 0 < n2 < n1 and (per_traj == LENGTH).any()
    pol.dynamics = dyn_b
    torch.manual_seed(123)
    roll, dinfo = pol.rollout_device(init, LENGTH)
    got = roll.to_host()
    assert list(got.keys()) == list(host.keys()) == ref.KEYS
    for k in ref.KEYS:
        assert got[k].dtype == host[k].dtype and got[k].shape == host[k].shape, (k, got[k].dtype, got[k].shape, host[k].dtype, host[k].shape)
        assert np.array_equal(ref.bits(got[k]), ref.bits(host[k])), k
    assert dinfo["num_transitions"] == hinfo["num_transitions"] == len(term)
    assert np.array_equal(ref.bits(dinfo["returns"]), ref.bits(hinfo["returns"]))
    # a second rollout starts from a fresh state: the same bits again
    torch.manual_seed(123)
    roll2, _ = pol.rollout_device(init, LENGTH)
    again = roll2.to_host()
    assert all(np.array_equal(ref.bits(again[k]), ref.bits(got[k])) for k in ref.KEYS)


def test_rollout_device_still_refuses_a_termination_function_without_a_kind():
    import torch
    from offlinerlkit.modules import RcslModule
    from offlinerlkit.nets import MLP
    from offlinerlkit.policy import AutoregressivePolicy, RcslPolicy
    from offlinerlkit.utils import termination_fns as tf
    dyn = _dynamics(tf.obs_unnormalization(tf.termination_fn_ant, 0.0, 1.0))
    assert dyn.term_kind is None
    mod = RcslModule(MLP(input_dim=OD + 1, hidden_dims=[32, 32], output_dim=AD), DEV)
    pol = RcslPolicy(dyn, AutoregressivePolicy(OD, AD, [32, 32], 1e-3, DEV), mod, torch.optim.Adam(mod.parameters(), lr=1e-3), DEV)
    with pytest.raises(NotImplementedError, match="term_kind"):
        pol.rollout_device(np.zeros((4, OD), np.float32), 2)
    # ... and the model-based rollouts, which start no state, are refused by name
    with pytest.raises(RuntimeError, match="reset_state"):
        dyn.step_device(torch.zeros(4, OD, device=DEV), torch.zeros(4, AD, device=DEV))
