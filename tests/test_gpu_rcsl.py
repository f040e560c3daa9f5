"""GPU: RCSL on the HIP engine (ORL_ALGO_RCSL, orl_learn_epoch, RcslPolicy, RcslPolicyTrainer) against the numpy oracle
(tests/rcsl_oracle.py) and the fixtures of the real reference (tests/golden/make_rcsl_golden.py).

Bars: loss 1e-4 (rel_err, floor 1e-2), ``pred`` 1e-4 of its scale, step-0 gradients at the per-precision constants of
tests/test_gpu_grads.py, post-step parameters by the run_case scheme of tests/test_gpu_algos.py with its absolute term scaled by
lr / 3e-4 (Adam's step is proportional to lr): mean |d| < 1e-6 (k + 1) s, at most 2e-3 of a tensor's elements beyond
4e-6 (k + 1) s + 1e-4 max |p|.  make_rcsl_golden.py asserts that the oracle meets half that against the reference."""
import numpy as np
import pytest
import torch

import rcsl_cases as rc
import rcsl_oracle as orc
from helpers import load_golden, rel_err, scale_err, check_state_against_golden
from test_gpu_grads import check_grads

pytestmark = pytest.mark.gpu
NET = 0      # ORL_NET_ACTOR


def make_engine(case, n_runs=1, precision=0, nets=None, algo="rcsl", **over):
    from offlinerlkit import _engine
    c, net, batches = rc.case_inputs(case)
    cfg = dict(obs_dim=c["obs_dim"], act_dim=c["act_dim"], hidden=c["hidden"], batch_size=c["B"], n_runs=n_runs, precision=precision,
               actor_lr=c["lr"])
    cfg.update(over)
    eng = _engine.Engine(_engine.default_config(algo, **cfg))
    if algo == "rcsl":
        for r in range(n_runs):
            eng.set_net(r, NET, nets[r] if nets is not None else net)
    return eng, c, net, batches


def lead(b, R=1):
    return dict(observations=np.stack([b["observations"]] * R), actions=np.stack([b["actions"]] * R), rewards=np.stack([b["rtgs"]] * R))


def check_params(got, ref, k, lr, tag):
    s = lr / 3e-4
    worst = 0.0
    for pn, v in got.items():
        d = np.abs(v - ref[pn])
        tol = 4e-6 * (k + 1) * s + 1e-4 * np.abs(ref[pn]).max()
        assert d.mean() < 1e-6 * (k + 1) * s, (tag, pn, k, d.mean())
        assert (d > tol).mean() < 2e-3, (tag, pn, k, (d > tol).mean())
        worst = max(worst, float(d.max()) / s)
    return worst


@pytest.mark.parametrize("case,precision", [(c, p) for c in rc.CASES for p in (0, 1)] + [("rcsl_tiny", 2)])
def test_rcsl_step(case, precision):
    """orl_step against the reference fixture and the oracle: loss, pred, step-0 gradient, parameters after every step; the net's
    tensor names are the reference's state_dict keys"""
    eng, c, net, batches = make_engine(case, precision=precision)
    g = load_golden(case)
    st = orc.init_state(net)
    try:
        assert eng.metric_names == ["loss"] == [str(k) for k in g["loss_keys"]]
        assert ["rcsl." + n for n, _, _ in eng.net_tensors(NET)] == [str(k) for k in g["keys"]]
        worst = 0.0
        for k, b in enumerate(batches):
            res, aux = orc.learn(st, c, b)
            m = eng.step(lead(b), [])[0]
            print(f"{case} precision {precision} step {k}: loss {m[0]:.6g} oracle {res['loss']:.6g} reference {g[f'step{k}/losses'][0]:.6g}")
            assert rel_err(m, np.array([res["loss"]]), floor=1e-2) < 1e-4, (case, k, m, res)
            assert rel_err(m, g[f"step{k}/losses"], floor=1e-2) < 1e-4, (case, k, m, g[f"step{k}/losses"])
            if k == 0:
                pred = eng.debug_read(0, "pred").reshape(c["B"], c["act_dim"])
                x = eng.debug_read(0, "rcsl_x").reshape(c["B"], c["obs_dim"] + 1)
                assert np.array_equal(x, aux["x"])
                print(f"  pred err / scale: oracle {scale_err(pred, aux['pred']):.2e} reference {scale_err(pred, g['step0/pred']):.2e}")
                assert scale_err(pred, aux["pred"]) < 1e-4 and scale_err(pred, g["step0/pred"]) < 1e-4
                report = []
                check_grads(eng, 0, NET, aux["grads"], (case, precision), precision, report)
                print(f"  step-0 gradients vs oracle: worst max/scale {max(x[2] for x in report):.2e}, worst rel L2 {max(x[3] for x in report):.2e}")
            got = eng.get_net(0, NET)
            check_state_against_golden(g, f"state{k}", {"rcsl": got}, atol=4e-6 * (k + 1) * c["lr"] / 3e-4)
            worst = max(worst, check_params(got, st["rcsl"], k, c["lr"], case))
        print(f"{case} precision {precision}: worst parameter error vs oracle, over lr / 3e-4: {worst:.2e}")
    finally:
        eng.close()


@pytest.mark.parametrize("precision", [0, 1, 2])
def test_identical_runs_stay_bit_identical(precision):
    R = 16
    eng, c, net, batches = make_engine("rcsl_hopper", n_runs=R, precision=precision)
    try:
        for k, b in enumerate(batches):
            m = eng.step(lead(b, R), [])
            for r in range(1, R):
                assert np.array_equal(m[0], m[r]), (k, r, m[0], m[r])
        a = eng.get_net(0, NET)
        for r in (1, R // 2, R - 1):
            b1 = eng.get_net(r, NET)
            for pn in a:
                assert np.array_equal(a[pn], b1[pn]), (pn, r)
    finally:
        eng.close()


@pytest.mark.parametrize("case", ["rcsl_odd", "rcsl_hopper"])
def test_distinct_runs_follow_the_oracle(case):
    """16 runs with their own weights and batches: every run follows its own oracle"""
    R = 16
    ins = [rc.case_inputs(case, run=r) for r in range(R)]
    eng, c, _, _ = make_engine(case, n_runs=R, nets=[i[1] for i in ins])
    states = [orc.init_state(i[1]) for i in ins]
    try:
        for k in range(rc.STEPS):
            bs = [i[2][k] for i in ins]
            m = eng.step(dict(observations=np.stack([b["observations"] for b in bs]), actions=np.stack([b["actions"] for b in bs]),
                              rewards=np.stack([b["rtgs"] for b in bs])), [])
            for r in range(R):
                res, _ = orc.learn(states[r], c, bs[r])
                assert rel_err(m[r], np.array([res["loss"]]), floor=1e-2) < 1e-4, (case, k, r, m[r], res)
        for r in (0, R - 1):
            check_params(eng.get_net(r, NET), states[r]["rcsl"], rc.STEPS - 1, c["lr"], (case, r))
    finally:
        eng.close()


def _buffer(data):
    from offlinerlkit import _engine
    n = len(data["observations"])
    buf = _engine.DeviceBuffer(data["observations"].shape[1], data["actions"].shape[1])
    buf.load(data["observations"], data["actions"], data["observations"], data["rtgs"].reshape(n), np.zeros(n, np.float32))
    return buf


@pytest.mark.parametrize("precision", [0, 1])
def test_learn_epoch_follows_the_order_and_masks_the_padding(precision):
    """rcsl_tiny, 3 runs, N = 3 B + 5: four steps, the last with 5 valid rows.  Epoch 1 step by step (``order`` slices): the batch taps
    are dataset[order] byte for byte on the valid rows, loss and parameters follow the oracle fed the valid rows only, the tail loss is
    NOT the loss over all B gathered rows, and the graph's step equals an eager orl_step on the tapped arrays (full steps: orl_step has no
    padding).  Then the same epoch in ONE call on a twin engine: its mean is the mean of the per-step values and its parameters are the
    stepwise engine's bit for bit; a second epoch with a new order reuses the graph and still follows the oracle."""
    R = 3
    c, data, orders = rc.epoch_inputs("rcsl_tiny", R)
    B, od, ad, n = c["B"], c["obs_dim"], c["act_dim"], len(data["observations"])
    eng, _, net, _ = make_engine("rcsl_tiny", n_runs=R, precision=precision)
    whole, _, _, _ = make_engine("rcsl_tiny", n_runs=R, precision=precision)
    eager, _, _, _ = make_engine("rcsl_tiny", n_runs=R, precision=precision)
    buf = _buffer(data)
    states = [orc.init_state(net) for _ in range(R)]
    try:
        eng.attach_buffer(buf); whole.attach_buffer(buf)
        per_step = []
        for s in range(4):
            sl = orders[0][:, s * B:(s + 1) * B]
            m, _ = eng.learn_epoch(sl)
            per_step.append(m.copy())
            assert eng.step_count() == s + 1
            taps = []
            for r in range(R):
                valid = sl[r] >= 0
                assert valid.sum() == (B if s < 3 else 5)
                t = dict(observations=eng.debug_read(r, "b_obs").reshape(B, od), actions=eng.debug_read(r, "b_act").reshape(B, ad),
                         rtgs=eng.debug_read(r, "b_rew").reshape(B, 1))
                taps.append(t)
                want = rc.gather(data, sl[r])
                for k in t:
                    assert np.array_equal(t[k][valid], want[k][valid]), (s, r, k)
                    assert np.array_equal(t[k], want[k]), (s, r, k)                      # padding reads dataset row 0: defined, in bounds
                x = eng.debug_read(r, "rcsl_x").reshape(B, od + 1)
                assert np.array_equal(x, np.concatenate([want["observations"], want["rtgs"]], 1))
                if s == 3:
                    all_rows, _ = orc.learn(orc.init_state(states[r]["rcsl"]), c, want)          # what an unmasked kernel would report
                res, aux = orc.learn(states[r], c, {k: v[valid] for k, v in want.items()})
                print(f"precision {precision} step {s} run {r}: loss {m[r, 0]:.6g} oracle (valid rows) {res['loss']:.6g}")
                assert rel_err(m[r], np.array([res["loss"]]), floor=1e-2) < 1e-4, (s, r, m[r], res)
                if s == 3:
                    assert abs(m[r, 0] - all_rows["loss"]) > 1e-3 * abs(res["loss"]), (r, m[r, 0], all_rows["loss"], res["loss"])
                check_params(eng.get_net(r, NET), states[r]["rcsl"], s, c["lr"], (s, r))
            if s < 3:
                me = eager.step(dict(observations=np.stack([t["observations"] for t in taps]), actions=np.stack([t["actions"] for t in taps]),
                                     rewards=np.stack([t["rtgs"] for t in taps])), [])
                assert rel_err(m, me, floor=1e-3) < 2e-6, (s, np.abs(m - me).max())
        mw, ms = whole.learn_epoch(orders[0])
        assert ms > 0 and whole.step_count() == 4
        assert np.allclose(mw, np.mean(per_step, axis=0), rtol=1e-6, atol=0), (mw, np.mean(per_step, axis=0))
        for r in range(R):
            a, b = eng.get_net(r, NET), whole.get_net(r, NET)
            for pn in a:
                assert np.array_equal(a[pn], b[pn]), (r, pn)
        # second epoch, new order, device-resident: same graph
        o2 = torch.as_tensor(orders[1], device="cuda:0")
        torch.cuda.synchronize()
        m2, _ = whole.learn_epoch((o2.data_ptr(), o2.shape[1]), on_device=True)
        assert whole.step_count() == 8
        tot = np.zeros(R)
        for s in range(4):
            for r in range(R):
                idx = orders[1][r, s * B:(s + 1) * B]
                res, _ = orc.learn(states[r], c, rc.gather(data, idx[idx >= 0]))
                tot[r] += res["loss"] / 4
        assert rel_err(m2[:, 0], tot, floor=1e-2) < 1e-4, (m2, tot)
        for r in range(R):
            check_params(whole.get_net(r, NET), states[r]["rcsl"], 7, c["lr"], ("epoch 2", r))
        # orl_learn_n keeps working on an RCSL engine (i.i.d. draws)
        m3, _ = whole.learn_n(5)
        assert np.isfinite(m3).all() and whole.step_count() == 13
        idx_rows = whole.debug_read(0, "b_obs").reshape(B, od)
        assert all(any(np.array_equal(row, d) for d in data["observations"]) for row in idx_rows)
    finally:
        eng.close(); whole.close(); eager.close(); buf.close()


def test_refusals_leave_the_engine_untouched():
    from offlinerlkit import _engine
    c, data, orders = rc.epoch_inputs("rcsl_tiny", 1)
    B, n = c["B"], len(data["observations"])
    eng, _, net, _ = make_engine("rcsl_tiny")
    buf = _buffer(data)
    try:
        def refused(call, text):
            before, steps = eng.get_net(0, NET), eng.step_count()
            with pytest.raises(RuntimeError, match=text):
                call()
            after = eng.get_net(0, NET)
            assert eng.step_count() == steps and all(np.array_equal(before[k], after[k]) for k in before)
        good = orders[0]
        refused(lambda: eng.learn_epoch(good), "no replay buffer")
        eng.attach_buffer(buf)
        bad = good.copy(); bad[0, 3] = n
        refused(lambda: eng.learn_epoch(bad), "beyond the buffer")
        t = torch.as_tensor(bad, device="cuda:0"); torch.cuda.synchronize()
        refused(lambda: eng.learn_epoch((t.data_ptr(), t.shape[1]), on_device=True), "beyond the buffer")
        refused(lambda: eng.learn_epoch(good[:, :3 * B + 5]), "multiple of batch_size")
        pad = np.concatenate([good, np.full((1, B), -1, np.int64)], 1)
        refused(lambda: eng.learn_epoch(pad), "padding")
        t2 = torch.as_tensor(pad, device="cuda:0"); torch.cuda.synchronize()
        refused(lambda: eng.learn_epoch((t2.data_ptr(), t2.shape[1]), on_device=True), "padding")
        refused(lambda: eng.set_next_samples(np.zeros((1, 4, c["obs_dim"]), np.float32)), "MOBILE")
        ring = _engine.DeviceBuffer(c["obs_dim"], c["act_dim"]); ring.reserve(64)
        refused(lambda: eng.attach_model_buffer(ring, 4), "RCSL")
        ring.close()
        m, _ = eng.learn_epoch(good)                                   # and the engine still works
        assert np.isfinite(m).all() and eng.step_count() == 4
    finally:
        eng.close()
    # a non-RCSL engine
    iql = _engine.Engine(_engine.default_config("iql", obs_dim=c["obs_dim"], act_dim=c["act_dim"], hidden=[32, 32], batch_size=B))
    try:
        iql.attach_buffer(buf)
        before = iql.get_net(0, NET)
        with pytest.raises(RuntimeError, match="RCSL engines only"):
            iql.learn_epoch(orders[0])
        after = iql.get_net(0, NET)
        assert iql.step_count() == 0 and all(np.array_equal(before[k], after[k]) for k in before)
    finally:
        iql.close(); buf.close()


def test_rtg_range_is_checked_at_attach_and_by_the_health_check():
    from offlinerlkit import _engine
    c, data, orders = rc.epoch_inputs("rcsl_tiny", 1)
    big = dict(data); big["rtgs"] = data["rtgs"].copy(); big["rtgs"][7, 0] = 70000.0
    buf, ok = _buffer(big), _buffer(data)
    e1, _, _, batches = make_engine("rcsl_tiny", precision=1)
    e0, _, _, _ = make_engine("rcsl_tiny", precision=0)
    try:
        with pytest.raises(RuntimeError, match="returns-to-go"):
            e1.attach_buffer(buf)
        e1.attach_buffer(ok)
        e0.attach_buffer(buf)
        m, _ = e0.learn_epoch(orders[0])
        assert np.isfinite(m).all()
        # a teacher-forced batch beyond the range: the health check scans the net's input, rtg column included
        b = {k: v.copy() for k, v in batches[0].items()}
        b["rtgs"][3, 0] = 1.0e5
        with pytest.warns(_engine.EngineHealthWarning):
            e1.step(lead(b), [])
            flags = e1.health_check()
        assert flags[0] & _engine.HEALTH_SPLIT_RANGE
    finally:
        e1.close(); e0.close(); buf.close(); ok.close()


# ---- Python layer ------------------------------------------------------------------------------------------------------------------------

def _policy(c, lr=None):
    from offlinerlkit.modules import RcslModule
    from offlinerlkit.nets import MLP
    from offlinerlkit.policy import RcslPolicy
    mod = RcslModule(MLP(input_dim=c["obs_dim"] + 1, hidden_dims=c["hidden"], output_dim=c["act_dim"]), "cuda:0")
    return RcslPolicy(None, None, mod, torch.optim.Adam(mod.parameters(), lr=lr or c["lr"]), "cuda:0")


def test_policy_learn_matches_the_fixture_and_follows_lr_changes():
    c, net, batches = rc.case_inputs("rcsl_tiny")
    g = load_golden("rcsl_tiny")
    pol = _policy(c)
    pol.rcsl.load_state_dict({k: torch.from_numpy(v) for k, v in net.items()})
    for k, b in enumerate(batches[:2]):
        res = pol.learn(b)
        assert list(res) == ["loss"] and rel_err(np.array([res["loss"]]), g[f"step{k}/losses"], floor=1e-2) < 1e-4
    assert list(pol.state_dict().keys()) == [str(k) for k in g["keys"]]
    sd = {k[len("rcsl."):]: v.cpu().numpy() for k, v in pol.state_dict().items()}            # the modules alias the engine's arena
    check_state_against_golden(g, "state1", {"rcsl": sd}, atol=4e-6 * 2)
    pred, _, _ = orc.forward(sd, batches[2]["observations"], batches[2]["rtgs"])
    assert scale_err(pol.select_action(batches[2]["observations"], batches[2]["rtgs"]), pred) < 1e-4
    # a scheduler's new learning rate reaches the engine: with lr = 0 a step moves nothing
    pol.rcsl_optim.param_groups[0]["lr"] = 0.0
    before = {k: v.clone() for k, v in pol.state_dict().items()}
    pol.learn(batches[2])
    assert all(torch.equal(v, pol.state_dict()[k]) for k, v in before.items())
    # several runs: [R, B, ...] batches, per-run keys
    pol.rcsl_optim.param_groups[0]["lr"] = c["lr"]
    pol.set_engine_options(n_runs=2, seed=3)
    res = pol.learn(dict(observations=np.stack([batches[2]["observations"], batches[3]["observations"]]),
                         actions=np.stack([batches[2]["actions"], batches[3]["actions"]]), rtgs=np.stack([batches[2]["rtgs"], batches[3]["rtgs"]])))
    assert set(res) == {"loss", "run0/loss", "run1/loss"} and res["run0/loss"] != res["run1/loss"]
    acts = pol.select_action_runs(np.stack([batches[0]["observations"]] * 2), np.stack([batches[0]["rtgs"]] * 2))
    pol.select_run(1)
    assert scale_err(acts[1], pol.select_action(batches[0]["observations"], batches[0]["rtgs"])) < 1e-5


@pytest.fixture(scope="module")
def pm_task():
    return rc.pm_dataset()


@pytest.mark.parametrize("fused,n_runs", [(True, 1), (True, 4), (False, 1), (False, 4)])
def test_trainer_learns_return_conditioned_control(pm_task, tmp_path, fused, n_runs):
    """End to end on the point mass of rcsl_cases.py (mixed-quality data, 1500 episodes = 30 000 rows, 10 epochs of 118 batches of 256,
    [64, 64], lr 1e-3): after training, the return when conditioned on the dataset's best return exceeds both the return when
    conditioned on its worst return and the dataset's mean return -- for every run of the engine.
    The same data and schedule through the real reference RcslPolicy / RcslPolicyTrainer on the CPU (torch seeds 0, 1, 2): best-conditioned
    -1.67 / -1.73 / -1.59, worst-conditioned -113.4 / -106.6 / -122.4, dataset mean -43.9 (best episode -1.26, worst -145.9): 3 of 3;
    at 20 epochs -1.65 / -1.74 / -1.60 against -113.0 / -120.5 / -113.0."""
    from offlinerlkit.policy_trainer import RcslPolicyTrainer
    from offlinerlkit.utils.logger import Logger
    data, rets = pm_task
    best, worst, mean = float(rets.max()), float(rets.min()), float(rets.mean())
    torch.manual_seed(0)
    pol = _policy(dict(obs_dim=rc.PM_OD, act_dim=rc.PM_AD, hidden=rc.PM_HID), lr=rc.PM_LR)
    pol.set_engine_options(n_runs=n_runs, seed=5)
    logger = Logger(str(tmp_path), {"policy_training_progress": "csv"})
    tr = RcslPolicyTrainer(pol, rc.PointMassEnv(5), data, data, best, logger, 5, epoch=rc.PM_EPOCHS, batch_size=rc.PM_BATCH, offline_ratio=1,
                           eval_episodes=3, fused=fused)
    out = tr.train()
    assert np.isfinite(out["last_10_performance"])
    rows = [ln.split(",") for ln in open(tmp_path / "record" / "policy_training_progress.csv").read().strip().split("\n")]
    loss = [float(r[rows[0].index("loss")]) for r in rows[1:]]
    assert len(loss) == rc.PM_EPOCHS and np.isfinite(loss).all() and loss[-1] < loss[0]
    assert pol.engine.step_count() == rc.PM_EPOCHS * 118
    pol.eval()
    for r in range(n_runs):
        pol.select_run(r)
        hi, lo = rc.pm_return(pol.select_action, best), rc.pm_return(pol.select_action, worst)
        print(f"fused {fused} run {r}/{n_runs}: loss {loss[0]:.4f} -> {loss[-1]:.4f}; return conditioned on best {hi:.2f}, on worst {lo:.2f}; dataset mean {mean:.2f}")
        assert hi > lo and hi > mean, (r, hi, lo, mean)
