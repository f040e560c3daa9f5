"""GPU: Gaussian RCSL on the HIP engine (ORL_ALGO_RCSL_GAUSS, k_rcslg_head, RcslGaussianPolicy through RcslPolicyTrainer) against the numpy
oracle (tests/rcsl_gauss_oracle.py) and the fixtures of the real reference (tests/golden/make_rcsl_gauss_golden.py).

Bars: those of tests/test_gpu_rcsl.py -- loss 1e-4 (rel_err, floor 1e-2), ``mu`` / ``logvar`` 1e-4 of their scale, step-0 gradients at the
per-precision constants of tests/test_gpu_grads.py (head tensors included), post-step parameters by ``check_params`` there with its
absolute term scaled by lr / 3e-4.  make_rcsl_gauss_golden.py asserts that the oracle meets half the parameter bar against the reference
(measured: at most 6.7e-8 (k + 1) lr / 3e-4 absolute, 5.5e-11 mean, over all cases and tensors) and that no fixture value sits at the edge
of the clamp (rcsl_gauss_cases.py)."""
import numpy as np
import pytest
import torch

import rcsl_cases as rc
import rcsl_gauss_cases as gc
import rcsl_gauss_oracle as orc
from helpers import load_golden, rel_err, scale_err, check_state_against_golden
from test_gpu_grads import check_grads
from test_gpu_rcsl import check_params, lead, _buffer

pytestmark = pytest.mark.gpu
NET = 0      # ORL_NET_ACTOR


def make_engine(case, n_runs=1, precision=0, nets=None, **over):
    from offlinerlkit import _engine
    c, net, batches = gc.case_inputs(case)
    cfg = dict(obs_dim=c["obs_dim"], act_dim=c["act_dim"], hidden=c["hidden"], batch_size=c["B"], n_runs=n_runs, precision=precision,
               actor_lr=c["lr"])
    cfg.update(over)
    eng = _engine.Engine(_engine.default_config("rcsl_gauss", **cfg))
    for r in range(n_runs):
        eng.set_net(r, NET, nets[r] if nets is not None else net)
    return eng, c, net, batches


@pytest.mark.parametrize("case,precision", [(c, p) for c in gc.CASES for p in (0, 1)] + [("rcslg_tiny", 2)])
def test_rcslg_step(case, precision):
    """orl_step against the reference fixture and the oracle: loss, taps (z, mu, post-clamp logvar), step-0 gradient, parameters after
    every step; the net's tensor names are the reference's state_dict keys, heads last and unstacked"""
    eng, c, net, batches = make_engine(case, precision=precision)
    g = load_golden(case)
    st = orc.init_state(net)
    B, A = c["B"], c["act_dim"]
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
                x = eng.debug_read(0, "rcsl_x").reshape(B, c["obs_dim"] + 1)
                assert np.array_equal(x, aux["x"])
                z, mu, lv = (eng.debug_read(0, n).reshape(B, A) for n in ("z", "mu", "logvar"))
                print(f"  err / scale: z {scale_err(z, aux['z']):.2e} mu {scale_err(mu, aux['mu']):.2e} / {scale_err(mu, g['step0/mu']):.2e} "
                      f"logvar {scale_err(lv, aux['logvar']):.2e} / {scale_err(lv, g['step0/logvar']):.2e}")
                assert scale_err(z, aux["z"]) < 1e-4
                assert scale_err(mu, aux["mu"]) < 1e-4 and scale_err(mu, g["step0/mu"]) < 1e-4
                assert scale_err(lv, aux["logvar"]) < 1e-4 and scale_err(lv, g["step0/logvar"]) < 1e-4
                assert lv.min() >= gc.LO and lv.max() <= gc.HI
                if c["head"] == "clamp":
                    assert np.array_equal(lv == gc.LO, aux["raw"] < gc.LO) and np.array_equal(lv == gc.HI, aux["raw"] > gc.HI)
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
    eng, c, net, batches = make_engine("rcslg_hopper", n_runs=R, precision=precision)
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


def test_distinct_runs_follow_the_oracle():
    """16 runs with their own weights, heads and batches: every run follows its own oracle"""
    R, case = 16, "rcslg_odd"
    ins = [gc.case_inputs(case, run=r) for r in range(R)]
    eng, c, _, _ = make_engine(case, n_runs=R, nets=[i[1] for i in ins])
    states = [orc.init_state(i[1]) for i in ins]
    try:
        for k in range(gc.STEPS):
            bs = [i[2][k] for i in ins]
            m = eng.step(dict(observations=np.stack([b["observations"] for b in bs]), actions=np.stack([b["actions"] for b in bs]),
                              rewards=np.stack([b["rtgs"] for b in bs])), [])
            for r in range(R):
                res, _ = orc.learn(states[r], c, bs[r])
                assert rel_err(m[r], np.array([res["loss"]]), floor=1e-2) < 1e-4, (case, k, r, m[r], res)
        for r in (0, R - 1):
            check_params(eng.get_net(r, NET), states[r]["rcsl"], gc.STEPS - 1, c["lr"], (case, r))
    finally:
        eng.close()


@pytest.mark.parametrize("precision", [0, 1])
def test_learn_epoch_follows_the_order_and_masks_the_padding(precision):
    """rcslg_tiny, 3 runs, N = 3 B + 5: four steps, the last with 5 valid rows.  Epoch 1 step by step (``order`` slices): loss and
    parameters follow the oracle fed the valid rows only, and the tail loss is NOT the loss over all B gathered rows (the generator
    asserts on the reference that the two differ by more than 1e-3).  The same epoch in ONE call on a twin engine, from a host order and
    from a device-resident one: parameters bit for bit those of the stepwise engine.  A second epoch with a new order reuses the graph
    and still follows the oracle."""
    R = 3
    c, data, orders = gc.epoch_inputs(R)
    B = c["B"]
    eng, _, net, _ = make_engine("rcslg_tiny", n_runs=R, precision=precision)
    whole, _, _, _ = make_engine("rcslg_tiny", n_runs=R, precision=precision)
    ondev, _, _, _ = make_engine("rcslg_tiny", n_runs=R, precision=precision)
    buf = _buffer(data)
    states = [orc.init_state(net) for _ in range(R)]
    try:
        for e in (eng, whole, ondev):
            e.attach_buffer(buf)
        per_step = []
        for s in range(4):
            sl = orders[0][:, s * B:(s + 1) * B]
            m, _ = eng.learn_epoch(sl)
            per_step.append(m.copy())
            assert eng.step_count() == s + 1
            for r in range(R):
                valid = sl[r] >= 0
                assert valid.sum() == (B if s < 3 else 5)
                want = rc.gather(data, sl[r])
                assert np.array_equal(eng.debug_read(r, "b_act").reshape(B, -1), want["actions"])
                if s == 3:
                    all_rows, _ = orc.learn(orc.init_state(states[r]["rcsl"]), c, want)          # what an unmasked kernel would report
                res, aux = orc.learn(states[r], c, {k: v[valid] for k, v in want.items()})
                print(f"precision {precision} step {s} run {r}: loss {m[r, 0]:.6g} oracle (valid rows) {res['loss']:.6g}")
                assert rel_err(m[r], np.array([res["loss"]]), floor=1e-2) < 1e-4, (s, r, m[r], res)
                if s == 3:
                    assert abs(m[r, 0] - all_rows["loss"]) > 1e-3 * abs(res["loss"]), (r, m[r, 0], all_rows["loss"], res["loss"])
                    mu = eng.debug_read(r, "mu").reshape(B, -1)
                    assert scale_err(mu[valid], aux["mu"]) < 1e-4
                check_params(eng.get_net(r, NET), states[r]["rcsl"], s, c["lr"], (s, r))
        mw, ms = whole.learn_epoch(orders[0])
        assert ms > 0 and whole.step_count() == 4
        assert np.allclose(mw, np.mean(per_step, axis=0), rtol=1e-6, atol=0), (mw, np.mean(per_step, axis=0))
        o1 = torch.as_tensor(orders[0], device="cuda:0")
        torch.cuda.synchronize()
        md, _ = ondev.learn_epoch((o1.data_ptr(), o1.shape[1]), on_device=True)
        assert np.array_equal(md, mw)
        for r in range(R):
            a, b, d = eng.get_net(r, NET), whole.get_net(r, NET), ondev.get_net(r, NET)
            for pn in a:
                assert np.array_equal(a[pn], b[pn]) and np.array_equal(a[pn], d[pn]), (r, pn)
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
        # RCSL's refusals hold for this algorithm id too
        from offlinerlkit import _engine
        ring = _engine.DeviceBuffer(c["obs_dim"], c["act_dim"]); ring.reserve(64)
        with pytest.raises(RuntimeError, match="RCSL"):
            whole.attach_model_buffer(ring, 4)
        ring.close()
        with pytest.raises(RuntimeError, match="multiple of batch_size"):
            whole.learn_epoch(orders[0][:, :3 * B + 5])
        assert whole.step_count() == 8
    finally:
        eng.close(); whole.close(); ondev.close(); buf.close()


# ---- Python layer ------------------------------------------------------------------------------------------------------------------------

def _policy(c, lr=None):
    from offlinerlkit.modules import DiagGaussian, RcslGaussianModule
    from offlinerlkit.nets import MLP
    from offlinerlkit.policy import RcslGaussianPolicy
    A = c["act_dim"]
    mod = RcslGaussianModule(MLP(input_dim=c["obs_dim"] + 1, hidden_dims=c["hidden"], output_dim=A),
                             DiagGaussian(A, A, unbounded=True, conditioned_sigma=True), "cuda:0")
    return RcslGaussianPolicy(None, None, mod, torch.optim.Adam(mod.parameters(), lr=lr or c["lr"]), "cuda:0")


def test_policy_learn_matches_the_fixture_and_follows_lr_changes():
    c, net, batches = gc.case_inputs("rcslg_tiny")
    g = load_golden("rcslg_tiny")
    pol = _policy(c)
    pol.rcsl.load_state_dict({k: torch.from_numpy(v) for k, v in net.items()})
    for k, b in enumerate(batches[:2]):
        res = pol.learn(b)
        assert list(res) == ["loss"] and rel_err(np.array([res["loss"]]), g[f"step{k}/losses"], floor=1e-2) < 1e-4
    assert list(pol.state_dict().keys()) == [str(k) for k in g["keys"]]
    sd = {k[len("rcsl."):]: v.cpu().numpy() for k, v in pol.state_dict().items()}            # the modules alias the engine's arena
    check_state_against_golden(g, "state1", {"rcsl": sd}, atol=4e-6 * 2)
    b = batches[2]
    mu, logvar, _ = orc.forward(sd, b["observations"], b["rtgs"])
    with torch.no_grad():
        pm, pl = pol.rcsl.get_dist_params(b["observations"], b["rtgs"])
    assert scale_err(pm.cpu().numpy(), mu) < 1e-4 and scale_err(pl.cpu().numpy(), logvar) < 1e-4
    # select_action samples Normal(mu, exp(head output)): under one seed, mu + exp(logvar) * randn
    torch.manual_seed(11)
    a = pol.select_action(b["observations"], b["rtgs"])
    torch.manual_seed(11)
    want = mu + np.exp(logvar) * torch.randn(mu.shape, device="cuda:0").cpu().numpy()
    assert scale_err(a, want) < 1e-5
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
    obs2, rtg2 = np.stack([batches[0]["observations"]] * 2), np.stack([batches[0]["rtgs"]] * 2)
    acts = pol.select_action_runs(obs2, rtg2, deterministic=True)
    pol.select_run(1)
    with torch.no_grad():
        mu1, lv1 = pol.rcsl.get_dist_params(batches[0]["observations"], batches[0]["rtgs"])
    assert scale_err(acts[1], mu1.cpu().numpy()) < 1e-5
    assert not np.array_equal(acts[0], acts[1])
    torch.manual_seed(5)
    sampled = pol.select_action_runs(obs2, rtg2)
    assert sampled.shape == acts.shape and np.all(np.abs(sampled - acts)[1] <= 6.0 * np.exp(lv1.cpu().numpy()) + 1e-6)
    assert not np.array_equal(sampled, acts)


@pytest.fixture(scope="module")
def pm_task():
    return rc.pm_dataset()


PM_EPOCHS = 20


@pytest.mark.parametrize("fused,n_runs", [(True, 1), (True, 4), (False, 1), (False, 4)])
def test_trainer_learns_return_conditioned_control(pm_task, tmp_path, fused, n_runs):
    """End to end on the point mass of rcsl_cases.py (mixed-quality data, 1500 episodes = 30 000 rows, 20 epochs of 118 batches of 256,
    [64, 64], lr 1e-3) through RcslPolicyTrainer: after training, the SAMPLED return when conditioned on the dataset's best return exceeds
    both the return when conditioned on its worst return and the dataset's mean return (-43.9) -- for every run of the engine.
    The same data and schedule through the real reference RcslGaussianPolicy on the CPU (torch seeds 0, 1, 2), best- / worst-conditioned:
      20 epochs  -19.5 / -2.1 / -2.0   against  -105.9 / -115.2 / -116.3   3 of 3
      10 epochs  -27.2 / -2.4 / -2.7   against   -96.4 / -103.7 / -112.9   3 of 3, seed 0's margin over the mean is thin: hence 20.
    The outcome depends on the initialisation far more than on the batch order: in the reference some initialisations (torch seed 0 is
    one) settle at an epoch loss near -1.0 and a best-conditioned return of -17 .. -31, the others near -1.3 and -2.  The seeds below
    were therefore chosen on the REFERENCE, not on the engine: torch seed 1 (run 0) and engine seed 7 (the initialisations of runs 1 - 3,
    ``_fresh_run_params``), each trained by the real reference policy on the CPU under two batch orders and sampled under two seeds,
    gave best-conditioned -2.1 .. -7.7 / -5.1 .. -8.6 / -2.2 .. -2.5 / -1.8 .. -2.0 against worst-conditioned -108 .. -122."""
    from offlinerlkit.policy_trainer import RcslPolicyTrainer
    from offlinerlkit.utils.logger import Logger
    data, rets = pm_task
    best, worst, mean = float(rets.max()), float(rets.min()), float(rets.mean())
    torch.manual_seed(1)
    pol = _policy(dict(obs_dim=rc.PM_OD, act_dim=rc.PM_AD, hidden=rc.PM_HID), lr=rc.PM_LR)
    pol.set_engine_options(n_runs=n_runs, seed=7)
    logger = Logger(str(tmp_path), {"policy_training_progress": "csv"})
    tr = RcslPolicyTrainer(pol, rc.PointMassEnv(5), data, data, best, logger, 5, epoch=PM_EPOCHS, batch_size=rc.PM_BATCH, offline_ratio=1,
                           eval_episodes=3, fused=fused)
    out = tr.train()
    assert np.isfinite(out["last_10_performance"])
    rows = [ln.split(",") for ln in open(tmp_path / "record" / "policy_training_progress.csv").read().strip().split("\n")]
    loss = [float(r[rows[0].index("loss")]) for r in rows[1:]]
    assert len(loss) == PM_EPOCHS and np.isfinite(loss).all() and loss[-1] < loss[0]
    assert pol.engine.step_count() == PM_EPOCHS * 118
    pol.eval()
    torch.manual_seed(1)
    for r in range(n_runs):
        pol.select_run(r)
        hi, lo = rc.pm_return(pol.select_action, best), rc.pm_return(pol.select_action, worst)
        print(f"fused {fused} run {r}/{n_runs}: loss {loss[0]:.4f} -> {loss[-1]:.4f}; return conditioned on best {hi:.2f}, on worst {lo:.2f}; dataset mean {mean:.2f}")
        assert hi > lo and hi > mean, (r, hi, lo, mean)
