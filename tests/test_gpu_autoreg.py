"""GPU: the autoregressive behaviour policy on the HIP engine (ORL_ALGO_AUTOREG: k_autoreg_prepare, the LeakyReLU flavours of the tiled
GEMM, k_autoreg_head, orl_autoreg_sample / k_autoreg_draw, AutoregressivePolicy through RcslPolicyTrainer, ``rollout``) against the numpy
oracle (tests/autoreg_oracle.py) and the fixtures of the real reference (tests/golden/make_autoreg_golden.py).

Bars: those of tests/test_gpu_rcsl.py -- loss 1e-4 (rel_err, floor 1e-2), taps 1e-4 of their scale (the expanded input and the targets
exactly), step-0 gradients at the per-precision constants of tests/test_gpu_grads.py, post-step parameters by ``check_params`` there and
``check_state_against_golden`` with atol = 4e-6 (k + 1) lr / 3e-4; sampling 1e-5 of scale.  make_autoreg_golden.py asserts that the oracle
meets half the parameter bar against the reference (measured: at most 4.7e-8 (k + 1) lr / 3e-4 absolute, 2.3e-10 mean, over all cases
and tensors) and that no fixture value of a case compared in full sits at the kink of the output LeakyReLU (autoreg_cases.py)."""
import numpy as np
import pytest
import torch

import autoreg_cases as ac
import autoreg_oracle as orc
from helpers import load_golden, rel_err, scale_err, check_state_against_golden
from test_gpu_grads import check_grads
from test_gpu_rcsl import check_params, _buffer

pytestmark = pytest.mark.gpu
NET = 0      # ORL_NET_ACTOR


def make_engine(case, n_runs=1, precision=0, nets=None, **over):
    from offlinerlkit import _engine
    c, net, batches = ac.case_inputs(case)
    cfg = dict(obs_dim=c["obs_dim"], act_dim=c["act_dim"], hidden=c["hidden"], batch_size=c["B"], n_runs=n_runs, precision=precision,
               actor_lr=c["lr"])
    cfg.update(over)
    eng = _engine.Engine(_engine.default_config("autoreg", **cfg))
    for r in range(n_runs):
        eng.set_net(r, NET, nets[r] if nets is not None else net)
    return eng, c, net, batches


def lead(b, R=1):
    """no return-to-go: orl_batch.rewards stays NULL"""
    return dict(observations=np.stack([b["observations"]] * R), actions=np.stack([b["actions"]] * R))


@pytest.mark.parametrize("case,precision", [(c, p) for c in ac.CASES for p in (0, 1)] + [("ar_tiny", 2), ("ar_ws", 2)])
def test_autoreg_step(case, precision):
    """orl_step against the reference fixture and the oracle: loss, taps (the expanded input and targets exactly; mean / logstd), step-0
    gradient, parameters after every step; the net's tensor names are the reference's state_dict keys"""
    eng, c, net, batches = make_engine(case, precision=precision)
    g = load_golden(case)
    st = orc.init_state(net)
    B, A, od = c["B"], c["act_dim"], c["obs_dim"]
    try:
        assert eng.metric_names == ["loss"] == [str(k) for k in g["loss_keys"]]
        assert [n for n, _, _ in eng.net_tensors(NET)] == [str(k) for k in g["keys"]]
        worst = 0.0
        for k, b in enumerate(batches):
            res, aux = orc.learn(st, c, b)
            m = eng.step(lead(b), [])[0]
            print(f"{case} precision {precision} step {k}: loss {m[0]:.6g} oracle {res['loss']:.6g} reference {g[f'step{k}/losses'][0]:.6g}")
            assert rel_err(m, np.array([res["loss"]]), floor=1e-2) < 1e-4, (case, k, m, res)
            assert rel_err(m, g[f"step{k}/losses"], floor=1e-2) < 1e-4, (case, k, m, g[f"step{k}/losses"])
            if k == 0:
                x = eng.debug_read(0, "ar_x").reshape(A * B, od + 2 * A)
                assert np.array_equal(x, aux["x"])
                assert np.array_equal(eng.debug_read(0, "ar_target").reshape(A * B), aux["target"])
                out = eng.debug_read(0, "ar_out").reshape(A * B, 2)
                mean, ls = out[:, 0], out[:, 1]
                print(f"  err / scale: mean {scale_err(mean, aux['mean']):.2e} / {scale_err(mean, g['step0/mean']):.2e} "
                      f"logstd {scale_err(ls, aux['logstd']):.2e} / {scale_err(ls, g['step0/logstd']):.2e}")
                assert scale_err(mean, aux["mean"]) < 1e-4 and scale_err(mean, g["step0/mean"]) < 1e-4
                assert scale_err(ls, aux["logstd"]) < 1e-4 and scale_err(ls, g["step0/logstd"]) < 1e-4
                assert (out > 0).any(axis=0).all() and (out < 0).any(axis=0).all()      # both branches of the output LeakyReLU
                report = []
                check_grads(eng, 0, NET, aux["grads"], (case, precision), precision, report)
                print(f"  step-0 gradients vs oracle: worst max/scale {max(x[2] for x in report):.2e}, worst rel L2 {max(x[3] for x in report):.2e}")
                if "step0/grads/model.0.weight" in g.files:
                    report = []
                    check_grads(eng, 0, NET, {n: g[f"step0/grads/{n}"] for n in net}, (case, precision, "reference"), precision, report)
            got = eng.get_net(0, NET)
            check_state_against_golden(g, f"state{k}", {"model": got}, atol=4e-6 * (k + 1) * c["lr"] / 3e-4)
            worst = max(worst, check_params(got, st["model"], k, c["lr"], case))
        print(f"{case} precision {precision}: worst parameter error vs oracle, over lr / 3e-4: {worst:.2e}")
    finally:
        eng.close()


@pytest.mark.parametrize("precision", [0, 1, 2])
def test_identical_runs_stay_bit_identical(precision):
    """16 runs of ar_ws: 4096 batched rows of [256, 256], where the ReLU-only weight-stationary launches would otherwise be picked"""
    R = 16
    eng, c, net, batches = make_engine("ar_ws", n_runs=R, precision=precision)
    st = orc.init_state(net)
    try:
        for k, b in enumerate(batches):
            m = eng.step(lead(b, R), [])
            res, _ = orc.learn(st, c, b)
            assert rel_err(m[0], np.array([res["loss"]]), floor=1e-2) < 1e-4, (k, m[0], res)
            for r in range(1, R):
                assert np.array_equal(m[0], m[r]), (k, r, m[0], m[r])
        a = eng.get_net(0, NET)
        check_params(a, st["model"], ac.STEPS - 1, c["lr"], "ar_ws x 16")
        for r in (1, R // 2, R - 1):
            b1 = eng.get_net(r, NET)
            for pn in a:
                assert np.array_equal(a[pn], b1[pn]), (pn, r)
    finally:
        eng.close()


def test_distinct_runs_follow_the_oracle():
    """16 runs with their own weights and batches: every run follows its own oracle"""
    R, case = 16, "ar_odd"
    ins = [ac.case_inputs(case, run=r) for r in range(R)]
    eng, c, _, _ = make_engine(case, n_runs=R, nets=[i[1] for i in ins])
    states = [orc.init_state(i[1]) for i in ins]
    try:
        for k in range(ac.STEPS):
            bs = [i[2][k] for i in ins]
            m = eng.step(dict(observations=np.stack([b["observations"] for b in bs]), actions=np.stack([b["actions"] for b in bs])), [])
            for r in range(R):
                res, _ = orc.learn(states[r], c, bs[r])
                assert rel_err(m[r], np.array([res["loss"]]), floor=1e-2) < 1e-4, (case, k, r, m[r], res)
        for r in (0, R - 1):
            check_params(eng.get_net(r, NET), states[r]["model"], ac.STEPS - 1, c["lr"], (case, r))
    finally:
        eng.close()


@pytest.mark.parametrize("precision", [0, 1])
def test_learn_epoch_follows_the_order_and_masks_the_padding(precision):
    """ar_tiny, 3 runs, N = 3 B + 5: four steps, the last with 5 valid rows.  Epoch 1 step by step (``order`` slices): loss and
    parameters follow the oracle fed the valid rows only, and the tail loss is NOT the loss over all B gathered rows (the generator
    asserts on the reference that the two differ by more than 1e-3).  The same epoch in ONE call on a twin engine, from a host order and
    from a device-resident one: parameters bit for bit those of the stepwise engine.  A second epoch with a new order reuses the graph
    and still follows the oracle."""
    R = 3
    c, data, orders = ac.epoch_inputs(R)
    B, A = c["B"], c["act_dim"]
    eng, _, net, _ = make_engine("ar_tiny", n_runs=R, precision=precision)
    whole, _, _, _ = make_engine("ar_tiny", n_runs=R, precision=precision)
    ondev, _, _, _ = make_engine("ar_tiny", n_runs=R, precision=precision)
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
                want = ac.gather(data, sl[r])
                assert np.array_equal(eng.debug_read(r, "b_act").reshape(B, -1), want["actions"])
                assert np.array_equal(eng.debug_read(r, "ar_x").reshape(A * B, -1), orc.expand(want["observations"], want["actions"])[0])
                if s == 3:
                    all_rows, _ = orc.learn(orc.init_state(states[r]["model"]), c, want)          # what an unmasked kernel would report
                res, aux = orc.learn(states[r], c, {k: v[valid] for k, v in want.items()})
                print(f"precision {precision} step {s} run {r}: loss {m[r, 0]:.6g} oracle (valid rows) {res['loss']:.6g}")
                assert rel_err(m[r], np.array([res["loss"]]), floor=1e-2) < 1e-4, (s, r, m[r], res)
                if s == 3:
                    assert abs(m[r, 0] - all_rows["loss"]) > 1e-3 * abs(res["loss"]), (r, m[r, 0], all_rows["loss"], res["loss"])
                    mean = eng.debug_read(r, "ar_out").reshape(A, B, 2)[:, valid, 0].reshape(-1)
                    assert scale_err(mean, aux["mean"]) < 1e-4
                check_params(eng.get_net(r, NET), states[r]["model"], s, c["lr"], (s, r))
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
                res, _ = orc.learn(states[r], c, ac.gather(data, idx[idx >= 0]))
                tot[r] += res["loss"] / 4
        assert rel_err(m2[:, 0], tot, floor=1e-2) < 1e-4, (m2, tot)
        for r in range(R):
            check_params(whole.get_net(r, NET), states[r]["model"], 7, c["lr"], ("epoch 2", r))
        # RCSL's refusals hold for this algorithm id too, with their messages
        from offlinerlkit import _engine
        ring = _engine.DeviceBuffer(c["obs_dim"], c["act_dim"]); ring.reserve(64)
        with pytest.raises(RuntimeError, match="not available for RCSL engines"):
            whole.attach_model_buffer(ring, 4)
        ring.close()
        with pytest.raises(RuntimeError, match="multiple of batch_size"):
            whole.learn_epoch(orders[0][:, :3 * B + 5])
        assert whole.step_count() == 8
    finally:
        eng.close(); whole.close(); ondev.close(); buf.close()


def test_learn_n_draws_from_the_attached_buffer():
    """orl_learn_n: two steps on device-drawn rows; the batch slots and the expanded input are consistent with the drawn rows"""
    c, data, _ = ac.epoch_inputs(1)
    B, A, od = c["B"], c["act_dim"], c["obs_dim"]
    eng, _, net, _ = make_engine("ar_tiny", n_runs=2)
    buf = _buffer(data)
    try:
        eng.attach_buffer(buf)
        before = eng.get_net(0, NET)
        m, ms = eng.learn_n(2)
        assert eng.step_count() == 2 and np.isfinite(m).all() and ms > 0
        assert any(not np.array_equal(before[k], v) for k, v in eng.get_net(0, NET).items())
        for r in range(2):
            bo, ba = eng.debug_read(r, "b_obs").reshape(B, od), eng.debug_read(r, "b_act").reshape(B, A)
            # every drawn row is a row of the dataset, observation and action of the SAME row
            for i in range(B):
                j = np.flatnonzero((data["observations"] == bo[i]).all(axis=1))
                assert len(j) == 1 and np.array_equal(data["actions"][j[0]], ba[i]), (r, i)
            x, t = orc.expand(bo, ba)
            assert np.array_equal(eng.debug_read(r, "ar_x").reshape(A * B, -1), x)
            assert np.array_equal(eng.debug_read(r, "ar_target").reshape(-1), t)
        assert not np.array_equal(eng.debug_read(0, "b_obs"), eng.debug_read(1, "b_obs"))
    finally:
        eng.close(); buf.close()


def test_teacher_forced_sampling_matches_the_reference_and_moves_nothing():
    g = load_golden("ar_sample")
    for case in ac.SAMPLE_CASES:
        eng, c, net, batches = make_engine(case)
        try:
            obs, eps = ac.sample_obs(case), g[f"{case}/eps"]
            m0 = eng.step(lead(batches[0]), [])[0]
            p0 = eng.get_net(0, NET)
            a = eng.autoreg_sample(obs[None], eps[None])[0]
            want = orc.sample(p0, obs, eps)
            assert scale_err(a, want) < 1e-5, (case, scale_err(a, want))
            assert all(np.array_equal(v, eng.get_net(0, NET)[k]) for k, v in p0.items()) and eng.step_count() == 1
            # against the reference's own one-row select_action: a twin engine that has not stepped
            twin, _, _, _ = make_engine(case)
            try:
                ar = twin.autoreg_sample(obs[None], eps[None])[0]
                print(f"{case}: sampled actions vs reference {scale_err(ar, g[f'{case}/actions']):.2e}, vs oracle {scale_err(ar, orc.sample(net, obs, eps)):.2e}")
                assert scale_err(ar, g[f"{case}/actions"]) < 1e-5 and scale_err(ar, orc.sample(net, obs, eps)) < 1e-5
            finally:
                twin.close()
            # a learn step after sampling is the step a never-sampling engine takes
            m1 = eng.step(lead(batches[1]), [])[0]
            st = orc.init_state(net)
            orc.learn(st, c, batches[0])
            res, _ = orc.learn(st, c, batches[1])
            assert rel_err(m1, np.array([res["loss"]]), floor=1e-2) < 1e-4 and eng.step_count() == 2
            check_params(eng.get_net(0, NET), st["model"], 1, c["lr"], case)
        finally:
            eng.close()
    # n grows between calls, 3 runs with distinct nets
    R, case = 3, "ar_odd"
    ins = [ac.case_inputs(case, run=r) for r in range(R)]
    eng, c, _, _ = make_engine(case, n_runs=R, nets=[i[1] for i in ins])
    rng = np.random.RandomState(9)
    try:
        for n in (1, 5, 70):
            obs = rng.standard_normal((R, n, c["obs_dim"])).astype(np.float32)
            eps = rng.standard_normal((R, n, c["act_dim"])).astype(np.float32)
            a = eng.autoreg_sample(obs, eps)
            for r in range(R):
                assert scale_err(a[r], orc.sample(ins[r][1], obs[r], eps[r])) < 1e-5, (n, r)
    finally:
        eng.close()
    # refused on any other algorithm
    from offlinerlkit import _engine
    other = _engine.Engine(_engine.default_config("rcsl", obs_dim=5, act_dim=2, hidden=[32, 32], batch_size=16))
    try:
        with pytest.raises(RuntimeError, match="not an AUTOREG engine"):
            other.autoreg_sample(np.zeros((1, 1, 5), np.float32))
    finally:
        other.close()


def _fixed_gaussian_net(c):
    """output weights zero, biases (0.3, 100 ln 0.5): leaky gives mean 0.3, logstd ln 0.5 -- every conditional is N(0.3, 0.5^2) exactly"""
    net, _ = ac.make_net(c)
    n = 2 * len(c["hidden"])
    net[f"model.{n}.weight"][:] = 0
    net[f"model.{n}.bias"][:] = [0.3, 100.0 * np.log(0.5)]
    return net


def test_device_drawn_sampling_has_the_right_moments_and_streams():
    from offlinerlkit import _engine
    c = dict(obs_dim=5, act_dim=4, hidden=[32, 32], B=16, lr=3e-4, seed=91)
    net = _fixed_gaussian_net(c)
    n, A = 4096, 4

    def engine():
        e = _engine.Engine(_engine.default_config("autoreg", obs_dim=5, act_dim=A, hidden=c["hidden"], batch_size=16, n_runs=2, seed=12))
        for r in range(2):
            e.set_net(r, NET, net)
        return e
    obs = np.random.RandomState(2).standard_normal((2, n, 5)).astype(np.float32)
    eng = engine()
    try:
        a1 = eng.autoreg_sample(obs)
        a2 = eng.autoreg_sample(obs)
    finally:
        eng.close()
    N = n * A
    for a in (a1[0], a1[1], a2[0]):
        print(f"device-drawn samples: mean {a.mean():.4f} (0.3), std {a.std():.4f} (0.5)")
        assert abs(a.mean() - 0.3) < 5 * 0.5 / np.sqrt(N) and abs(a.std() - 0.5) < 5 * 0.5 / np.sqrt(2 * N)
    assert not np.array_equal(a1, a2) and not np.array_equal(a1[0], a1[1])
    fresh = engine()
    try:
        assert np.array_equal(fresh.autoreg_sample(obs), a1)
    finally:
        fresh.close()


# ---- Python layer ------------------------------------------------------------------------------------------------------------------------

def _policy(c, lr=None):
    from offlinerlkit.policy import AutoregressivePolicy
    return AutoregressivePolicy(c["obs_dim"], c["act_dim"], list(c["hidden"]), lr or c["lr"], "cuda:0")


def test_policy_learn_select_action_and_runs():
    c, net, batches = ac.case_inputs("ar_tiny")
    g = load_golden("ar_tiny")
    A = c["act_dim"]
    pol = _policy(c)
    pol.load_state_dict({k: torch.from_numpy(v) for k, v in net.items()})
    for k, b in enumerate(batches[:2]):
        res = pol.learn(b)
        assert list(res) == ["loss"] and rel_err(np.array([res["loss"]]), g[f"step{k}/losses"], floor=1e-2) < 1e-4
    assert list(pol.state_dict().keys()) == [str(k) for k in g["keys"]]
    sd = {k: v.cpu().numpy() for k, v in pol.state_dict().items()}            # the module aliases the engine's arena
    check_state_against_golden(g, "state1", {"model": sd}, atol=4e-6 * 2)
    with torch.no_grad():
        fit = float(pol.fit(torch.as_tensor(batches[2]["observations"], device="cuda:0"), torch.as_tensor(batches[2]["actions"], device="cuda:0")))
    assert rel_err(np.array([fit]), g["step2/losses"], floor=1e-2) < 1e-4
    # select_action: under one seed, the oracle fed torch.randn((n, A)) of the device generator
    obs = np.random.RandomState(4).standard_normal((16, c["obs_dim"])).astype(np.float32)
    torch.manual_seed(11)
    a = pol.select_action(obs, None)
    torch.manual_seed(11)
    want = orc.sample(sd, obs, torch.randn((16, A), device="cuda:0").cpu().numpy())
    assert a.shape == (16, A) and scale_err(a, want) < 1e-5
    assert scale_err(pol.select_action(obs[:1]), want[:1]) > 1e-3      # (another draw)
    # a scheduler's new learning rate reaches the engine: with lr = 0 a step moves nothing
    pol.rcsl_optim.param_groups[0]["lr"] = 0.0
    before = {k: v.clone() for k, v in pol.state_dict().items()}
    pol.learn(batches[2])
    assert all(torch.equal(v, pol.state_dict()[k]) for k, v in before.items())
    # several runs: [R, B, ...] batches, per-run keys; run 1 starts from a fresh initialisation
    pol.rcsl_optim.param_groups[0]["lr"] = c["lr"]
    pol.set_engine_options(n_runs=2, seed=3)
    res = pol.learn(dict(observations=np.stack([batches[2]["observations"], batches[3]["observations"]]),
                         actions=np.stack([batches[2]["actions"], batches[3]["actions"]]), rtgs=np.stack([batches[2]["rtgs"], batches[3]["rtgs"]])))
    assert set(res) == {"loss", "run0/loss", "run1/loss"} and res["run0/loss"] != res["run1/loss"]
    sd0, sd1 = pol.run_state_dict(0), pol.run_state_dict(1)
    assert all(not torch.equal(sd0[k], sd1[k]) for k in sd0)
    obs2 = np.stack([obs, obs])
    torch.manual_seed(5)
    acts = pol.select_action_runs(obs2)
    torch.manual_seed(5)
    eps = torch.randn((2, 16, A), device="cuda:0").cpu().numpy()
    for r in range(2):
        assert scale_err(acts[r], orc.sample({k: v.cpu().numpy() for k, v in (sd0, sd1)[r].items()}, obs, eps[r])) < 1e-5
        pol.select_run(r)
        torch.manual_seed(6)
        one = pol.select_action(obs)
        torch.manual_seed(6)
        assert scale_err(one, orc.sample({k: v.cpu().numpy() for k, v in (sd0, sd1)[r].items()}, obs, torch.randn((16, A), device="cuda:0").cpu().numpy())) < 1e-5
    assert not np.array_equal(acts[0], acts[1])
    # row r of select_action_runs is select_run(r); select_action under the draws of that row
    pol.select_run(1)
    # a policy that has never learned binds an engine on its first select_action
    fresh = _policy(c)
    assert fresh.engine is None and fresh.select_action(obs[:3]).shape == (3, A) and fresh.engine is not None


CORR_EPOCHS, CORR_BAR = 10, -0.31


@pytest.mark.parametrize("fused,n_runs", [(True, 1), (True, 4), (False, 1), (False, 4)])
def test_trainer_learns_correlated_action_dimensions(tmp_path, fused, n_runs):
    """End to end through RcslPolicyTrainer on autoreg_cases.corr_dataset (8192 rows, obs = noise, a0 ~ N(0, 1), a1 = -a0 + 0.1 N(0, 1)),
    [64, 64], lr 1e-3, batch 256, 10 epochs of 32 batches: the correlation of 2000 SAMPLED action pairs is strongly negative -- the
    conditioning of dimension 1 on the sampled dimension 0 is real; a head with one Gaussian per dimension would give about 0 -- and the
    epoch loss falls, for every run of the engine.
    The same data and schedule through the real reference AutoregressivePolicy on the CPU (torch seeds 0, 1, 2), one-row select_action
    on the first 2000 observations:
      10 epochs  loss 1.333 -> 1.217 / 1.329 -> 1.166 / 1.343 -> 1.206   corr -0.412 / -0.512 / -0.492
       5 epochs                                                          corr -0.369 / -0.442 / -0.449
    (The reference's LeakyReLU behind the output layer keeps logstd above 0.01 z, so the conditional std stays near 1 and the correlation
    well short of the data's -0.995: that is the reference's model, reproduced.)  Bar: the weakest of the three, -0.412, relaxed by the
    spread between them, 0.100: corr < -0.31."""
    from offlinerlkit.policy_trainer import RcslPolicyTrainer
    from offlinerlkit.utils.logger import Logger
    import rcsl_cases as rc
    data = ac.corr_dataset()
    torch.manual_seed(1)
    pol = _policy(dict(obs_dim=ac.C_OD, act_dim=ac.C_AD, hidden=ac.C_HID), lr=ac.C_LR)
    pol.set_engine_options(n_runs=n_runs, seed=7)
    logger = Logger(str(tmp_path), {"policy_training_progress": "csv"})

    class Env(rc.PointMassEnv):      # (the trainer evaluates every epoch: three short episodes of the point mass, any actions)
        pass
    tr = RcslPolicyTrainer(pol, Env(5), data, data, 0.0, logger, 5, epoch=CORR_EPOCHS, batch_size=ac.C_BATCH, offline_ratio=1,
                           eval_episodes=1, fused=fused)
    out = tr.train()
    assert np.isfinite(out["last_10_performance"])
    rows = [ln.split(",") for ln in open(tmp_path / "record" / "policy_training_progress.csv").read().strip().split("\n")]
    loss = [float(r[rows[0].index("loss")]) for r in rows[1:]]
    assert len(loss) == CORR_EPOCHS and np.isfinite(loss).all() and loss[-1] < loss[0]
    assert pol.engine.step_count() == CORR_EPOCHS * 32
    pol.eval()
    torch.manual_seed(1)
    for r in range(n_runs):
        pol.select_run(r)
        a = pol.select_action(data["observations"][:2000])
        corr = float(np.corrcoef(a[:, 0], a[:, 1])[0, 1])
        print(f"fused {fused} run {r}/{n_runs}: loss {loss[0]:.4f} -> {loss[-1]:.4f}; corr(a0, a1) of 2000 samples {corr:.3f}")
        assert corr < CORR_BAR, (r, corr)


def test_rollout_on_the_device_objects():
    """RcslPolicy(dynamics, AutoregressivePolicy).rollout with a small real EnsembleDynamics"""
    from offlinerlkit.dynamics import EnsembleDynamics
    from offlinerlkit.modules import EnsembleDynamicsModel, RcslModule
    from offlinerlkit.nets import MLP
    from offlinerlkit.policy import RcslPolicy
    from offlinerlkit.utils.scaler import StandardScaler
    from offlinerlkit.utils.termination_fns import get_termination_fn
    od, ad = 11, 3
    torch.manual_seed(2)
    model = EnsembleDynamicsModel(obs_dim=od, action_dim=ad, hidden_dims=[16, 16], num_ensemble=3, num_elites=2, weight_decays=[2.5e-5, 5e-5, 7.5e-5],
                                  device="cuda:0")
    scaler = StandardScaler(mu=np.zeros((1, od + ad), np.float32), std=np.ones((1, od + ad), np.float32))
    dyn = EnsembleDynamics(model, torch.optim.Adam(model.parameters(), lr=1e-3), scaler, get_termination_fn("hopper-medium-v2"))
    data = dict(observations=np.random.RandomState(3).standard_normal((32, od)).astype(np.float32))
    beh = _policy(dict(obs_dim=od, act_dim=ad, hidden=[32, 32]), lr=1e-3)
    mod = RcslModule(MLP(input_dim=od + 1, hidden_dims=[16, 16], output_dim=ad), "cuda:0")
    pol = RcslPolicy(dyn, beh, mod, torch.optim.Adam(mod.parameters(), lr=1e-3), "cuda:0")
    init = data["observations"][:32].copy()
    init[:, 0] = 1.0; init[:, 1] = 0.0      # (a healthy hopper: height 1, angle 0)
    tr, info = pol.rollout(init, 3)
    N = len(tr["obss"])
    assert list(tr.keys()) == ["obss", "next_obss", "actions", "rewards", "terminals", "traj_idxs", "acc_rets", "rtgs"]
    assert 32 <= N <= 96 and info["num_transitions"] == N and info["returns"].shape == (32,)
    assert tr["obss"].shape == tr["next_obss"].shape == (N, od) and tr["actions"].shape == (N, ad)
    assert tr["rewards"].shape == tr["terminals"].shape == tr["rtgs"].shape == (N, 1) and tr["traj_idxs"].shape == tr["acc_rets"].shape == (N,)
    assert np.array_equal(tr["traj_idxs"][:32], np.arange(32)) and tr["terminals"].dtype == bool
    assert np.allclose(tr["rtgs"][:, 0] + tr["acc_rets"], info["returns"][tr["traj_idxs"]], rtol=1e-6, atol=1e-6)
    assert np.isfinite(tr["rewards"]).all() and np.isfinite(tr["actions"]).all() and np.isfinite(info["reward_mean"])
