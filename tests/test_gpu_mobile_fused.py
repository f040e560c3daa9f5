"""GPU: MOBILE's learn as one device loop -- orl_mobile_learn_n (csrc/algo_mobile.inc: Engine::mobile_loop), the fused sample producer
k_dyn_sample_rows behind orl::dynsample_enqueue (csrc/dynamics.hip) and offlinerlkit.policy.MOBILEDevicePolicy -- against the two-call
path it replaces (orl_dynsample_next, orl_engine_set_next_samples, orl_step: the same kernels on the same inputs, so bytes are compared),
against tests/mobile_oracle.py on the tapped batch, samples and noise, and through MBPolicyTrainer(fused=True).

Gates.  Producer against orl_dynsample_next and loop against its replay on an eager twin: byte equality (metrics of the replay:
test_gpu_learn_n.py's bar for same-kernel paths, rel_err(floor=1e-3) < 2e-6).  Oracle: the project's 1e-4 relative gate on the losses and
|pen - ref| <= 1e-4 * max|lcb_q| on the penalty, as test_gpu_mobile.py.  Shapes: mobile_tiny (a non-sorted elite order, obs_dim 5: no
whole quad per row end, D = 6: the reward column in the second quad, 144 penalty rows) and mobile_ws (5 120 penalty rows: over the
weight-stationary threshold and no multiple of it)."""
import warnings

import numpy as np
import pytest
import torch

import mobile_cases as mc
import mobile_oracle as mo
import synth
import test_gpu_mobile as tgm
from helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = tgm.DEV
NETS = tgm.NETS
N_REAL, N_MODEL = 2000, 1500
_DATA = {}


def _datasets(od, ad):
    """(dataset rows, ring rows) with disjoint value ranges, computed once per shape and never modified: observation column 0 and the
    reward lie in [-1, 1] on the dataset rows and in [2, 4] on the model rows"""
    if (od, ad) not in _DATA:
        out = []
        for seed, n, model in ((11, N_REAL, False), (12, N_MODEL, True)):
            ds = synth.make_dataset(seed, n, od, ad, term_p=0.05)
            o, no = ds["observations"].copy(), ds["next_observations"].copy()
            r = np.tanh(ds["rewards"]).astype(np.float32)
            o[:, 0] = np.tanh(o[:, 0])
            if model:
                o[:, 0] += 3.0
                r = r + np.float32(3.0)
            out.append((o, ds["actions"], no, r, ds["terminals"].astype(np.float32)))
        _DATA[(od, ad)] = tuple(out)
    return _DATA[(od, ad)]


class Rig:
    """a MOBILE engine with its dataset buffer and model ring attached, and its dynamics"""

    def __init__(self, case, precision=0, seed=9, dyn_seed=5, attach=True):
        from offlinerlkit import _engine
        self.d = d = tgm.case_data(case)
        c = d["c"]
        self.od, self.ad, self.B, self.B_real = c["obs_dim"], c["act_dim"], c["B_real"] + c["B_fake"], c["B_real"]
        self.M = c["S"] * len(c["elite_idx"]) * self.B
        self.eng = tgm.policy_engine(d, 1, precision, seed=seed)
        self.dyn = tgm.dyn_engine(c, [d["dyn"]], d["scaler"], seed=dyn_seed)
        self.real, self.model = _engine.DeviceBuffer(self.od, self.ad), _engine.DeviceBuffer(self.od, self.ad)
        real_rows, model_rows = _datasets(self.od, self.ad)
        self.real.load(*real_rows)
        self.model.reserve(2 * N_MODEL)
        self.model.append(*model_rows)
        if attach:
            self.eng.attach_buffer(self.real)
            self.eng.attach_model_buffer(self.model, self.B_real)

    def learn_n(self, n):
        return self.eng.mobile_learn_n(self.dyn, n)

    def tap(self, name, cols):
        return self.eng.debug_read(0, name).reshape(-1, cols)

    def batch(self):
        od, ad = self.od, self.ad
        return dict(observations=self.tap("b_obs", od), actions=self.tap("b_act", ad), next_observations=self.tap("b_nobs", od),
                    rewards=self.tap("b_rew", 1), terminals=self.tap("b_term", 1))

    def noise(self):
        return [self.tap(n, self.ad) for n in ("n_eps_lcb", "n_eps_next", "n_eps_actor")]

    def operands(self):
        """(xs [M][OP], xl [M][XP]) of the last penalty pass"""
        return self.tap("xs", -(-self.od // 4) * 4), self.tap("xl", -(-(self.od + self.ad) // 4) * 4)

    def params(self):
        out = b"".join(self.eng.get_net(0, nid)[k].tobytes() for nid in NETS.values() for k in sorted(self.eng.get_net(0, nid)))
        for nid in self.eng.trainable_nets():
            m, v = self.eng.adam_state(0, nid)
            out += m.tobytes() + v.tobytes()
        return out

    def close(self):
        for x in (self.eng, self.dyn, self.real, self.model):
            x.close()


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV).unsqueeze(0).contiguous()


# ---- 1. the fused producer is the two-kernel path, bit for bit -----------------------------------------------------------------------
@pytest.mark.parametrize("case", ["mobile_tiny", "mobile_ws"])
def test_fused_producer_equals_sample_next_and_assemble(case):
    rig = Rig(case)
    c = rig.d["c"]
    twin = tgm.dyn_engine(c, [rig.d["dyn"]], rig.d["scaler"], seed=5)      # same weights, scaler, elites, seed and call counter
    od, ad = rig.od, rig.ad
    try:
        for step in range(3):                                               # the call counter: 0, 1, 2
            assert rig.dyn.sample_calls() == twin.sample_calls() == step
            rig.learn_n(1)
            b = rig.batch()
            xs, xl = rig.operands()
            ref = twin.sample_next_device(_dev(b["observations"]), _dev(b["actions"]), c["S"])[0].cpu().numpy().reshape(-1, od)
            assert xs.shape[0] == xl.shape[0] == ref.shape[0] == rig.M
            assert xs[:, :od].tobytes() == ref.tobytes(), (case, step, np.abs(xs[:, :od] - ref).max())
            assert xl[:, :od].tobytes() == ref.tobytes(), (case, step)
            assert np.all(xs[:, od:] == 0) and np.all(xl[:, od + ad:] == 0)
            # the action columns of xl are the sampling job's: tanh-squashed actions, not left-over zeros
            assert np.all(np.abs(xl[:, od:od + ad]) <= 1) and np.any(xl[:, od:od + ad] != 0)
            if step:
                assert prev != ref.tobytes()
            prev = ref.tobytes()
            # the forward saw the bits it sees from packed rows
            assert rig.dyn.debug_read(0, "step.x").tobytes() == twin.debug_read(0, "step.x").tobytes()
            assert rig.dyn.debug_read(0, "step.out").tobytes() == twin.debug_read(0, "step.out").tobytes()
    finally:
        rig.close(); twin.close()


# ---- 2. the loop is the replay of its steps ------------------------------------------------------------------------------------------
def _replay(rig, twin, steps=4):
    """`steps` x learn_n(1) on rig, each replayed on the eager engine `twin` from the taps; returns the largest metric error"""
    worst = 0.0
    for k in range(steps):
        m, _ = rig.learn_n(1)
        b, nz = rig.batch(), rig.noise()
        xs, _ = rig.operands()
        twin.set_next_samples(np.ascontiguousarray(xs[:, :rig.od])[None])
        me = twin.step({kk: v[None] for kk, v in b.items()}, [v[None] for v in nz])
        err = rel_err(m, me, floor=1e-3)
        print(f"step {k}: loop {m[0]} eager {me[0]} rel_err {err:.3e}")
        assert err < 2e-6, (k, m, me)
        worst = max(worst, err)
    return worst


def _twin_state(eng):
    out = b"".join(eng.get_net(0, nid)[k].tobytes() for nid in NETS.values() for k in sorted(eng.get_net(0, nid)))
    for nid in eng.trainable_nets():
        m, v = eng.adam_state(0, nid)
        out += m.tobytes() + v.tobytes()
    return out


@pytest.mark.parametrize("case,precision", [("mobile_tiny", 0), ("mobile_tiny", 2), ("mobile_ws", 1)])
def test_loop_is_the_replay_of_its_steps(case, precision):
    rig = Rig(case, precision)
    twin = tgm.policy_engine(rig.d, 1, precision, seed=9)
    try:
        _replay(rig, twin)
        assert rig.eng.step_count() == twin.step_count() == 4
        assert rig.params() == _twin_state(twin)                           # all five nets and the Adam moments, byte for byte
        assert not rig.eng.health().any()
    finally:
        rig.close(); twin.close()


# ---- 3. one call of 4 steps == four calls of 1 step ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["mobile_tiny", "mobile_ws"])
def test_one_call_of_four_steps_equals_four_calls_of_one(case):
    a, b = Rig(case), Rig(case)
    try:
        m4, ms = a.learn_n(4)
        m1 = np.stack([b.learn_n(1)[0] for _ in range(4)])
        assert ms > 0
        assert rel_err(m4, m1.astype(np.float64).mean(axis=0), floor=1e-3) < 2e-6, (m4, m1)
        assert a.params() == b.params()
        assert a.eng.step_count() == b.eng.step_count() == 4
        assert a.dyn.sample_calls() == b.dyn.sample_calls() == 4
        for name, cols in (("b_obs", a.od), ("n_eps_lcb", a.ad), ("penalty", 1), ("lcb_q", 1), ("ql1", 1), ("ql2", 1), ("logp_l", 1)):
            assert a.tap(name, cols).tobytes() == b.tap(name, cols).tobytes(), name      # the taps hold the last step's values
    finally:
        a.close(); b.close()


# ---- 4. oracle -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["mobile_tiny", "mobile_ws"])
def test_loop_matches_the_oracle_on_the_tapped_inputs(case, monkeypatch):
    # the oracle's penalty pass on the samples the loop drew (the device Philox draws have no host counterpart)
    monkeypatch.setattr(mo, "compute_lcb", lambda state, cfg, dyn, scaler, obs, act, noise: mo.lcb_from_samples(state, noise["samples"], noise["eps_lcb"]))
    rig = Rig(case)
    d, c = rig.d, rig.d["c"]
    st = tgm.fresh_state(d)
    keys = rig.eng.metric_names
    S, E = c["S"], len(c["elite_idx"])
    try:
        for k in range(3 if case == "mobile_tiny" else 1):
            m, _ = rig.learn_n(1)
            b, nz = rig.batch(), rig.noise()
            xs, _ = rig.operands()
            noise = dict(samples=xs[:, :rig.od].reshape(S, E, rig.B, rig.od).copy(), eps_lcb=nz[0], eps_next=nz[1], eps_actor=nz[2])
            res, aux = mo.learn(st, d["cfg"], d["dyn"], d["scaler"], b, noise)
            ora = np.array([res[x] for x in keys])
            assert rel_err(m[0], ora, floor=1e-2) < 1e-4, (case, k, m[0], ora)
            pen = rig.tap("penalty", 1)
            qscale = np.abs(aux["lcb_q"]).max()
            perr = np.abs(pen - aux["penalty"].reshape(-1, 1)).max()
            print(f"{case} step {k}: max |pen - ref| = {perr:.3e} = {perr / qscale:.3e} of max|lcb_q|")
            assert perr <= 1e-4 * qscale, (case, k, perr, qscale)
    finally:
        rig.close()


# ---- 5. batch layout and draws ---------------------------------------------------------------------------------------------------------
def test_batch_layout_draws_and_untouched_step_stream():
    rig = Rig("mobile_tiny")
    c = rig.d["c"]
    fresh = tgm.dyn_engine(c, [rig.d["dyn"]], rig.d["scaler"], seed=5)
    Br = rig.B_real
    try:
        seen = []
        for _ in range(2):
            rig.learn_n(1)
            b = rig.batch()
            o0, r = b["observations"][:, 0], b["rewards"][:, 0]
            assert np.all(np.abs(o0[:Br]) <= 1) and np.all(np.abs(r[:Br]) <= 1)                     # dataset rows
            assert np.all((o0[Br:] >= 2) & (o0[Br:] <= 4)) and np.all((r[Br:] >= 2) & (r[Br:] <= 4))   # ring rows
            pen = rig.tap("penalty", 1)
            assert np.all(pen[:Br] == 0) and np.all(pen[Br:] > 0)
            seen.append(b["observations"].tobytes())
        assert seen[0] != seen[1]
        # orl_dyn_step's stream: a step_device after the loop gives the bits it gives without the loop
        rng = np.random.default_rng(4)
        obs, act = _dev(rng.normal(size=(300, rig.od)).astype(np.float32)), _dev(rng.uniform(-1, 1, size=(300, rig.ad)).astype(np.float32))
        for x, y in zip(rig.dyn.step_device(obs, act), fresh.step_device(obs, act)):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
        assert rig.dyn.sample_calls() == 2 and fresh.sample_calls() == 0
    finally:
        rig.close(); fresh.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_move_no_counter():
    from offlinerlkit import _engine
    rig = Rig("mobile_tiny", attach=False)
    d, c = rig.d, rig.d["c"]
    eng, dyn = rig.eng, rig.dyn
    before = rig.params()
    others = []

    def refused(match, e=None, dy=None, n=2):
        e, dy = e or eng, dy or dyn
        steps, calls = e.step_count(), dy.sample_calls()
        with pytest.raises(RuntimeError, match=match):
            e.mobile_learn_n(dy, n)
        assert "orl_mobile_learn_n" in _engine.last_error()
        assert e.step_count() == steps and dy.sample_calls() == calls
    try:
        # buffers: none, the dataset alone, an empty ring, a ring attached with another real-row count
        refused("no replay buffer")
        eng.attach_buffer(rig.real)
        refused("no model ring")
        empty = _engine.DeviceBuffer(rig.od, rig.ad)
        others.append(empty)
        empty.reserve(64)
        eng.attach_model_buffer(empty, rig.B_real)
        refused("empty")
        eng.attach_model_buffer(rig.model, rig.B_real + 1)
        refused("real_rows")
        eng.attach_model_buffer(rig.model, rig.B_real)
        refused("n_steps", n=0)
        refused("n_steps", n=-3)
        # the other engine kinds and several runs on either side
        sac = _engine.Engine(_engine.default_config("sac", obs_dim=rig.od, act_dim=rig.ad, hidden=c["hidden"], batch_size=rig.B))
        others.append(sac)
        refused("not a MOBILE engine", e=sac)
        eng2 = tgm.policy_engine(d, 2)
        others.append(eng2)
        refused("n_runs == 1", e=eng2)
        dyn2 = tgm.dyn_engine(c, [d["dyn"], d["dyn"]], d["scaler"])
        others.append(dyn2)
        refused("n_runs == 1", dy=dyn2)
        if torch.cuda.device_count() > 1:
            L = len(c["dyn_hidden"])
            far = _engine.Dynamics(_engine.default_dyn_config(obs_dim=rig.od, act_dim=rig.ad, hidden=c["dyn_hidden"], num_ensemble=c["K"],
                                                              num_elites=len(c["elite_idx"]), weight_decay=[0.0] * (L + 1), device=1))
            others.append(far)
            refused("one device", dy=far)
        # dims, a dynamics without reward, the elite count
        for over in (dict(obs_dim=rig.od + 1), dict(act_dim=rig.ad + 1)):
            c2 = dict(c, **over)
            w = c2["obs_dim"] + c2["act_dim"]
            wide = tgm.dyn_engine(c2, [mc.make_dynamics(np.random.RandomState(1), c2)], (np.zeros((1, w), np.float32), np.ones((1, w), np.float32)))
            others.append(wide)
            refused("dims", dy=wide)
        L = len(c["dyn_hidden"])
        norew = _engine.Dynamics(_engine.default_dyn_config(obs_dim=rig.od, act_dim=rig.ad, hidden=c["dyn_hidden"], num_ensemble=c["K"],
                                                            num_elites=len(c["elite_idx"]), weight_decay=[0.0] * (L + 1), with_reward=0))
        others.append(norew)
        refused("with_reward", dy=norew)
        dyn.set_elites(0, [2, 0])
        refused("mobile_num_elites")
        dyn.set_elites(0, [1])
        refused("2 elites")
        dyn.set_elites(0, c["elite_idx"])
        # pending samples are refused and survive the refusal: the next orl_step consumes them
        mb = synth.mix_batch(d["batches"][0])
        eng.set_next_samples(d["samples0"].reshape(1, -1, rig.od))
        refused("pending")
        # orl_learn_n keeps refusing the engine
        with pytest.raises(RuntimeError, match="MOBILE"):
            eng.learn_n(2)
        assert rig.params() == before
        assert eng.step_count() == 0 and dyn.sample_calls() == 0
        twin = tgm.policy_engine(d, 1, 0, seed=9)
        others.append(twin)
        twin.set_next_samples(d["samples0"].reshape(1, -1, rig.od))
        slots = tgm._lead(tgm._slots(d["noises"][0]), 1)
        m, mt = eng.step(tgm._lead(mb, 1), slots), twin.step(tgm._lead(mb, 1), slots)
        assert m.tobytes() == mt.tobytes() and eng.step_count() == 1
        # ... and after all of them the loop runs
        m, _ = rig.learn_n(2)
        assert np.isfinite(m).all() and eng.step_count() == 3 and dyn.sample_calls() == 2
    finally:
        rig.close()
        for x in others:
            x.close()


# ---- 7. the trainer, end to end --------------------------------------------------------------------------------------------------------
def test_fused_mb_trainer_end_to_end(tmp_path):
    """MBPolicyTrainer(fused=True) with MOBILEDevicePolicy on the point-mass task, at the size of
    test_gpu_mobile.py::test_mb_trainer_end_to_end and with its assertions"""
    from offlinerlkit import _engine
    from offlinerlkit.buffer import ReplayBuffer
    from offlinerlkit.modules import ActorProb, Critic, TanhDiagGaussian
    from offlinerlkit.nets import MLP
    from offlinerlkit.policy import MOBILEDevicePolicy, MOBILEPolicy
    from offlinerlkit.policy_trainer import MBPolicyTrainer
    from offlinerlkit.utils.logger import Logger
    from test_gpu_mb_trainer import ROLLOUT, _dynamics
    from test_gpu_training import AD, HID, OD, PointMass, make_dataset, rollout_return
    torch.manual_seed(3)
    np.random.seed(3)
    ds = make_dataset(n_episodes=300)
    logger = Logger(str(tmp_path), {"consoleout_backup": "stdout", "policy_training_progress": "csv", "dynamics_training_progress": "csv"})
    real = ReplayBuffer(len(ds["rewards"]), (OD,), np.float32, AD, np.float32, device=DEV)
    real.load_dataset(ds)
    dyn = _dynamics(real.sample_all(), logger)
    dyn._penalty_coef = 0.0                               # run_mobile.py builds the dynamics without a reward penalty: MOBILE's is in the target
    adam = lambda m, lr: torch.optim.Adam(m.parameters(), lr=lr)
    actor = ActorProb(MLP(OD, HID), TanhDiagGaussian(HID[-1], AD, unbounded=True, conditioned_sigma=True), DEV)
    critics = torch.nn.ModuleList([Critic(MLP(OD + AD, HID), DEV), Critic(MLP(OD + AD, HID), DEV)])
    log_alpha = torch.zeros(1, requires_grad=True, device=DEV)
    alpha = (-float(AD), log_alpha, torch.optim.Adam([log_alpha], lr=1e-3))
    actor_optim = adam(actor, 1e-3)
    pol = MOBILEDevicePolicy(dyn, actor, critics, actor_optim, adam(critics, 1e-3), tau=0.005, gamma=0.95, alpha=alpha, penalty_coef=1.5,
                             num_samples=10, deterministic_backup=True)
    assert isinstance(pol, MOBILEPolicy)
    pol.eval()
    untrained = rollout_return(lambda o: pol.select_action(o.reshape(1, -1), deterministic=True)[0], 10, 1000)
    fake = ReplayBuffer(ROLLOUT[1] * ROLLOUT[2] * 2, (OD,), np.float32, AD, np.float32, device=DEV)

    class Env(PointMass):
        def get_normalized_score(self, x):
            return x / 20.0
    epochs, steps = 2, 250
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(actor_optim, epochs)         # run_mobile.py:106
    with warnings.catch_warnings():
        warnings.simplefilter("error", _engine.EngineHealthWarning)                  # a raised health flag fails the test
        res = MBPolicyTrainer(pol, Env(1000), real, fake, logger, ROLLOUT, epoch=epochs, step_per_epoch=steps, batch_size=256,
                              real_ratio=0.05, eval_episodes=5, lr_scheduler=sched, fused=True).train()
    rows = [ln.split(",") for ln in open(tmp_path / "record" / "policy_training_progress.csv").read().strip().split("\n")]
    head = rows[0]
    losses = ["loss/actor", "loss/critic", "loss/alpha", "alpha"]                    # mobile.py:187-194
    evals = ["eval/normalized_episode_reward", "eval/normalized_episode_reward_std", "eval/episode_length", "eval/episode_length_std"]
    assert set(losses + evals + ["rollout_info/num_transitions", "rollout_info/reward_mean", "timestep"]) <= set(head)
    assert "loss/critic1" not in head
    col = lambda k: np.array([float(x[head.index(k)]) for x in rows[1:]])
    for k in losses + evals:
        assert np.isfinite(col(k)).all(), k
    assert pol.engine.step_count() == epochs * steps and not pol.engine.health().any()
    assert pol.engine.cfg.mobile_real_rows == 12 and pol.engine.cfg.mobile_num_elites == 3
    assert dyn._eng.sample_calls() == epochs * steps                                   # every step took its samples inside the loop
    assert abs(actor_optim.param_groups[0]["lr"]) < 1e-9                               # two scheduler steps of a two-epoch cosine: lr 0
    pol.eval()
    trained = rollout_return(lambda o: pol.select_action(o.reshape(1, -1), deterministic=True)[0], 10, 1000)
    print(f"mobile, fused: return of the untrained policy {untrained:.2f}, after {epochs * steps} steps {trained:.2f}; "
          f"normalised eval per epoch {col('eval/normalized_episode_reward').round(2).tolist()}")
    assert trained > untrained, (trained, untrained)
    assert np.isfinite(res["last_10_performance"])
