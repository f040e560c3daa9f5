"""GPU: MOBILE -- orl_dynsample_next (csrc/dynamics.hip), the ORL_ALGO_MOBILE schedule (csrc/algo_mobile.inc: penalty pass, k_lcb_penalty,
k_mobile_td_loss) and offlinerlkit.policy.MOBILEPolicy -- against the fixtures of the real reference (tests/golden/make_mobile_golden.py)
and tests/mobile_oracle.py, which test_mobile_cpu.py pins to them.

Gates.  Samples: 1e-5 of their scale + 1e-6, test_gpu_dynamics.py's bar for step()'s next_obs.  Penalty: every Q-value under it is held
to the project's 1e-4 relative gate and a standard deviation of such values cannot be asked to do better than that in absolute terms, so
|pen - ref| <= 1e-4 * max|lcb_q| of the fixture, at precision 0, 1 and 2 (measured maxima: DESIGN.md section 4.x3).  Losses, q1 / q2 /
target_q and post-step parameters: test_gpu_mb.py's bars for the MOPO fixtures (1e-4 relative; parameters 4e-6 (k + 1) at precision 0)."""
import warnings

import numpy as np
import pytest
import torch

import mobile_cases as mc
import mobile_oracle as mo
import synth
from helpers import check_state_against_golden, clone_state, load_golden, mopo_oracle_setup, rel_err, scale_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NETS = {"actor": 0, "critic1": 1, "critic2": 2, "critic1_old": 3, "critic2_old": 4}
_CACHE = {}


def case_data(case):
    """inputs, fixture and the oracle's samples of step 0 (computed once per case, never modified)"""
    if case not in _CACHE:
        c, st, dyn, scaler, batches, noises = mc.case_inputs(case)
        cfg = mc.oracle_cfg(c)
        mb = synth.mix_batch(batches[0])
        smp = mo.sample_next_obss(dyn, scaler, cfg["elites"], mb["observations"], mb["actions"], noises[0]["dyn"])
        _CACHE[case] = dict(c=c, cfg=cfg, st=st, dyn=dyn, scaler=scaler, batches=batches, noises=noises, g=load_golden(case), samples0=smp)
    return _CACHE[case]


def fresh_state(d):
    from oracle import sac as osac
    st = clone_state(d["st"])
    osac.init_opt(st)
    return st


def dyn_engine(c, dyns, scaler, seed=5):
    """an orl_dynamics of len(dyns) runs, run r with the parameters dyns[r]"""
    from offlinerlkit import _engine
    L = len(c["dyn_hidden"])
    cfg = _engine.default_dyn_config(obs_dim=c["obs_dim"], act_dim=c["act_dim"], hidden=c["dyn_hidden"], num_ensemble=c["K"],
                                     num_elites=len(c["elite_idx"]), weight_decay=[0.0] * (L + 1), n_runs=len(dyns), seed=seed)
    eng = _engine.Dynamics(cfg)
    for r, st in enumerate(dyns):
        full = dict(st)
        for k, v in st.items():
            if k.endswith(("weight", "bias")):
                full[k.replace("weight", "saved_weight").replace("bias", "saved_bias")] = v
        eng.set_params(r, full)
        eng.set_scaler(r, scaler[0], scaler[1])
        eng.set_elites(r, c["elite_idx"])
    return eng


def policy_engine(d, R=1, precision=0, **over):
    from offlinerlkit import _engine
    c, cfg = d["c"], d["cfg"]
    o = dict(obs_dim=c["obs_dim"], act_dim=c["act_dim"], hidden=c["hidden"], batch_size=c["B_real"] + c["B_fake"], n_runs=R,
             precision=precision, target_entropy=cfg["target_entropy"], auto_alpha=int(cfg["auto_alpha"]), alpha=cfg["alpha"],
             mobile_num_samples=c["S"], mobile_num_elites=len(c["elite_idx"]), mobile_real_rows=c["B_real"],
             penalty_coef=c["penalty_coef"], deterministic_backup=int(c["det"]))
    o.update(over)
    eng = _engine.Engine(_engine.default_config("mobile", **o))
    for r in range(R):
        for nm, nid in NETS.items():
            eng.set_net(r, nid, d["st"][nm])
        eng.set_scalar(r, _engine.SCALAR_LOG_ALPHA, float(d["st"]["log_alpha"][0]))
    return eng


def _lead(x, R):
    if isinstance(x, dict):
        return {k: np.stack([v] * R) for k, v in x.items()}
    return [np.stack([v] * R) for v in x]


def _slots(n):
    return [n["eps_lcb"], n["eps_next"], n["eps_actor"]]


def _close(a, b):
    return np.abs(a - b).max() <= 1e-5 * np.abs(b).max() + 1e-6


# ---- orl_dynsample_next -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["mobile_tiny", "mobile_ws"])
def test_sample_next_vs_fixture(case):
    d = case_data(case)
    c, g, n = d["c"], d["g"], d["noises"][0]
    mb = synth.mix_batch(d["batches"][0])
    eng = dyn_engine(c, [d["dyn"]], d["scaler"])
    out = eng.sample_next(mb["observations"][None], mb["actions"][None], c["S"], n["dyn"][None])[0]
    assert out.shape == d["samples0"].shape
    ref = g["step0/samples/digest"]
    assert np.abs(synth.digest(out) - ref).max() <= 1e-5 * np.abs(ref).max() + 1e-6
    if "step0/samples/full" in g.files:
        assert _close(out, g["step0/samples/full"])           # row order (S, E, B), elite order [2, 0, 3], obs added to the first od columns
    assert _close(out, d["samples0"])
    # the device form returns the same bytes and reads nothing back
    t = lambda a: torch.tensor(a, device=DEV).unsqueeze(0).contiguous()
    dev = eng.sample_next_device(t(mb["observations"]), t(mb["actions"]), c["S"], t(n["dyn"]))
    assert dev.is_cuda and np.array_equal(dev[0].cpu().numpy(), out)
    eng.close()


def test_sample_next_two_runs_with_different_weights():
    d = case_data("mobile_tiny")
    c, n = d["c"], d["noises"][0]
    other = mc.make_dynamics(np.random.RandomState(99), c)
    mb = synth.mix_batch(d["batches"][0])
    obs2 = np.stack([mb["observations"], mb["observations"][::-1]])
    act2 = np.stack([mb["actions"], mb["actions"][::-1]])
    nz2 = np.stack([n["dyn"], d["noises"][1]["dyn"]])
    eng = dyn_engine(c, [d["dyn"], other], d["scaler"])
    out = eng.sample_next(obs2, act2, c["S"], nz2)
    assert _close(out[0], d["g"]["step0/samples/full"])
    ref1 = mo.sample_next_obss(other, d["scaler"], c["elite_idx"], obs2[1], act2[1], nz2[1])
    assert _close(out[1], ref1)
    assert not _close(out[1], mo.sample_next_obss(d["dyn"], d["scaler"], c["elite_idx"], obs2[1], act2[1], nz2[1]))
    eng.close()


def test_sample_next_refusals():
    from offlinerlkit import _engine
    d = case_data("mobile_tiny")
    c = d["c"]
    mb = synth.mix_batch(d["batches"][0])
    o, a = mb["observations"][None], mb["actions"][None]
    eng = dyn_engine(c, [d["dyn"]], d["scaler"])
    with pytest.raises(RuntimeError, match="num_samples"):
        eng.sample_next(o, a, 0)
    eng.set_elites(0, [1])
    with pytest.raises(RuntimeError, match="2 elites"):
        eng.sample_next(o, a, 2)
    eng.close()
    eng = dyn_engine(c, [d["dyn"], d["dyn"]], d["scaler"])
    eng.set_elites(1, [0, 1])
    with pytest.raises(RuntimeError, match="same number of elites"):
        eng.sample_next(np.concatenate([o, o]), np.concatenate([a, a]), 2)
    eng.close()
    assert "orl_dynsample_next" in _engine.last_error()


def test_device_philox_draws_and_untouched_step_stream():
    d = case_data("mobile_tiny")
    c = d["c"]
    od, ad, E, S, n = c["obs_dim"], c["act_dim"], len(c["elite_idx"]), 4, 4096
    rng = np.random.default_rng(3)
    obs = rng.normal(size=(1, n, od)).astype(np.float32)
    act = rng.uniform(-1, 1, size=(1, n, ad)).astype(np.float32)
    eng = dyn_engine(c, [d["dyn"]], d["scaler"], seed=11)
    zero = np.zeros((1, S, E, n, od + 1), np.float32)
    mean = eng.sample_next(obs, act, S, zero)[0]
    std = eng.sample_next(obs, act, S, zero + 1)[0] - mean
    first = eng.sample_next(obs, act, S)[0]
    second = eng.sample_next(obs, act, S)[0]
    assert not np.array_equal(first, second)                   # keyed by the entry point's call counter
    for x in (first, second):
        z = ((x - mean) / std).astype(np.float64).reshape(-1, od)
        N = z.shape[0]
        assert np.all(np.abs(z.mean(axis=0)) <= 5.0 / np.sqrt(N)), z.mean(axis=0)         # 5 standard errors of the model mean
        assert np.all(np.abs(z.var(axis=0) - 1.0) <= 0.05), z.var(axis=0)
    # samples and elites are separate draws: no two (sample, elite) blocks share their noise
    zz = ((first - mean) / std).reshape(S * E, -1)
    assert np.abs(np.corrcoef(zz) - np.eye(S * E)).max() < 0.05
    eng.close()
    # orl_dyn_step before and after draws what it draws without the new call in between
    o1, a1 = obs[:, :300], act[:, :300]
    ea, eb = dyn_engine(c, [d["dyn"]], d["scaler"], seed=11), dyn_engine(c, [d["dyn"]], d["scaler"], seed=11)
    a_first, a_second = ea.step(o1, a1), ea.step(o1, a1)
    b_first = eb.step(o1, a1)
    eb.sample_next(o1, a1, 2)
    b_second = eb.step(o1, a1)
    for x, y in zip(a_first + a_second, b_first + b_second):
        assert np.array_equal(x, y)
    assert not np.array_equal(a_first[0], a_second[0])
    ea.close(); eb.close()


# ---- the engine: penalty, losses, parameters ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,R,precision", [(c, 1, 0) for c in mc.CASES] + [("mobile_default", 4, 1), ("mobile_default", 4, 2)])
def test_step_matches_oracle_and_reference(case, R, precision):
    d = case_data(case)
    c, cfg, g = d["c"], d["cfg"], d["g"]
    st = fresh_state(d)
    keys = [str(k) for k in g["loss_keys"]]
    dyn = dyn_engine(c, [d["dyn"]], d["scaler"])
    eng = policy_engine(d, R, precision)
    assert eng.metric_names == keys
    B_real = c["B_real"]
    try:
        for k, (b, n) in enumerate(zip(d["batches"], d["noises"])):
            mb = synth.mix_batch(b)
            res, aux = mo.learn(st, cfg, d["dyn"], d["scaler"], mb, n)
            smp = dyn.sample_next(mb["observations"][None], mb["actions"][None], c["S"], n["dyn"][None])[0]
            eng.set_next_samples(np.stack([smp.reshape(-1, c["obs_dim"])] * R))
            m = eng.step(_lead(mb, R), _lead(_slots(n), R))
            ora = np.array([res[x] for x in keys])
            qscale = np.abs(g[f"step{k}/lcb_q"]).max()
            for r in {0, R - 1}:
                assert rel_err(m[r], ora, floor=1e-2) < 1e-4, (case, k, r, m[r], ora)
                assert rel_err(m[r], g[f"step{k}/losses"], floor=1e-2) < 1e-4, (case, k, r, m[r], g[f"step{k}/losses"])
                pen = eng.debug_read(r, "penalty")
                perr = np.abs(pen - g[f"step{k}/penalty"].reshape(-1)).max()
                print(f"{case} precision {precision} step {k} run {r}: max |pen - ref| = {perr:.3e} = {perr / qscale:.3e} of max|lcb_q|")
                assert perr <= 1e-4 * qscale, (case, precision, k, r, perr, qscale)
                assert np.all(pen[:B_real] == 0)
                assert scale_err(eng.debug_read(r, "lcb_q"), g[f"step{k}/lcb_q"]) < 1e-4
                tq = eng.debug_read(r, "target_q")
                assert scale_err(tq, g[f"step{k}/target_q"]) < 1e-4
                assert np.any(tq == 0) and np.all(tq >= 0)                                  # the clamp is active and exact
                assert scale_err(eng.debug_read(r, "q1"), g[f"step{k}/q1"]) < 1e-4
                assert scale_err(eng.debug_read(r, "q2"), g[f"step{k}/q2"]) < 1e-4
            if precision == 0 and k in (0, len(d["batches"]) - 1):
                nets = {nm: eng.get_net(0, nid) for nm, nid in NETS.items()}
                check_state_against_golden(g, f"state{k}", nets, atol=4e-6 * (k + 1))
        assert not eng.health().any()
    finally:
        eng.close(); dyn.close()


@pytest.mark.parametrize("precision", [0, 1, 2])
def test_many_row_penalty_pass_takes_the_weight_stationary_launches(precision):
    """at run_mobile.py's shape (12 800 penalty rows) the target critics' forward is the launch CQL's B * N pass takes from 4096 rows:
    weight-stationary, with the three-plane flavour at precision 2"""
    d = case_data("mobile_default")
    c, n = d["c"], d["noises"][0]
    eng = policy_engine(d, 1, precision)
    eng.profile_enable(True)
    mb = synth.mix_batch(d["batches"][0])
    eng.set_next_samples(d["samples0"].reshape(1, -1, c["obs_dim"]))
    eng.step(_lead(mb, 1), _lead(_slots(n), 1))
    tags = {row["name"] for row in eng.profile_table()}
    lcb = sorted(t for t in tags if "lcb" in t)
    print("precision", precision, "penalty-pass launches:", lcb)
    assert any(t.startswith("target_lcb") for t in lcb) and any(t.startswith("actor_lcb") for t in lcb) and "lcb.penalty" in tags
    # the tiled launch of a two-hidden-layer net issues .fwd0 on its own; the weight-stationary one fuses layer 0 into .fwd1
    assert not any(t.startswith("target_lcb.fwd0") for t in lcb), lcb
    if precision == 2:
        assert any(t.startswith("target_lcb") and t.endswith("@p3") for t in lcb), lcb
    eng.close()


def test_mask_edge_cases():
    d = case_data("mobile_tiny")
    c, n = d["c"], d["noises"][0]
    B = c["B_real"] + c["B_fake"]
    mb = synth.mix_batch(d["batches"][0])
    smp = d["samples0"].reshape(1, -1, c["obs_dim"])

    def run(**over):
        eng = policy_engine(d, 1, 0, seed=3, **over)
        eng.set_next_samples(smp)
        m = eng.step(_lead(mb, 1), _lead(_slots(n), 1))
        out = (m.copy(), eng.debug_read(0, "penalty"), {nm: eng.get_net(0, nid) for nm, nid in NETS.items()})
        eng.close()
        return out
    m0, pen0, _ = run(mobile_real_rows=0)
    assert np.isfinite(m0).all() and np.all(pen0 > 0)
    m7, pen7, nets7 = run(mobile_real_rows=B, penalty_coef=7.0)
    mz, penz, netsz = run(mobile_real_rows=B, penalty_coef=0.0)
    assert np.all(pen7 == 0) and np.all(penz == 0)
    assert m7.tobytes() == mz.tobytes()
    for nm in NETS:
        for k in nets7[nm]:
            assert nets7[nm][k].tobytes() == netsz[nm][k].tobytes(), (nm, k)
    with pytest.raises(RuntimeError, match="mobile_real_rows"):
        policy_engine(d, 1, 0, mobile_real_rows=B + 1)
    with pytest.raises(RuntimeError, match="mobile_num_elites"):
        policy_engine(d, 1, 0, mobile_num_elites=1)


def test_missing_samples_and_learn_n_are_refused():
    d = case_data("mobile_tiny")
    c, n = d["c"], d["noises"][0]
    mb = synth.mix_batch(d["batches"][0])
    eng = policy_engine(d)
    before = {nm: eng.get_net(0, nid) for nm, nid in NETS.items()}
    with pytest.raises(RuntimeError, match="orl_engine_set_next_samples"):
        eng.step(_lead(mb, 1), _lead(_slots(n), 1))
    assert eng.step_count() == 0
    for nm, nid in NETS.items():
        after = eng.get_net(0, nid)
        assert all(after[k].tobytes() == before[nm][k].tobytes() for k in after)
    with pytest.raises(RuntimeError, match="MOBILE"):
        eng.learn_n(2)
    # one step per hand-over
    eng.set_next_samples(d["samples0"].reshape(1, -1, c["obs_dim"]))
    eng.step(_lead(mb, 1), _lead(_slots(n), 1))
    with pytest.raises(RuntimeError, match="orl_engine_set_next_samples"):
        eng.step(_lead(mb, 1), _lead(_slots(n), 1))
    assert eng.step_count() == 1
    eng.close()
    from offlinerlkit import _engine
    sac = _engine.Engine(_engine.default_config("sac", obs_dim=5, act_dim=2, hidden=[32, 32], batch_size=16))
    with pytest.raises(RuntimeError, match="not a MOBILE engine"):
        sac.set_next_samples(np.zeros((1, 16, 5), np.float32))
    sac.close()


def test_sac_engine_is_untouched_by_a_mobile_engine_in_the_same_process():
    import test_gpu_mb as tmb
    cfg, st, batches, noises = mopo_oracle_setup("mopo_tiny")
    c = synth.MOPO_CASES["mopo_tiny"]
    mb = synth.mix_batch(batches[0])
    nz = [noises[0]["eps_next"], noises[0]["eps_actor"]]

    def sac_step():
        eng = tmb._engine("sac", c, cfg, st, 1, 0, seed=21)
        m = eng.step(_lead(mb, 1), _lead(nz, 1))
        out = m.tobytes() + b"".join(eng.get_net(0, nid)[k].tobytes() for nid in NETS.values() for k in sorted(eng.get_net(0, nid))) + \
            eng.debug_read(0, "target_q").tobytes()
        eng.close()
        return out
    before = sac_step()
    d = case_data("mobile_tiny")
    eng = policy_engine(d)
    eng.set_next_samples(d["samples0"].reshape(1, -1, d["c"]["obs_dim"]))
    eng.step(_lead(synth.mix_batch(d["batches"][0]), 1), _lead(_slots(d["noises"][0]), 1))
    after_alive = sac_step()
    eng.close()
    assert before == after_alive == sac_step()


# ---- MOBILEPolicy ---------------------------------------------------------------------------------------------------------------------
def _package_dynamics(d):
    from offlinerlkit.dynamics import EnsembleDynamics
    from offlinerlkit.modules import EnsembleDynamicsModel
    from offlinerlkit.utils.scaler import StandardScaler
    c = d["c"]
    model = EnsembleDynamicsModel(c["obs_dim"], c["act_dim"], c["dyn_hidden"], c["K"], len(c["elite_idx"]),
                                  weight_decays=[0.0] * (len(c["dyn_hidden"]) + 1), device=DEV)
    with torch.no_grad():
        params = dict(model.named_parameters())
        for k, v in d["dyn"].items():
            params[k].copy_(torch.from_numpy(v))
    model.set_elites(list(c["elite_idx"]))
    return EnsembleDynamics(model, torch.optim.Adam(model.parameters(), lr=1e-3), StandardScaler(d["scaler"][0], d["scaler"][1]),
                            lambda o, a, n: np.zeros((len(o), 1), bool))


def _package_policy(d, dyn):
    from offlinerlkit.modules import ActorProb, Critic, TanhDiagGaussian
    from offlinerlkit.nets import MLP
    from offlinerlkit.policy import MOBILEPolicy
    from test_gpu_api import load
    c, cfg, st = d["c"], d["cfg"], d["st"]
    od, ad, hid = c["obs_dim"], c["act_dim"], c["hidden"]
    actor = ActorProb(MLP(od, hid), TanhDiagGaussian(hid[-1], ad, unbounded=True, conditioned_sigma=True), DEV)
    critics = torch.nn.ModuleList([Critic(MLP(od + ad, hid), DEV), Critic(MLP(od + ad, hid), DEV)])
    load(actor, st["actor"]); load(critics[0], st["critic1"]); load(critics[1], st["critic2"])
    if cfg["auto_alpha"]:
        log_alpha = torch.tensor(st["log_alpha"].copy(), requires_grad=True, device=DEV)
        alpha = (cfg["target_entropy"], log_alpha, torch.optim.Adam([log_alpha], lr=cfg["alpha_lr"]))
    else:
        alpha = cfg["alpha"]
    pol = MOBILEPolicy(dyn, actor, critics, torch.optim.Adam(actor.parameters(), lr=cfg["actor_lr"]),
                       torch.optim.Adam(critics.parameters(), lr=cfg["critic_lr"]), tau=cfg["tau"], gamma=cfg["gamma"], alpha=alpha,
                       penalty_coef=c["penalty_coef"], num_samples=c["S"], deterministic_backup=c["det"])
    load(pol.critics_old[0], st["critic1_old"]); load(pol.critics_old[1], st["critic2_old"])
    return pol


def _tb2(b):
    return {part: {k: torch.tensor(v, device=DEV) for k, v in b[part].items()} for part in ("real", "fake")}


@pytest.mark.parametrize("case", ["mobile_tiny", "mobile_tiny_fixed_alpha_det"])
def test_policy_learn_and_compute_lcb_vs_reference(case):
    d = case_data(case)
    c, g = d["c"], d["g"]
    dyn = _package_dynamics(d)
    pol = _package_policy(d, dyn)
    pol.set_engine_options(seed=7, precision=0)
    keys = [str(k) for k in g["loss_keys"]]
    B_real = c["B_real"]
    # sample_next_obss: the reference's public call, (S, E, B, od) on the dynamics' device
    mb0 = synth.mix_batch(d["batches"][0])
    s = dyn.sample_next_obss(torch.tensor(mb0["observations"], device=DEV), torch.tensor(mb0["actions"], device=DEV), c["S"])
    assert s.is_cuda and tuple(s.shape) == d["samples0"].shape and torch.isfinite(s).all()
    s_np = dyn.sample_next_obss(mb0["observations"], mb0["actions"], c["S"])
    assert tuple(s_np.shape) == tuple(s.shape)
    # compute_lcb: the un-zeroed penalty (the fixture's rows are zeroed on the real rows: the model rows are compared)
    n0 = d["noises"][0]
    pen = pol.compute_lcb(torch.tensor(mb0["observations"], device=DEV), torch.tensor(mb0["actions"], device=DEV), noise=(n0["eps_lcb"], n0["dyn"]))
    assert pen.is_cuda and tuple(pen.shape) == (B_real + c["B_fake"], 1)
    pen = pen.cpu().numpy().reshape(-1)
    qscale = np.abs(g["step0/lcb_q"]).max()
    assert np.abs(pen[B_real:] - g["step0/penalty"].reshape(-1)[B_real:]).max() <= 1e-4 * qscale
    ora_pen, _ = mo.compute_lcb(fresh_state(d), d["cfg"], d["dyn"], d["scaler"], mb0["observations"], mb0["actions"], n0)
    assert np.abs(pen - ora_pen.reshape(-1)).max() <= 1e-4 * qscale and np.all(pen[:B_real] > 0)
    assert pol.engine.step_count() == 0
    for k, (b, n) in enumerate(zip(d["batches"], d["noises"])):
        res = pol.learn(_tb2(b), noise=[n["eps_lcb"], n["eps_next"], n["eps_actor"], n["dyn"]])
        assert list(res.keys()) == keys
        got = np.array([res[x] for x in keys])
        assert rel_err(got, g[f"step{k}/losses"], floor=1e-2) < 1e-4, (case, k, got, g[f"step{k}/losses"])
        assert np.all(pol.engine.debug_read(0, "penalty")[:B_real] == 0)
    sd = pol.state_dict()
    assert list(sd.keys()) == [str(x) for x in g["state_keys"]]
    last = len(d["batches"]) - 1
    nets = {"actor": "actor", "critic1": "critics.0", "critic2": "critics.1", "critic1_old": "critics_old.0", "critic2_old": "critics_old.1"}
    got = {nm: {k[len(pre) + 1:]: v.detach().cpu().numpy() for k, v in sd.items() if k.startswith(pre + ".")} for nm, pre in nets.items()}
    check_state_against_golden(g, f"state{last}", got, atol=4e-6 * (last + 1))
    # another real / model split re-binds the engine around the weights and the optimizer state
    b = d["batches"][0]
    cut = {part: {k: v[:2] if part == "real" else v for k, v in b[part].items()} for part in b}
    res = pol.learn(_tb2(cut))
    assert np.isfinite(list(res.values())).all() and pol.engine.step_count() == last + 2
    assert pol.engine.cfg.mobile_real_rows == 2 and pol.engine.cfg.batch_size == 2 + c["B_fake"]
    assert not pol.engine.health().any()
    pol._unbind()


def test_mb_trainer_end_to_end(tmp_path):
    """MBPolicyTrainer(fused=False) with MOBILEPolicy on the point-mass task, at the size of test_gpu_mb_trainer.py's MOPO case"""
    from offlinerlkit.buffer import ReplayBuffer
    from offlinerlkit.modules import ActorProb, Critic, TanhDiagGaussian
    from offlinerlkit.nets import MLP
    from offlinerlkit.policy import MOBILEPolicy
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
    pol = MOBILEPolicy(dyn, actor, critics, actor_optim, adam(critics, 1e-3), tau=0.005, gamma=0.95, alpha=alpha, penalty_coef=1.5,
                       num_samples=10, deterministic_backup=True)
    pol.eval()
    untrained = rollout_return(lambda o: pol.select_action(o.reshape(1, -1), deterministic=True)[0], 10, 1000)
    fake = ReplayBuffer(ROLLOUT[1] * ROLLOUT[2] * 2, (OD,), np.float32, AD, np.float32, device=DEV)

    class Env(PointMass):
        def get_normalized_score(self, x):
            return x / 20.0
    epochs, steps = 2, 250
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(actor_optim, epochs)         # run_mobile.py:106
    with pytest.raises(ValueError, match="rollout_device"):
        MBPolicyTrainer(pol, Env(1000), real, fake, logger, ROLLOUT, epoch=epochs, step_per_epoch=steps, fused=True)
    from offlinerlkit import _engine
    with warnings.catch_warnings():
        warnings.simplefilter("error", _engine.EngineHealthWarning)                  # a raised health flag fails the test
        res = MBPolicyTrainer(pol, Env(1000), real, fake, logger, ROLLOUT, epoch=epochs, step_per_epoch=steps, batch_size=256,
                              real_ratio=0.05, eval_episodes=5, lr_scheduler=sched, fused=False).train()
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
    assert abs(actor_optim.param_groups[0]["lr"]) < 1e-9                               # two scheduler steps of a two-epoch cosine: lr 0
    pol.eval()
    trained = rollout_return(lambda o: pol.select_action(o.reshape(1, -1), deterministic=True)[0], 10, 1000)
    print(f"mobile: return of the untrained policy {untrained:.2f}, after {epochs * steps} steps {trained:.2f}; "
          f"normalised eval per epoch {col('eval/normalized_episode_reward').round(2).tolist()}")
    assert trained > untrained, (trained, untrained)
    assert np.isfinite(res["last_10_performance"])
