"""CPU: tests/mobile_oracle.py (numpy restatement of sample_next_obss / compute_lcb / MOBILEPolicy.learn) pinned to the fixtures of the real
reference (tests/golden/make_mobile_golden.py) at the bars of test_oracle_golden.py / test_rambo_cpu.py -- losses and Q-values 1e-4
relative, Q arrays 1e-5 of their scale, parameters a few 1e-6 absolute --, and what MOBILEPolicy refuses without a GPU."""
import numpy as np
import pytest
import torch

import mobile_cases as mc
import mobile_oracle as mo
import synth
from helpers import check_state_against_golden, clone_state, load_golden, rel_err, rel_err_keys, key_scales, scale_err

NETS = ("actor", "critic1", "critic2", "critic1_old", "critic2_old")


def oracle_setup(case):
    from oracle import sac as osac
    c, st, dyn, scaler, batches, noises = mc.case_inputs(case)
    st = clone_state(st)
    osac.init_opt(st)
    return c, mc.oracle_cfg(c), st, dyn, scaler, batches, noises


@pytest.mark.parametrize("case", list(mc.CASES))
def test_oracle_matches_reference(case):
    g = load_golden(case)
    c, cfg, st, dyn, scaler, batches, noises = oracle_setup(case)
    keys = [str(k) for k in g["loss_keys"]]
    B_real = c["B_real"]
    for k, (b, n) in enumerate(zip(batches, noises)):
        mb = synth.mix_batch(b)
        if k == 0:
            smp = mo.sample_next_obss(dyn, scaler, cfg["elites"], mb["observations"], mb["actions"], n["dyn"])
            assert smp.shape == (c["S"], len(c["elite_idx"]), B_real + c["B_fake"], c["obs_dim"])
            ref = g["step0/samples/digest"]
            assert np.abs(synth.digest(smp) - ref).max() <= 1e-5 * np.abs(ref).max() + 1e-6
            if "step0/samples/full" in g.files:
                assert np.abs(smp - g["step0/samples/full"]).max() <= 1e-5 * np.abs(g["step0/samples/full"]).max() + 1e-6
        res, aux = mo.learn(st, cfg, dyn, scaler, mb, n)
        assert list(res.keys()) == keys
        got, ref = np.array([res[x] for x in keys]), g[f"step{k}/losses"]
        assert rel_err(got, ref, floor=1e-2) < 1e-4, (case, k, got, ref)
        assert rel_err_keys(got, ref, key_scales(g)) < 1e-4, (case, k, got, ref)
        for name in ("q1", "q2", "target_q", "lcb_q"):
            assert scale_err(aux[name], g[f"step{k}/{name}"]) < 1e-5, (case, k, name)
        # a standard deviation of Q-values held to 1e-5 of the Q scale cannot be asked to do better than that in absolute terms
        qscale = np.abs(g[f"step{k}/lcb_q"]).max()
        assert np.abs(aux["penalty"] - g[f"step{k}/penalty"]).max() <= 1e-5 * qscale, (case, k)
        assert np.all(aux["penalty"][:B_real] == 0) and np.all(g[f"step{k}/penalty"][:B_real] == 0)
        assert np.array_equal(aux["target_q"] == 0, g[f"step{k}/target_q"] == 0) or \
            np.abs(aux["raw_target"][(aux["target_q"] == 0) != (g[f"step{k}/target_q"] == 0)]).max() < 1e-5
        if k in (0, len(batches) - 1):
            check_state_against_golden(g, f"state{k}", {nm: st[nm] for nm in NETS}, atol=2e-6 * (k + 1))
            if cfg["auto_alpha"]:
                assert abs(float(st["log_alpha"][0]) - float(g[f"state{k}/log_alpha"][0])) < 1e-6


@pytest.mark.parametrize("case", list(mc.CASES))
def test_fixtures_are_not_vacuous(case):
    """what the generator asserted, read back from the committed files"""
    g = load_golden(case)
    c = mc.CASES[case]
    assert 0.10 <= float(g["step0/clamped_fraction"][0]) <= 0.90
    assert np.any(g["step0/target_q"] == 0) and np.any(g["step0/target_q"] > 0)
    pen, qscale = g["step0/penalty"].reshape(-1), np.abs(g["step0/lcb_q"]).max()
    assert np.all(pen[:c["B_real"]] == 0) and np.all(pen[c["B_real"]:] > 1e-3 * qscale)
    assert g["step0/lcb_q"].shape == (c["S"] * len(c["elite_idx"]) * (c["B_real"] + c["B_fake"]), 1)
    assert list(c["elite_idx"]) != sorted(c["elite_idx"])


def _policy(n_critics=2, dynamics=None):
    from offlinerlkit.modules import ActorProb, Critic, TanhDiagGaussian
    from offlinerlkit.nets import MLP
    from offlinerlkit.policy import MOBILEPolicy
    od, ad, hid = 5, 2, [32, 32]
    actor = ActorProb(MLP(od, hid), TanhDiagGaussian(hid[-1], ad, unbounded=True, conditioned_sigma=True), "cpu")
    critics = torch.nn.ModuleList([Critic(MLP(od + ad, hid), "cpu") for _ in range(n_critics)])
    return MOBILEPolicy(dynamics if dynamics is not None else object(), actor, critics, torch.optim.Adam(actor.parameters(), lr=1e-4),
                        torch.optim.Adam(critics.parameters(), lr=3e-4), penalty_coef=1.5, num_samples=10, deterministic_backup=True)


def test_state_dict_keys_are_the_references():
    pol = _policy()
    g = load_golden("mobile_tiny")
    assert list(pol.state_dict().keys()) == [str(k) for k in g["state_keys"]]
    assert {k.split(".")[0] + "." + k.split(".")[1] for k in pol.state_dict() if not k.startswith("actor.")} == \
        {"critics.0", "critics.1", "critics_old.0", "critics_old.1"}


def test_refusals_without_a_gpu():
    with pytest.raises(NotImplementedError, match="two critics"):
        _policy(n_critics=3)
    with pytest.raises(NotImplementedError, match="two critics"):
        _policy(n_critics=1)
    pol = _policy()
    with pytest.raises(NotImplementedError, match="n_runs"):
        pol.set_engine_options(n_runs=2)
    pol.set_engine_options(n_runs=1, precision=0)
    assert not hasattr(pol, "learn_n") and not hasattr(pol, "rollout_device")
    with pytest.raises(ValueError, match="real"):
        pol.learn({"observations": np.zeros((4, 5), np.float32)})


def test_fused_trainer_refuses_the_policy():
    import mb_trainer_fakes as fk
    from offlinerlkit.policy_trainer import MBPolicyTrainer
    from offlinerlkit.utils import termination_fns as tf

    class Dyn:
        term_kind = tf.term_kind(tf.termination_fn_halfcheetah)
    pol = _policy(dynamics=Dyn())
    kw = dict(epoch=1, step_per_epoch=fk.STEPS, batch_size=fk.BATCH, real_ratio=fk.REAL_RATIO, eval_episodes=1)
    with pytest.raises(ValueError, match="rollout_device"):
        MBPolicyTrainer(pol, fk.FakeEnv(), object(), object(), None, fk.ROLLOUT, fused=True, **kw)
    MBPolicyTrainer(pol, fk.FakeEnv(), object(), object(), None, fk.ROLLOUT, fused=False, **kw)


def test_dynamics_no_longer_refuses_sample_next_obss_and_abi_symbols():
    import inspect
    from offlinerlkit import _engine
    from offlinerlkit.dynamics import EnsembleDynamics
    assert "NotImplementedError" not in inspect.getsource(EnsembleDynamics.sample_next_obss)
    assert hasattr(EnsembleDynamics, "sample_next_obss_device")
    for sym in ("orl_dynsample_next", "orl_engine_set_next_samples", "orl_engine_lcb_penalty"):
        assert sym in _engine.ABI_SYMBOLS
    assert _engine.ALGO_ID["mobile"] == 6
    names = [f[0] for f in _engine.OrlConfig._fields_]
    assert names[-5:] == ["external_arena", "mobile_num_samples", "mobile_num_elites", "mobile_real_rows", "penalty_coef"]


def test_config_defaults_are_run_mobiles():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("orl_build", os.path.join(root, "offlinerl-kit_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from offlinerlkit import _engine
    cfg = _engine.default_config("mobile")
    assert (cfg.mobile_num_samples, cfg.mobile_num_elites, cfg.mobile_real_rows, cfg.deterministic_backup) == (10, 5, 12, 1)
    assert abs(cfg.penalty_coef - 1.5) < 1e-7 and cfg.external_arena is None and cfg.batch_size == 256
    # the nets are SAC's: same arena as an ORL_ALGO_SAC engine of the same shape
    lib = _engine.load_library()
    import ctypes
    assert lib.orl_arena_floats(ctypes.byref(cfg)) == lib.orl_arena_floats(ctypes.byref(_engine.default_config("sac")))
