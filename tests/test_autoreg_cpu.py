"""CPU: the autoregressive behaviour policy without a GPU -- the numpy oracle (tests/autoreg_oracle.py) against fixtures of the real
reference's ``AutoregressivePolicy`` (``learn``, one-row ``select_action``), the state_dict key inventory, the constructor's refusals, and
``rollout`` on fake collaborators against the reference's ``RcslPolicy.rollout``.  Fixtures: tests/golden/make_autoreg_golden.py."""
import numpy as np
import pytest
import torch

import autoreg_cases as ac
import autoreg_oracle as orc
from helpers import load_golden, rel_err, scale_err, check_state_against_golden


@pytest.mark.parametrize("case", list(ac.CASES))
def test_oracle_matches_reference(case):
    """losses 1e-4 relative, mean / logstd / step-0 gradients 1e-5 of scale, parameters at 2e-6 (k + 1) absolute scaled by lr / 3e-4
    (half the GPU tests' bar, as in tests/test_rcsl_cpu.py)"""
    g = load_golden(case)
    c, net, batches = ac.case_inputs(case)
    st = orc.init_state(net)
    assert [str(k) for k in g["loss_keys"]] == ["loss"]
    assert list(net.keys()) == [str(k) for k in g["keys"]]
    for k, b in enumerate(batches):
        res, aux = orc.learn(st, c, b)
        assert list(res.keys()) == ["loss"]
        got, ref = np.array([res["loss"]]), g[f"step{k}/losses"]
        assert rel_err(got, ref, floor=1e-2) < 1e-4, (case, k, got, ref)
        if k == 0:
            assert scale_err(aux["mean"], g["step0/mean"]) < 1e-5 and scale_err(aux["logstd"], g["step0/logstd"]) < 1e-5
            zt = aux["z_tail"]
            assert ((zt > 0).mean(axis=0) >= 0.1).all() and ((zt < 0).mean(axis=0) >= 0.1).all()      # both branches of the output LeakyReLU
            n_grads = 0
            for n, gr in aux["grads"].items():
                if f"step0/grads/{n}" in g.files:
                    assert scale_err(gr, g[f"step0/grads/{n}"]) < 1e-5, n
                    n_grads += 1
            assert n_grads == (len(net) if c["full"] or c.get("grads") else 0)
        check_state_against_golden(g, f"state{k}", {"model": st["model"]}, atol=2e-6 * (k + 1) * c["lr"] / 3e-4)


def test_expanded_rows_are_the_references():
    """row j * B + b = [obs_b | act_b[k] 1[k < j] | onehot_j], target act_b[j]"""
    obs = np.arange(6, dtype=np.float32).reshape(2, 3)
    act = np.array([[1, 2, 3], [4, 5, 6]], np.float32)
    x, t = orc.expand(obs, act)
    assert x.shape == (6, 9) and np.array_equal(t, [1, 4, 2, 5, 3, 6])
    assert np.array_equal(x[0], [0, 1, 2, 0, 0, 0, 1, 0, 0]) and np.array_equal(x[3], [3, 4, 5, 4, 0, 0, 0, 1, 0])
    assert np.array_equal(x[4], [0, 1, 2, 1, 2, 0, 0, 0, 1])


def test_masked_rows_are_the_partial_batch():
    """the oracle's validity mask: a batch padded with other rows and masked learns exactly what the valid rows alone teach"""
    c, net, batches = ac.case_inputs("ar_tiny")
    a, b = orc.init_state(net), orc.init_state(net)
    valid = np.arange(c["B"]) < 5
    ra, _ = orc.learn(a, c, {k: v[:5] for k, v in batches[0].items()})
    rb, aux = orc.learn(b, c, batches[0], valid)
    assert ra["loss"] == pytest.approx(rb["loss"], rel=1e-6)
    assert not aux["dz_tail"].reshape(c["act_dim"], c["B"], 2)[:, 5:].any()
    for n in a["model"]:
        assert np.abs(a["model"][n] - b["model"][n]).max() < 1e-7
    full, _ = orc.learn(orc.init_state(net), c, batches[0])
    assert abs(full["loss"] - ra["loss"]) > 1e-3 * abs(ra["loss"])


@pytest.mark.parametrize("case", list(ac.SAMPLE_CASES))
def test_oracle_sampling_matches_the_references_select_action(case):
    g = load_golden("ar_sample")
    _, net, _ = ac.case_inputs(case)
    a = orc.sample(net, ac.sample_obs(case), g[f"{case}/eps"])
    assert scale_err(a, g[f"{case}/actions"]) < 1e-6


def _policy(hidden=(32, 32), od=5, ad=2, lr=1e-3):
    from offlinerlkit.policy import AutoregressivePolicy
    return AutoregressivePolicy(od, ad, list(hidden), lr, "cpu")


@pytest.mark.parametrize("case", list(ac.CASES))
def test_state_dict_keys_are_the_references(case):
    c = ac.CASES[case]
    pol = _policy(c["hidden"], c["obs_dim"], c["act_dim"])
    assert list(pol.state_dict().keys()) == [str(k) for k in load_golden(case)["keys"]]
    sd = pol.state_dict()
    assert tuple(sd["model.0.weight"].shape) == (c["hidden"][0], c["obs_dim"] + 2 * c["act_dim"])
    assert tuple(sd[f"model.{2 * len(c['hidden'])}.weight"].shape) == (2, c["hidden"][-1])
    assert isinstance(pol.rcsl_optim, torch.optim.Adam) and pol.rcsl_optim.param_groups[0]["lr"] == 1e-3


def test_fit_restates_the_references_loss():
    c, net, batches = ac.case_inputs("ar_tiny")
    g = load_golden("ar_tiny")
    pol = _policy(c["hidden"], c["obs_dim"], c["act_dim"])
    pol.load_state_dict({k: torch.from_numpy(v) for k, v in net.items()})
    with torch.no_grad():
        loss = float(pol.fit(torch.from_numpy(batches[0]["observations"]), torch.from_numpy(batches[0]["actions"])))
    assert abs(loss - g["step0/losses"][0]) < 1e-5 * abs(g["step0/losses"][0])


def test_refusals_need_no_gpu():
    from offlinerlkit import _engine
    assert _engine.ALGO_ID["autoreg"] == _engine.ALGO_AUTOREG == 9 and "orl_autoreg_sample" in _engine.ABI_SYMBOLS
    _policy([16])
    _policy([16] * 4, ad=32)
    for why, kw in (("hidden layers", dict(hidden=[16] * 5)), ("hidden layers", dict(hidden=[])), ("act_dim", dict(ad=33))):
        with pytest.raises(NotImplementedError, match=why):
            _policy(**kw)
    p = _policy()
    p.rcsl_optim = torch.optim.SGD(p.model.parameters(), lr=1e-3)
    with pytest.raises(NotImplementedError, match="Adam"):
        p._dims()
    for kw in (dict(weight_decay=1e-4), dict(amsgrad=True)):
        p = _policy()
        p.rcsl_optim = torch.optim.Adam(p.model.parameters(), lr=1e-3, **kw)
        with pytest.raises(NotImplementedError, match="weight_decay / amsgrad"):
            p._dims()
    L, Lk = torch.nn.Linear, torch.nn.LeakyReLU
    for model in ([L(9, 32), torch.nn.ReLU(), L(32, 2), Lk()], [L(9, 32), Lk(0.2), L(32, 2), Lk()], [L(9, 32), Lk(), L(32, 3), Lk()],
                  [L(9, 32), Lk(), L(32, 2)], [L(8, 32), Lk(), L(32, 2), Lk()], [L(9, 2), Lk()]):
        p = _policy()
        p.model = torch.nn.ModuleList(model)
        with pytest.raises(NotImplementedError, match=r"Linear, LeakyReLU\(0.01\)"):
            p._dims()
    assert not hasattr(_policy(), "sample_init_noise")


def test_learn_needs_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    c, _, batches = ac.case_inputs("ar_tiny")
    with pytest.raises(RuntimeError, match="MI355X"):
        _policy(c["hidden"], c["obs_dim"], c["act_dim"]).learn(batches[0])


def _rcsl(dynamics, rollout_policy, gauss=False):
    from offlinerlkit.modules import DiagGaussian, RcslGaussianModule, RcslModule
    from offlinerlkit.nets import MLP
    from offlinerlkit.policy import RcslGaussianPolicy, RcslPolicy
    bb = MLP(input_dim=ac.R_OBS + 1, hidden_dims=[16, 16], output_dim=ac.R_ACT)
    if gauss:
        mod = RcslGaussianModule(bb, DiagGaussian(ac.R_ACT, ac.R_ACT, unbounded=True, conditioned_sigma=True), "cpu")
        return RcslGaussianPolicy(dynamics, rollout_policy, mod, torch.optim.Adam(mod.parameters(), lr=1e-3), "cpu")
    mod = RcslModule(bb, "cpu")
    return RcslPolicy(dynamics, rollout_policy, mod, torch.optim.Adam(mod.parameters(), lr=1e-3), "cpu")


@pytest.mark.parametrize("gauss", [False, True])
@pytest.mark.parametrize("name", list(ac.ROLLOUTS))
def test_rollout_matches_the_reference(name, gauss):
    """integer and boolean arrays exactly, floats at 1e-6; thinning at different steps, the early break when every trajectory has ended,
    both rollout-policy interfaces"""
    g = load_golden("ar_rollout")
    dyn, rp, init, horizon = ac.rollout_collaborators(name)
    tr, info = _rcsl(dyn, rp, gauss).rollout(init, horizon)
    keys = ["obss", "next_obss", "actions", "rewards", "terminals", "traj_idxs", "acc_rets", "rtgs"]
    assert list(tr.keys()) == keys and list(info.keys()) == ["num_transitions", "reward_mean", "returns"]
    for k in keys:
        ref = g[f"{name}/{k}"]
        assert tr[k].shape == ref.shape and tr[k].dtype == ref.dtype, (k, tr[k].shape, tr[k].dtype, ref.shape, ref.dtype)
        if ref.dtype.kind in "biu":
            assert np.array_equal(tr[k], ref), k
        else:
            assert np.abs(tr[k] - ref).max() <= 1e-6 * max(np.abs(ref).max(), 1.0), k
    assert tr["rtgs"].shape == (len(tr["obss"]), 1)
    assert info["num_transitions"] == int(g[f"{name}/info/num_transitions"][0]) == len(tr["obss"])
    assert abs(info["reward_mean"] - g[f"{name}/info/reward_mean"][0]) <= 1e-6
    assert np.abs(info["returns"] - g[f"{name}/info/returns"]).max() <= 1e-6
    if name == "all_end_early":
        assert len(tr["obss"]) < init.shape[0] * horizon and tr["terminals"][-1].all()


def test_rollout_still_needs_both_collaborators():
    dyn, rp, init, horizon = ac.rollout_collaborators("thinning_plain")
    for d, p in ((None, None), (dyn, None), (None, rp)):
        with pytest.raises(NotImplementedError, match="rollout"):
            _rcsl(d, p).rollout(init, horizon)
