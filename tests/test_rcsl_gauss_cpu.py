"""CPU: Gaussian RCSL without a GPU -- the numpy oracle (tests/rcsl_gauss_oracle.py) against fixtures of the real reference
``RcslGaussianPolicy.learn``, ``RcslGaussianModule`` against the fixtures' ``mu`` / ``logvar``, the state_dict key inventory and the
constructor's refusals.  Fixtures: tests/golden/make_rcsl_gauss_golden.py."""
import numpy as np
import pytest
import torch

import rcsl_gauss_cases as gc
import rcsl_gauss_oracle as orc
from helpers import load_golden, rel_err, scale_err, check_state_against_golden


@pytest.mark.parametrize("case", list(gc.CASES))
def test_oracle_matches_reference(case):
    """losses 1e-4 relative, mu / logvar / step-0 gradients 1e-5 of scale, parameters at 2e-6 (k + 1) absolute scaled by lr / 3e-4
    (half the GPU tests' bar, as in tests/test_rcsl_cpu.py)"""
    g = load_golden(case)
    c, net, batches = gc.case_inputs(case)
    st = orc.init_state(net)
    assert [str(k) for k in g["loss_keys"]] == ["loss"]
    assert list(net.keys()) == [str(k)[len("rcsl."):] for k in g["keys"]]
    for k, b in enumerate(batches):
        res, aux = orc.learn(st, c, b)
        assert list(res.keys()) == ["loss"]
        got, ref = np.array([res["loss"]]), g[f"step{k}/losses"]
        assert rel_err(got, ref, floor=1e-2) < 1e-4, (case, k, got, ref)
        if k == 0:
            assert scale_err(aux["mu"], g["step0/mu"]) < 1e-5 and scale_err(aux["logvar"], g["step0/logvar"]) < 1e-5
            clamped = (aux["raw"] < gc.LO) | (aux["raw"] > gc.HI)
            assert clamped.any() == (c["head"] == "clamp")
            for n, gr in aux["grads"].items():
                if f"step0/grads/{n}" in g.files:
                    assert scale_err(gr, g[f"step0/grads/{n}"]) < 1e-5, n
        check_state_against_golden(g, f"state{k}", {"rcsl": st["rcsl"]}, atol=2e-6 * (k + 1) * c["lr"] / 3e-4)


def test_clamped_entries_pass_no_gradient():
    """rcslg_tiny: action dimension 0 (sigma bias -5.5) sits below the lower bound on every row of step 0, so its row of the sigma
    head gets no gradient at all, while dimension 1 is clamped on some rows only and does"""
    c, net, batches = gc.case_inputs("rcslg_tiny")
    _, aux = orc.learn(orc.init_state(net), c, batches[0])
    clamped = (aux["raw"] < gc.LO) | (aux["raw"] > gc.HI)
    assert clamped[:, 0].all() and clamped[:, 1].any() and not clamped[:, 1].all()
    gw, gb = aux["grads"]["dist_net.sigma.weight"], aux["grads"]["dist_net.sigma.bias"]
    assert not gw[0].any() and gb[0] == 0 and gw[1].any() and gb[1] != 0


def test_masked_rows_are_the_partial_batch():
    """the oracle's validity mask: a batch padded with other rows and masked learns exactly what the valid rows alone teach"""
    c, net, batches = gc.case_inputs("rcslg_tiny")
    a, b = orc.init_state(net), orc.init_state(net)
    valid = np.arange(c["B"]) < 5
    ra, _ = orc.learn(a, c, {k: v[:5] for k, v in batches[0].items()})
    rb, aux = orc.learn(b, c, batches[0], valid)
    assert ra["loss"] == pytest.approx(rb["loss"], rel=1e-6) and not aux["dz"][5:].any()
    for n in a["rcsl"]:
        assert np.abs(a["rcsl"][n] - b["rcsl"][n]).max() < 1e-7
    full, _ = orc.learn(orc.init_state(net), c, batches[0])
    assert abs(full["loss"] - ra["loss"]) > 1e-3 * abs(ra["loss"])


def _policy(hidden, od=5, ad=2, optim=torch.optim.Adam, latent=None, out=None, **dist):
    from offlinerlkit.modules import DiagGaussian, RcslGaussianModule
    from offlinerlkit.nets import MLP
    from offlinerlkit.policy import RcslGaussianPolicy
    kw = dict(unbounded=True, conditioned_sigma=True)
    kw.update(dist)
    mod = RcslGaussianModule(MLP(input_dim=od + 1, hidden_dims=hidden, output_dim=out or ad), DiagGaussian(latent or ad, ad, **kw), "cpu")
    return RcslGaussianPolicy(None, None, mod, optim(mod.parameters(), lr=1e-3), "cpu")


@pytest.mark.parametrize("case", list(gc.CASES))
def test_state_dict_keys_are_the_references(case):
    c = gc.case_dict(case)
    pol = _policy(c["hidden"], c["obs_dim"], c["act_dim"])
    assert list(pol.state_dict().keys()) == [str(k) for k in load_golden(case)["keys"]]
    sd = pol.state_dict()
    A = c["act_dim"]
    assert tuple(sd[f"rcsl.backbone.model.{2 * len(c['hidden'])}.weight"].shape) == (A, c["hidden"][-1])
    assert tuple(sd["rcsl.dist_net.mu.weight"].shape) == tuple(sd["rcsl.dist_net.sigma.weight"].shape) == (A, A)


@pytest.mark.parametrize("case", ["rcslg_tiny", "rcslg_odd", "rcslg_act32"])
def test_module_matches_the_fixture(case):
    """get_dist_params -> (mu, logvar) of the fixture; forward -> NormalWrapper(mu, exp(logvar)); select_action samples it"""
    from offlinerlkit.modules import NormalWrapper
    c, net, batches = gc.case_inputs(case)
    g = load_golden(case)
    pol = _policy(c["hidden"], c["obs_dim"], c["act_dim"])
    pol.rcsl.load_state_dict({k: torch.from_numpy(v) for k, v in net.items()})
    b = batches[0]
    with torch.no_grad():
        mu, logvar = pol.rcsl.get_dist_params(b["observations"], b["rtgs"])
        dist = pol.rcsl(b["observations"], b["rtgs"][:, 0])                      # 1-D rtg
    assert scale_err(mu.numpy(), g["step0/mu"]) < 1e-5 and scale_err(logvar.numpy(), g["step0/logvar"]) < 1e-5
    assert isinstance(dist, NormalWrapper)
    assert scale_err(dist.mean.numpy(), g["step0/mu"]) < 1e-5 and scale_err(dist.scale.numpy(), np.exp(g["step0/logvar"])) < 1e-5
    torch.manual_seed(3)
    a = pol.select_action(b["observations"], b["rtgs"])
    torch.manual_seed(3)
    want = g["step0/mu"] + np.exp(g["step0/logvar"]) * torch.randn(mu.shape).numpy()
    assert a.shape == mu.shape and scale_err(a, want) < 1e-5


def test_refusals_need_no_gpu():
    _policy([32, 32])
    _policy([16] * 4)
    for why, kw in (("Adam", dict(optim=torch.optim.SGD)), ("hidden layers", dict(hidden=[16] * 5)), ("unbounded", dict(unbounded=False)),
                    ("conditioned_sigma", dict(conditioned_sigma=False)), ("latent_dim", dict(latent=4, out=4)),
                    ("clamps", dict(sigma_min=-20.0)), ("clamps", dict(sigma_max=1.0))):
        kw = dict(dict(hidden=[32, 32]), **kw)
        with pytest.raises(NotImplementedError, match=why):
            _policy(**kw)
    with pytest.raises(NotImplementedError, match="Linear, ReLU"):
        from offlinerlkit.nets import MLP
        p = _policy([32, 32])
        p.rcsl.backbone = MLP(input_dim=6, hidden_dims=[32, 32], output_dim=2, activation=torch.nn.Tanh)
        p._dims()
    with pytest.raises(NotImplementedError, match="rollout"):
        _policy([16, 16]).rollout(np.zeros((1, 5), np.float32), 3)


def test_engine_knows_the_algorithm_id():
    from offlinerlkit import _engine
    assert _engine.ALGO_ID["rcsl_gauss"] == _engine.ALGO_RCSL_GAUSS == 8
