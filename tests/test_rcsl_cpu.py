"""CPU: RCSL without a GPU -- the numpy oracle (tests/rcsl_oracle.py) against fixtures of the real reference ``RcslPolicy.learn``, the
state_dict key inventory, ``RcslPolicyTrainer`` against the trace of the real trainer, ``traj_rtg_datasets`` against the real function,
the epoch order builder and the constructor's refusals.  Fixtures: tests/golden/make_rcsl_golden.py."""
import multiprocessing

import numpy as np
import pytest
import torch

import rcsl_cases as rc
import rcsl_oracle as orc
from helpers import load_golden, rel_err, scale_err, check_state_against_golden


@pytest.mark.parametrize("case", list(rc.CASES))
def test_rcsl_oracle_matches_reference(case):
    """losses 1e-4 relative, parameters at test_oracle_golden.py's 2e-6 (k + 1) absolute, scaled by lr / 3e-4 (Adam's step is
    proportional to lr; the tiny cases run at 3e-4, hopper at run_rcsl.py's 1e-3)"""
    g = load_golden(case)
    c, net, batches = rc.case_inputs(case)
    st = orc.init_state(net)
    assert [str(k) for k in g["loss_keys"]] == ["loss"]
    for k, b in enumerate(batches):
        res, aux = orc.learn(st, c, b)
        assert list(res.keys()) == ["loss"]
        got, ref = np.array([res["loss"]]), g[f"step{k}/losses"]
        assert rel_err(got, ref, floor=1e-2) < 1e-4, (case, k, got, ref)
        if k == 0:
            assert scale_err(aux["pred"], g["step0/pred"]) < 1e-5
            for n, gr in aux["grads"].items():
                if f"step0/grads/{n}" in g.files:
                    assert scale_err(gr, g[f"step0/grads/{n}"]) < 1e-5, n
        check_state_against_golden(g, f"state{k}", {"rcsl": st["rcsl"]}, atol=2e-6 * (k + 1) * c["lr"] / 3e-4)


def test_masked_rows_are_the_partial_batch():
    """the oracle's validity mask: a batch padded with other rows and masked learns exactly what the valid rows alone teach"""
    c, net, batches = rc.case_inputs("rcsl_tiny")
    a, b = orc.init_state(net), orc.init_state(net)
    valid = np.arange(c["B"]) < 5
    ra, _ = orc.learn(a, c, {k: v[:5] for k, v in batches[0].items()})
    rb, aux = orc.learn(b, c, batches[0], valid)
    assert ra["loss"] == pytest.approx(rb["loss"], rel=1e-6) and not aux["dpred"][5:].any()
    for n in a["rcsl"]:
        assert np.abs(a["rcsl"][n] - b["rcsl"][n]).max() < 1e-7
    full, _ = orc.learn(orc.init_state(net), c, batches[0])
    assert abs(full["loss"] - ra["loss"]) > 1e-3 * abs(ra["loss"])


def _policy(hidden, od=5, ad=2, optim=torch.optim.Adam):
    from offlinerlkit.modules import RcslModule
    from offlinerlkit.nets import MLP
    from offlinerlkit.policy import RcslPolicy
    mod = RcslModule(MLP(input_dim=od + 1, hidden_dims=hidden, output_dim=ad), "cpu")
    return RcslPolicy(None, None, mod, optim(mod.parameters(), lr=1e-3), "cpu")


@pytest.mark.parametrize("case", list(rc.CASES))
def test_state_dict_keys_are_the_references(case):
    c = rc.CASES[case]
    pol = _policy(c["hidden"], c["obs_dim"], c["act_dim"])
    assert list(pol.state_dict().keys()) == [str(k) for k in load_golden(case)["keys"]]
    sd = pol.state_dict()
    assert tuple(sd[f"rcsl.backbone.model.{2 * len(c['hidden'])}.weight"].shape) == (c["act_dim"], c["hidden"][-1])


def test_module_forward_and_select_action_on_the_cpu():
    c, net, batches = rc.case_inputs("rcsl_tiny")
    pol = _policy(c["hidden"])
    pol.rcsl.load_state_dict({k: torch.from_numpy(v) for k, v in net.items()})
    b = batches[0]
    pred, _, _ = orc.forward(net, b["observations"], b["rtgs"])
    assert scale_err(pol.select_action(b["observations"], b["rtgs"]), pred) < 1e-5
    assert np.array_equal(pol.select_action(b["observations"], b["rtgs"][:, 0]), pol.select_action(b["observations"], b["rtgs"]))   # 1-D rtg


def test_refusals_need_no_gpu():
    with pytest.raises(NotImplementedError):
        _policy([32, 32], optim=torch.optim.SGD)
    with pytest.raises(NotImplementedError):
        _policy([16] * 5)
    _policy([16] * 4)
    with pytest.raises(NotImplementedError):
        _policy([16, 16]).rollout(np.zeros((1, 5), np.float32), 3)


@pytest.mark.parametrize("variant", list(rc.TRAINER_VARIANTS))
def test_trainer_matches_the_reference_trace(variant, monkeypatch):
    """logged keys in order, every row, timesteps, return value (with the reference's double append under eval_env2), scheduler steps,
    checkpoints, the rtg the policy was conditioned on at every evaluation step, the env seeds -- and, under the same torch seed, the
    batch order of the reference's shuffled DataLoader, partial last batch included.  No child process exists while it trains."""
    from offlinerlkit.policy_trainer import RcslPolicyTrainer
    g = load_golden("rcsl_trainer_trace")
    learn = rc.RecordingPolicy.learn

    def watched(self, batch):
        assert multiprocessing.active_children() == []
        return learn(self, batch)
    monkeypatch.setattr(rc.RecordingPolicy, "learn", watched)
    out = rc.run_trainer(RcslPolicyTrainer, variant, fused=False)
    assert multiprocessing.active_children() == []
    for k, v in out.items():
        ref = g[f"{variant}/{k}"]
        if v.dtype.kind == "f":
            assert v.shape == ref.shape and np.allclose(v, ref, rtol=1e-12, atol=0), (k, v, ref)
        else:
            assert np.array_equal(v, ref), (k, v, ref)
    assert list(out["order_lens"][:6]) == [8, 8, 8, 8, 8, 5]          # 45 rows in batches of 8: the partial batch goes through learn
    assert sorted(out["orders"][:rc.T_N]) == list(range(rc.T_N))


def test_trainer_refuses_a_mixed_offline_ratio():
    import tempfile
    from offlinerlkit.policy_trainer import RcslPolicyTrainer
    with tempfile.TemporaryDirectory() as d:
        tr = RcslPolicyTrainer(rc.RecordingPolicy(), rc.GymEnv(), rc.trainer_dataset(), rc.trainer_dataset(), rc.T_GOAL, rc.RecordingLogger(d), 0,
                               epoch=1, batch_size=8, offline_ratio=0.5, fused=False)
        with pytest.raises(NotImplementedError):
            tr.train()


def test_traj_rtg_datasets_equals_the_reference():
    from offlinerlkit.utils.load_dataset import traj_rtg_datasets, discount_cumsum
    g = load_golden("rcsl_dataset")
    for tag, use_to in (("timeouts", True), ("steps", False)):
        full, init_obss, max_ret = traj_rtg_datasets(rc.TrajEnv(use_to))
        assert set(full) == {"observations", "next_observations", "actions", "rewards", "rtgs", "terminals"}
        for k, v in full.items():
            assert v.dtype == g[f"{tag}/{k}"].dtype and np.array_equal(v, g[f"{tag}/{k}"]), (tag, k)
        assert init_obss.dtype == np.float32 and np.array_equal(init_obss, g[f"{tag}/init_obss"])
        assert max_ret == g[f"{tag}/max_return"][0]
    assert len(g["timeouts/rewards"]) == 231                          # rows behind the last trajectory end (230) are dropped
    x = np.array([1.0, 2.0, 3.0], np.float32)
    assert np.array_equal(discount_cumsum(x), [6.0, 5.0, 3.0]) and np.array_equal(discount_cumsum(x, 0.5), [2.75, 3.5, 3.0])


def test_epoch_order_visits_every_row_once_per_run():
    from offlinerlkit.policy.rcsl import epoch_order
    torch.manual_seed(3)
    n, B, R = 3 * 16 + 5, 16, 3
    o = epoch_order(n, B, R)
    assert o.shape == (R, 4 * B) and o.dtype == np.int64
    for r in range(R):
        assert sorted(o[r, :n]) == list(range(n)) and (o[r, n:] == -1).all()
    assert not np.array_equal(o[0], o[1]) and not np.array_equal(o[1], o[2])
    assert epoch_order(32, 16).shape == (1, 32) and (epoch_order(32, 16) >= 0).all()      # a full last batch: no padding
