"""No GPU: the fused actor sampling's ABI symbol and the rollout-precision switch's own bookkeeping."""
import os
import re

import pytest

from helpers import GOLDEN_DIR


def test_symbol_is_declared_listed_and_exported():
    from offlinerlkit import _engine
    with open(os.path.join(GOLDEN_DIR, "..", "..", "include", "orl_engine.h")) as fh:
        header = fh.read()
    assert re.search(r"\borl_actor_sample\(orl_engine\* e", header)
    assert "orl_actor_sample" in _engine.ABI_SYMBOLS
    assert _engine.load_library().orl_actor_sample is not None      # (ctypes resolves the name in the shared library or raises)


def test_policy_keeps_the_switch_without_an_engine():
    import torch
    from offlinerlkit.modules import ActorProb, Critic, TanhDiagGaussian
    from offlinerlkit.nets import MLP
    from offlinerlkit.policy import MOPOPolicy
    actor = ActorProb(MLP(5, [32, 32]), TanhDiagGaussian(32, 2, unbounded=True, conditioned_sigma=True), "cpu")
    c1, c2 = Critic(MLP(7, [32, 32]), "cpu"), Critic(MLP(7, [32, 32]), "cpu")
    adam = lambda m: torch.optim.Adam(m.parameters(), lr=1e-3)
    pol = MOPOPolicy(None, actor, c1, c2, adam(actor), adam(c1), adam(c2))
    assert pol._rollout_precision == 0 and pol._eng is None
    for p in (1, 0, 1):
        pol.set_rollout_precision(p)
        assert pol._rollout_precision == p and pol._eng is None
    for bad in (True, 2, -1):
        with pytest.raises(ValueError, match="0 or 1"):
            pol.set_rollout_precision(bad)
    assert pol._rollout_precision == 1
