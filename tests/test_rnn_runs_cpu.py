"""CPU: the host-only side of multi-run RNNDynamics objects (``orl_rnn_config::n_runs``): the config checks, which need no device, and
the new entry points' export and declaration."""
import os
import re

import pytest

import rnn_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN_SYMBOLS = ["orl_rnn_set_run", "orl_rnn_get_run", "orl_rnn_step_runs", "orl_rnn_learn_epoch_runs", "orl_rnn_forward_runs",
               "orl_rnn_debug_read_run", "orl_rnn_debug_grads_run"]


def _cfg(**over):
    from offlinerlkit import _engine
    c = rc.CASES["rnn_tiny"]
    return _engine.default_rnn_config(input_dim=c["input_dim"], output_dim=c["output_dim"], hidden=c["hidden"], rnn_num_layers=c["L"], **over)


def test_config_floats_is_the_per_run_size_and_n_runs_is_bounded():
    from offlinerlkit import _engine
    import ctypes
    lib = _engine.load_library()
    one = _engine.rnn_run_floats(_cfg(n_runs=1))
    assert one > 0 and one == _engine.rnn_config_floats(_cfg(n_runs=1))
    for R in (3, 64):
        cfg = _cfg(n_runs=R)
        assert lib.orl_rnn_config_floats(ctypes.byref(cfg)) == one and _engine.rnn_run_floats(cfg) == one      # the arena is n_runs times this
        with pytest.raises(RuntimeError, match="rnn_run_floats"):      # the one-run helper names the per-run one
            _engine.rnn_config_floats(cfg)
    for R in (0, 65, -1):
        cfg = _cfg(n_runs=R)
        assert lib.orl_rnn_config_floats(ctypes.byref(cfg)) < 0
        with pytest.raises(RuntimeError, match=r"n_runs must be in \[1, 64\]"):
            _engine.rnn_run_floats(cfg)


def test_run_entry_points_are_exported_and_declared():
    from offlinerlkit import _engine
    lib = _engine.load_library()
    header = open(os.path.join(ROOT, "include", "orl_engine.h")).read()
    declared = set(re.findall(r"\b(orl_[a-z0-9_]+)\s*\(", header))
    for sym in RUN_SYMBOLS:
        assert sym in declared, f"{sym} is not declared in include/orl_engine.h"
        assert sym in _engine.ABI_SYMBOLS
        assert hasattr(lib, sym), f"missing symbol {sym}"


def test_class_options_are_checked_without_a_device():
    import torch
    from offlinerlkit.dynamics import RNNDynamics, _fresh_rnn_params
    from offlinerlkit.nets import RNNModel
    from offlinerlkit.utils.scaler import StandardScaler
    m = RNNModel(5, 4, [24, 24], 1, 0.0)
    dyn = RNNDynamics(m, torch.optim.Adam(m.parameters(), lr=1e-3), StandardScaler(), rc.terminal_fn)
    for bad in (0, 65):
        with pytest.raises(ValueError, match="n_runs"):
            dyn.set_engine_options(n_runs=bad)
    dyn.set_engine_options(n_runs=3, seed=5)
    with pytest.raises(RuntimeError, match="only run 0"):
        dyn.select_run(2)
    with pytest.raises(ValueError, match="out of range"):
        dyn.select_run(3)
    # a run's fresh initialisation is the constructor's under that torch seed, and drawing it leaves the global stream alone
    torch.manual_seed(11)
    before = torch.get_rng_state()
    got = _fresh_rnn_params(m, 6)
    assert torch.equal(torch.get_rng_state(), before)
    torch.manual_seed(6)
    want = RNNModel(5, 4, [24, 24], 1, 0.0).state_dict()
    assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in want)
