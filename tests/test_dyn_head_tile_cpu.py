"""The step_head option of the dynamics ensemble (k_dyn_head_tile) as far as it shows without a GPU: the config
field, its default, and that it adds no C function and moves no parameter."""
import pytest

from offlinerlkit import _engine


def test_step_head_config_field():
    assert _engine.default_dyn_config().step_head == 0
    cfg = _engine.default_dyn_config(step_head=1)
    assert cfg.step_head == 1 and cfg.precision == 0 and cfg.external_arena is None
    assert _engine.OrlDynConfig._fields_[-2:] == [("external_arena", _engine.C.c_void_p), ("step_head", _engine.C.c_int32)]
    lib = _engine.load_library()
    over = dict(obs_dim=3, act_dim=2, hidden=[32, 32], num_ensemble=3, num_elites=2)
    assert lib.orl_dyn_config_floats(_engine.default_dyn_config(step_head=1, **over)) == lib.orl_dyn_config_floats(_engine.default_dyn_config(**over))
    assert len([s for s in _engine.ABI_SYMBOLS if s.startswith("orl_dyn_")]) == 24
    assert isinstance(_engine.Dynamics.step_head, property)
    with pytest.raises(RuntimeError, match="step_head must be 0"):          # refused before any device is looked for
        _engine.Dynamics(_engine.default_dyn_config(step_head=2))
