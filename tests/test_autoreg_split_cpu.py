"""No GPU: the sample-precision option of the autoregressive policy -- the two ABI symbols and the policy's own bookkeeping."""
import os
import re

import pytest

from helpers import GOLDEN_DIR

NAMES = ("orl_autoreg_set_sample_precision", "orl_autoreg_sample_precision")


def test_symbols_are_declared_listed_and_exported():
    from offlinerlkit import _engine
    with open(os.path.join(GOLDEN_DIR, "..", "..", "include", "orl_engine.h")) as fh:
        header = fh.read()
    lib = _engine.load_library()
    for n in NAMES:
        assert re.search(rf"\b{n}\(orl_engine\* e", header), n
        assert n in _engine.ABI_SYMBOLS, n
        assert getattr(lib, n) is not None, n                 # (ctypes resolves the name in the shared library or raises)


def test_policy_keeps_the_option_without_an_engine():
    from offlinerlkit.policy import AutoregressivePolicy
    pol = AutoregressivePolicy(5, 2, [32, 32], 1e-3, "cpu")
    assert pol._sample_precision == 0 and pol._eng is None
    for p in (1, 0, 1):
        pol.set_sample_precision(p)
        assert pol._sample_precision == p and pol._eng is None
    for bad in (2, -1, True, 0.5):
        with pytest.raises(ValueError, match="0 or 1"):
            pol.set_sample_precision(bad)
    assert pol._sample_precision == 1
