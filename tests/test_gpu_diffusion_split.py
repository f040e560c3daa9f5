"""GPU: DiffusionBC's sampler at sample precision 1 -- the fused Linear + GroupNorm + Mish kernel on split-fp16 MFMAs
(csrc/diffusion_fused.hip) -- against the float64 numpy oracle, stage by stage and at the sampled actions; the switch, the plane
cache, the range flag and the policy class.  Cases, references and the bar (16 x D32, the 1e-4 gate on the actions):
tests/diffusion_split_cases.py.  Measured err / D32 per case: profiles/diffusion_sample_split_accuracy.json."""
import numpy as np
import pytest

import diffusion_oracle as orc
import diffusion_split_cases as sc
import diffusion_wide_cases as wc
from test_gpu_diffusion import make_engine, unpack

pytestmark = pytest.mark.gpu


def sample_with_taps(eng, ref):
    c, rows = ref["c"], len(ref["obs"])
    got = dict(act=eng.sample(ref["obs"], ref["noise"].reshape(rows, -1), z=ref["z"]))
    for s in sc.stage_names(c):
        got[s] = eng.debug_read("s." + s, cap=ref["o64"][s].size)
    return got


@pytest.mark.parametrize("name,rows", sc.RUNS)
def test_split_sampling_against_the_float64_oracle(name, rows):
    ref = sc.reference(name, rows)
    eng, _ = make_engine(ref["c"])
    try:
        eng.set_sample_precision(1)
        assert eng.sample_precision == 1
        sc.check(sample_with_taps(eng, ref), ref, f"{name} x {rows}")
    finally:
        eng.close()


def test_the_switch_back_and_the_plane_cache():
    ref = sc.reference("H", 17)
    c, args = ref["c"], (ref["obs"], ref["noise"].reshape(17, -1))
    eng, P = make_engine(c)
    plain, _ = make_engine(c)
    try:
        eng.set_sample_precision(1)
        first = eng.sample(*args, z=ref["z"])
        eng.set_sample_precision(0)
        back, never = eng.sample(*args, z=ref["z"]), plain.sample(*args, z=ref["z"])
        assert np.array_equal(back, never) and not np.array_equal(back, first)
        assert np.array_equal(eng.debug_read("s.pred"), plain.debug_read("s.pred"))       # the taps at precision 0
        # one optimizer step at lr 1e-3 moves the EMA (decay 0: the new parameters); the planes must follow it
        eng.set_lr(np.full(4, 1e-3))
        eng.set_sample_precision(1)
        eng.step(np.arange(c["B"], dtype=np.int64))
        P2 = unpack(eng, eng.get(eng.EMA), P)
        assert not np.array_equal(eng.get(eng.EMA), plain.get(plain.EMA))
        ref2 = sc.reference_for(P2, c, 17)
        got = sample_with_taps(eng, ref2)
        assert not np.array_equal(got["act"], first)
        sc.check(got, ref2, "H x 17 after a step")
    finally:
        eng.close()
        plain.close()


def test_refusals():
    from offlinerlkit import _engine
    eng, _ = make_engine(sc.CASES["H"])
    wide, _ = make_engine(wc.CASES["B"])                     # one group of 512 channels
    try:
        with pytest.raises(RuntimeError, match="must be 0 .* or 1"):
            eng.set_sample_precision(2)
        assert eng.sample_precision == 0
        with pytest.raises(RuntimeError, match="512 channels is wider than the 128"):
            wide.set_sample_precision(1)
        wide.set_sample_precision(0)
        with pytest.raises(RuntimeError, match="unknown tap"):
            eng.debug_read("s.gf")
        with pytest.raises(RuntimeError, match="nothing recorded"):
            eng.debug_read("s.yf")
    finally:
        eng.close()
        wide.close()


def test_range_flag_is_raised_and_cleared():
    ref = sc.reference("H", 17)
    eng, _ = make_engine(ref["c"])
    try:
        eng.set_sample_precision(1)
        args = (ref["noise"].reshape(17, -1),)
        good = eng.sample(ref["obs"], *args, z=ref["z"])
        far = ref["obs"].copy()
        far[3, 1] = 1e6                                       # finite, beyond what an fp16 hi plane holds
        with pytest.raises(RuntimeError, match="range flag: an activation"):
            eng.sample(far, *args, z=ref["z"])
        assert np.array_equal(eng.sample(ref["obs"], *args, z=ref["z"]), good)
    finally:
        eng.close()


def test_policy_class_runs_the_split_sampler(tmp_path):
    import torch
    from test_gpu_diffusion import DEV, _policy
    import diffusion_cases as dc
    c = dc.CASES["d"]
    pol = _policy(c, tmp_path)
    pol.set_sample_precision(1)                               # before the engine exists
    obs = torch.as_tensor(np.random.RandomState(2).standard_normal((5, c["obs_dim"])).astype(np.float32), device=DEV)
    table = pol.sample_init_noise(9)
    idx = torch.as_tensor([8, 0, 3, 3, 5], device=DEV)
    eng = pol._engine()
    assert eng.sample_precision == 1
    direct = eng.sample(obs, table.reshape(9, -1).contiguous(), noise_idx=idx)
    # z comes from Philox keyed by (seed, call counter): compare the first call of policies built alike
    pol2 = _policy(c, tmp_path / "b")
    got = pol2.select_action_device(obs, table, noise_index=idx)
    assert pol2._engine().sample_precision == 0
    pol3 = _policy(c, tmp_path / "c")
    pol3._engine()
    pol3.set_sample_precision(1)                              # after the engine exists
    got1 = pol3.select_action_device(obs, table, noise_index=idx)
    assert torch.equal(got1, direct) and not torch.equal(got, direct)
    assert float((got1 - got).abs().max()) < 1e-3
