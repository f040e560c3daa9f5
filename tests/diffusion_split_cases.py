"""DiffusionBC sampling at sample precision 1 (csrc/diffusion_fused.hip): the nets, row counts and float64 references of
tests/test_gpu_diffusion_split.py.

The reference is ``diffusion_oracle.sample(..., dtype=np.float64, trace=...)`` with teacher-forced z and init_noise.  The oracle's trace
holds every pass's x0 before the clip, so the x that enters the last pass (t = 0) is rebuilt from it with the fp32 schedule table the
oracle itself uses, and one ``forward(keep=True)`` on that x gives the stages the engine's ``s.*`` taps hold.  D32 of a stage is the
distance of the same procedure in fp32 from the float64 one; a split-fp16 stage is held to SPLIT x BAR x D32: BAR = 4 is the project's
margin over D32 (tests/diffusion_wide_cases.py), SPLIT = 4 = 2^-22 / 2^-24 the operand rounding of two fp16 planes against fp32's."""
import functools

import numpy as np

import diffusion_cases as dc
import diffusion_oracle as orc
import diffusion_wide_cases as wc
from helpers import scale_err

SPLIT = 4.0
CASES = {
    "cg2": dict(wc._BASE, down_dims=[16, 32], seed=1201),                   # groups of 2 and 4 channels: 8 / 4 groups per 16-column fragment
    "W": dict(wc._BASE, n_groups=2, down_dims=[64, 256], dsed=32, seed=1202),   # groups of 32 and of the limit, 128; every tile at 4100 rows
    "H": wc.CASES["H"],                                                     # identity residual read from the two ranges of [x | skip]
    "A": wc.CASES["A"],                                                     # groups of 64, 65 (odd, 128-column slab) and 128; [x | skip] split at 65
}
# 1, 17, 33: row tails of the 16-row tile; 65: past two 32-row tiles; 4100 x W3: enough workgroups for the 32-row and 128-column tiles
CASES["W3"] = dict(CASES["W"], N=3)                                           # fewer passes where the oracle has 4100 rows to do
RUNS = [(n, r) for n in "cg2 W H A".split() for r in (1, 17, 33, 65)] + [("W3", 4100)]


def stage_names(c):
    nb = len(orc.block_plan(c["act_dim"], c["down_dims"])[0])
    return ["film"] + [f"{s}.{b}" for b in range(nb) for s in ("y1", "out")] + ["yf", "pred"]


def run_oracle(P, c, obs, noise, z, dtype):
    """-> the sampled actions and the stages of the last pass"""
    from offlinerlkit.policy.diffusion import ddpm_schedule
    coef = ddpm_schedule(c["N"])[2]
    trace = []
    act = orc.sample(P, c, obs, noise, z, dtype=dtype, trace=trace)
    x = noise.reshape(len(obs), -1).astype(np.float32).astype(dtype)
    for t in range(c["N"] - 1, 0, -1):
        x = (coef[t, 2] * np.clip(trace[c["N"] - 1 - t], -1.0, 1.0).astype(dtype) + coef[t, 3] * x).astype(dtype)
        x = (x + coef[t, 4] * z[t]).astype(dtype)
    pred, A = orc.forward(P, c, x, np.zeros(len(obs), np.int64), obs, dtype=dtype, keep=True)
    out = dict(act=act, film=np.concatenate([b["film"] for b in A["blocks"]], axis=1), yf=A["yf"], pred=pred)
    for b, blk in enumerate(A["blocks"]):
        out[f"y1.{b}"], out[f"out.{b}"] = blk["y1"], A["outs"][b]
    return out


def reference_for(P, c, rows):
    obs, noise, z = wc.make_sample_inputs(c, rows)
    o32, o64 = run_oracle(P, c, obs, noise, z, np.float32), run_oracle(P, c, obs, noise, z, np.float64)
    return dict(c=c, P=P, obs=obs, noise=noise, z=z, o64=o64, D32={s: scale_err(o32[s], o64[s]) for s in o64})


@functools.lru_cache(maxsize=None)
def reference(name, rows):
    """per (case, rows), computed once and read-only: parameters, inputs, the float64 oracle's actions and last-pass stages, D32"""
    c = CASES[name]
    return reference_for(dc.make_params(c, wc.shapes_of(c)), c, rows)


def check(got, ref, tag):
    """engine actions and taps against the float64 oracle: every stage and the actions within SPLIT x BAR x D32, the actions also
    inside the project's gate.  Prints every err / D32 before it asserts; returns them."""
    ratios = {}
    for s in ["act"] + stage_names(ref["c"]):
        assert ref["D32"][s] > 0.0, (tag, s)
        ratios[s] = scale_err(np.asarray(got[s]).reshape(ref["o64"][s].shape), ref["o64"][s]) / ref["D32"][s]
    gate = scale_err(got["act"], ref["o64"]["act"])
    worst = max(ratios, key=ratios.get)
    print(f"{tag}: worst err / D32 {ratios[worst]:.2f} at {worst} (bar {SPLIT * wc.BAR:.0f}); actions {gate:.2e} of the {wc.GATE:.0e} gate")
    print("    " + ", ".join(f"{k} {v:.2f}" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v <= SPLIT * wc.BAR}
    assert not bad, (tag, "err / D32 above 16", bad)
    assert gate < wc.GATE, (tag, gate)
    return ratios
