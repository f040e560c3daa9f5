"""Synthetic inputs of the Gaussian-RCSL fixtures, shared by make_rcsl_gauss_golden.py (which feeds them to the real reference) and by the
tests (numpy oracle, HIP engine).  Backbones, batches and the ordered-epoch dataset are rcsl_cases'; this file adds the DiagGaussian head
(``dist_net.{mu, sigma}.{weight, bias}``, both A x A) and three shapes of its own.  Pure numpy; no reference code.

The head decides how much of the clamp(-5, 2) on the sigma output a case exercises:
  "clamp"  weights U(+-1/sqrt(A)) (nn.Linear's init), the sigma bias spread over linspace(-5.5, 2.5, A): both bounds are active.  The head's
           seed (RandomState(case seed + 500 + offset), draws in the order mu.weight, mu.bias, sigma.weight) is chosen so that at every
           one of the 4 steps IN THE REFERENCE at least 3 % of the values are clamped at each bound, at most 75 % in total, and no
           pre-clamp value lies within 1e-3 of max |pre-clamp| of either bound (10x the 1e-4 bar of the taps): the tests do not hinge on
           which side of a bound a value falls.  make_rcsl_gauss_golden.py asserts all of it (and finds such offsets: --search).
  "open"   sigma.weight scaled by 0.05 and the bias spread over linspace(-3, 0, A): nothing is clamped and every value stays at least 1
           inside the bounds at every step (asserted by the generator).  These cases cover a shape, not the mask: among 768 values x 4 steps
           (hopper) no head seed of 120 kept the 1e-3 margin with both bounds active.
"""
from collections import OrderedDict

import numpy as np

import rcsl_cases as rc

f32 = np.float32
STEPS = rc.STEPS
LO, HI = -5.0, 2.0
CASES = {
    # input width 6: no multiple of 4
    "rcslg_tiny": dict(base="rcsl_tiny", head="clamp", offset=5),
    "rcslg_odd": dict(base="rcsl_odd", head="clamp", offset=2),
    # run_rcsl.py's shape on hopper
    "rcslg_hopper": dict(base="rcsl_hopper", head="open", offset=5),
    # run_rcsl_gauss.py's default width (two layers of it).  lr 3e-4 and returns-to-go up to 600: at the launcher's 1e-3 on returns of 3200
    # the sigma output of this net swings by +-50 within the 4 steps and no head stays open, nor 25 % of its values unclamped
    "rcslg_wide": dict(obs_dim=11, act_dim=3, hidden=[1024, 1024], B=32, lr=3e-4, seed=74, rtg_hi=600.0, full=False, head="open", offset=1),
    # the act_dim ceiling of the head kernel (no "clamp" head seed of 120 keeps the margin on 256 values x 4 steps: an open head)
    "rcslg_act32": dict(obs_dim=6, act_dim=32, hidden=[32], B=8, lr=3e-4, seed=75, rtg_hi=100.0, full=True, head="open", offset=2),
}


def case_dict(case):
    c = dict(CASES[case])
    if "base" in c:
        c = dict(rc.CASES[c["base"]], **c)
    return c


def make_head(c, run=0, offset=None):
    A = c["act_dim"]
    off = c.get("offset", 0) if offset is None else offset
    rng = np.random.RandomState(c["seed"] + 1000 * run + 500 + off)
    k = 1.0 / np.sqrt(A)
    h = OrderedDict()
    h["dist_net.mu.weight"] = rng.uniform(-k, k, (A, A)).astype(f32)
    h["dist_net.mu.bias"] = rng.uniform(-k, k, A).astype(f32)
    w = rng.uniform(-k, k, (A, A)).astype(f32)
    if c["head"] == "clamp":
        h["dist_net.sigma.weight"] = w
        h["dist_net.sigma.bias"] = np.linspace(-5.5, 2.5, A).astype(f32)
    else:
        h["dist_net.sigma.weight"] = (f32(0.05) * w).astype(f32)
        h["dist_net.sigma.bias"] = np.linspace(-3.0, 0.0, A).astype(f32)
    return h


def case_inputs(case, run=0, offset=None):
    """(case dict, initial net = backbone + head, STEPS batches); ``run`` > 0: other weights and batches of the same shape"""
    c = case_dict(case)
    if "base" in c:
        _, net, batches = rc.case_inputs(c["base"], run)
    else:
        rng = np.random.RandomState(c["seed"] + 1000 * run)
        net = rc.make_net(rng, c)
        batches = [rc.make_rows(rng, c["B"], c) for _ in range(STEPS)]
    net = OrderedDict(net)
    net.update(make_head(c, run, offset))
    return c, net, batches


def epoch_inputs(n_runs=3, n_epochs=2):
    """rcsl_cases' ordered-epoch dataset and orders (N = 3 B + 5 rows of the tiny shape)"""
    _, data, orders = rc.epoch_inputs("rcsl_tiny", n_runs, n_epochs)
    return case_dict("rcslg_tiny"), data, orders
