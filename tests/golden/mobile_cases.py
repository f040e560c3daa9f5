"""Deterministic synthetic inputs of the MOBILE fixtures, shared by the generator (make_mobile_golden.py feeds them to the real
reference) and by the tests (which feed the very same arrays to tests/mobile_oracle.py and to the HIP engines).  Pure numpy on top of
synth.py; no reference code involved.  Everything derives from ``np.random.RandomState(seed)``: the fixtures hold the reference's
outputs, not the inputs."""
from collections import OrderedDict

import numpy as np

import synth

f32 = np.float32

# B_real + B_fake rows per batch, real rows first.  ``rew_shift`` moves the synthetic N(0, 1) rewards so that the clamp at 0 of the TD
# target is active on a fraction of the rows that the generator asserts to lie in [10 %, 90 %] at step 0.  0 does that where the critics'
# values are small next to the rewards' spread; mobile_ws adds the entropy bonus -alpha logp' of six action dims (about +3) to every
# target, which its shift takes back.
CASES = {
    # smallest shape on which the row order (S, E, B), the elite order, the real-row mask, the unbiased std and the clamp can each be wrong
    "mobile_tiny": dict(obs_dim=5, act_dim=2, hidden=[32, 32], dyn_hidden=[16, 16], K=4, elite_idx=[2, 0, 3], S=3, B_real=4, B_fake=12,
                        steps=3, seed=701, penalty_coef=1.0, det=False, rew_shift=0.0, over={}),
    "mobile_tiny_fixed_alpha_det": dict(obs_dim=5, act_dim=2, hidden=[32, 32], dyn_hidden=[16, 16], K=4, elite_idx=[2, 0, 3], S=3, B_real=4,
                                        B_fake=12, steps=3, seed=702, penalty_coef=1.0, det=True, rew_shift=0.0,
                                        over=dict(auto_alpha=False, alpha=0.2)),
    # 4 * 5 * 256 = 5 120 penalty rows: over the 4096-row threshold of the weight-stationary launches and no multiple of it
    "mobile_ws": dict(obs_dim=17, act_dim=6, hidden=[256, 256], dyn_hidden=[200, 200, 200, 200], K=7, elite_idx=[6, 1, 3, 0, 4], S=4,
                      B_real=12, B_fake=244, steps=1, seed=71, penalty_coef=1.0, det=False, rew_shift=-3.0, over={}),
    # run_mobile.py's defaults: 10 samples x 5 elites x 256 rows = 12 800 penalty rows, penalty_coef 1.5, deterministic backup
    "mobile_default": dict(obs_dim=17, act_dim=6, hidden=[256, 256], dyn_hidden=[200, 200, 200, 200], K=7, elite_idx=[6, 1, 3, 0, 4], S=10,
                           B_real=12, B_fake=244, steps=1, seed=72, penalty_coef=1.5, det=True, rew_shift=0.0, over={}),
}


def make_dynamics(rng, c):
    """EnsembleDynamicsModel parameters in state_dict names (weights (K, in, out), biases (K, 1, out)): the constructor's magnitudes
    (normal weights of std 1 / (2 sqrt(in)), max / min_logvar 0.5 / -10) with small biases and a spread in max_logvar so that the
    members, the dims and both soft clamps differ"""
    od, ad, K = c["obs_dim"], c["act_dim"], c["K"]
    D = od + 1
    dims = [od + ad] + list(c["dyn_hidden"]) + [2 * D]
    st = OrderedDict()
    st["max_logvar"] = (0.5 + 0.1 * rng.standard_normal(D)).astype(f32)
    st["min_logvar"] = (-10.0 + 0.1 * rng.standard_normal(D)).astype(f32)
    for l in range(len(dims) - 1):
        i, o = dims[l], dims[l + 1]
        pre = f"backbones.{l}." if l < len(dims) - 2 else "output_layer."
        st[pre + "weight"] = (rng.standard_normal((K, i, o)) / (2.0 * np.sqrt(i))).astype(f32)
        st[pre + "bias"] = (0.05 * rng.standard_normal((K, 1, o))).astype(f32)
    # the log-variance half of the output bias: std around exp(-1) so that the samples spread without swamping the members' means
    st["output_layer.bias"][:, :, D:] -= 2.0
    return st


def case_inputs(case):
    """-> (case dict, policy state, dynamics state, (scaler mu, std) of shape (1, obs + act), batches, noises).  noises[k]: ``dyn``
    (S, E, B, obs_dim + 1), ``eps_lcb`` (S * E * B, A), ``eps_next`` (B, A), ``eps_actor`` (B, A): the reference's draw order."""
    c = CASES[case]
    rng = np.random.RandomState(c["seed"])
    od, ad = c["obs_dim"], c["act_dim"]
    state = synth._sac_like_state(rng, c)
    dyn = make_dynamics(rng, c)
    mu = (0.25 * rng.standard_normal((1, od + ad))).astype(f32)
    std = (1.0 + 0.5 * rng.uniform(size=(1, od + ad))).astype(f32)
    B, S, E = c["B_real"] + c["B_fake"], c["S"], len(c["elite_idx"])
    batches, noises = [], []
    for _ in range(c["steps"]):
        b = synth._split_batch(rng, c)
        for part in b.values():
            part["rewards"] = (part["rewards"] + f32(c["rew_shift"])).astype(f32)
        batches.append(b)
        noises.append(OrderedDict(dyn=rng.standard_normal((S, E, B, od + 1)).astype(f32),
                                  eps_lcb=rng.standard_normal((S * E * B, ad)).astype(f32),
                                  eps_next=rng.standard_normal((B, ad)).astype(f32),
                                  eps_actor=rng.standard_normal((B, ad)).astype(f32)))
    return c, state, dyn, (mu, std), batches, noises


def oracle_cfg(c):
    from oracle import sac as osac
    cfg = osac.default_cfg(c["obs_dim"], c["act_dim"])
    cfg.update(hidden=c["hidden"], penalty_coef=c["penalty_coef"], num_samples=c["S"], deterministic_backup=c["det"],
               real_rows=c["B_real"], elites=list(c["elite_idx"]))
    cfg.update(c["over"])
    return cfg
