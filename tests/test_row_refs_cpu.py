"""CPU: the value-with-bound type of tests/row_refs.py on cases with a known answer, and every restatement against the fp32 numpy
oracle's matching intermediate on random inputs -- the oracle's fp32 result must lie inside the restatement's OWN bound.  This proves the
float64 references before tests/test_gpu_row_kernels.py lets them judge a kernel."""
import math

import numpy as np
import pytest

import row_refs as rr
import synth
from helpers import clone_state
from oracle import cql as ocql, edac as oedac, iql as oiql, nn, td3bc as otd3
from row_refs import BV, FACTOR, U

f32 = np.float32


def inside(got, ref, tag, factor=FACTOR):
    r = rr.ratio(got, ref)
    assert r <= factor, (tag, r)
    return r


# ---------------------------------------------------------------------------------------------------------------------------------
# the bound type
# ---------------------------------------------------------------------------------------------------------------------------------
def test_single_operations_bound_one_rounding():
    rng = np.random.RandomState(0)
    x = (rng.standard_normal(4096) * 10.0 ** rng.uniform(-6, 6, 4096)).astype(f32)
    y = (rng.standard_normal(4096) * 10.0 ** rng.uniform(-6, 6, 4096)).astype(f32)
    X, Y = BV.exact(x), BV.exact(y)
    assert (X.e == 0).all() and np.array_equal(X.v, x.astype(np.float64))
    for got, ref in ((x + y, X + Y), (x - y, X - Y), (x * y, X * Y), (x / y, X / Y)):
        assert inside(got, ref, "op", factor=1.0) <= 1.0          # a correctly rounded operation loses at most u |z|
        assert (ref.e <= U * np.abs(ref.v) + rr.TINY).all() and (ref.e >= 0.5 * U * np.abs(ref.v)).all()
    # operands that are not fp32 numbers enter as what fp32 holds of them
    assert BV.exact(0.1).v == float(f32(0.1)) and BV.exact(3).v == 3.0


def test_error_propagates_through_the_derivatives():
    x, y = BV(np.array([2.0]), np.array([1e-3])), BV(np.array([-5.0]), np.array([2e-3]))
    assert math.isclose((x + y).e[0], 3e-3 + U * 3.0)
    assert math.isclose((x - y).e[0], 3e-3 + U * 7.0)
    assert math.isclose((x * y).e[0], 5.0 * 1e-3 + 2.0 * 2e-3 + U * 10.0 + rr.TINY)
    assert math.isclose((x / y).e[0], 1e-3 / 5.0 + 2.0 * 2e-3 / 25.0 + U * 0.4 + rr.TINY)
    assert math.isclose(rr.exp(x).e[0], math.exp(2.0) * (1e-3 + 2 * U) + rr.TINY)
    assert math.isclose(rr.log(x).e[0], 1e-3 / 2.0 + 2 * U * math.log(2.0) + rr.TINY)
    assert math.isclose(rr.tanh(x).e[0], (1 - math.tanh(2.0) ** 2) * 1e-3 + 2 * U * math.tanh(2.0) + rr.TINY)
    assert math.isclose(rr.sqrt(x).e[0], 1e-3 / (2 * math.sqrt(2.0)) + 2 * U * math.sqrt(2.0) + rr.TINY)
    assert rr.abs_(y).v[0] == 5.0 and rr.abs_(y).e[0] == 2e-3 and (-y).e[0] == 2e-3


def test_library_calls_of_numpy_fp32_sit_inside_the_bar():
    """numpy's vectorised fp32 exp / log / tanh are 1 .. 3 ulp routines, like the device library's: inside FACTOR x (2 u |z|)"""
    rng = np.random.RandomState(1)
    x = rng.uniform(-20, 20, 4096).astype(f32)
    inside(np.exp(x), rr.exp(x), "exp")
    inside(np.tanh(x), rr.tanh(x), "tanh")
    inside(np.log(np.abs(x) + f32(1e-3)), rr.log(np.abs(x) + f32(1e-3)), "log")
    assert inside(np.sqrt(np.abs(x)), rr.sqrt(np.abs(x)), "sqrt", 1.0) <= 1.0


def test_min_max_clip_where_round_nothing_and_keep_the_winners_bound():
    big, small = rr.exp(np.array([150.0, -150.0], f32)), BV.exact(100.0)
    m = rr.minimum(big, small)
    assert m.v[0] == 100.0 and m.e[0] == 0.0                 # the cap wins for sure: exact
    assert m.v[1] == math.exp(-150.0) and m.e[1] >= rr.TINY  # an fp32 exp underflows to 0 here: the absolute floor covers it
    x = BV(np.array([1.0, 1.0]), np.array([0.1, 0.1]))
    y = BV(np.array([1.05, 9.0]), np.array([0.3, 0.3]))
    m = rr.minimum(x, y)
    assert m.v.tolist() == [1.0, 1.0] and m.e.tolist() == [0.3, 0.1]        # overlapping intervals: the larger bound; separated: the winner's
    assert rr.maximum(x, y).v.tolist() == [1.05, 9.0] and rr.maximum(x, y).e.tolist() == [0.3, 0.3]
    c = rr.clip(np.array([-6.0, -5.0, 0.5, 2.0, 7.0], f32), -5.0, 2.0)
    assert c.v.tolist() == [-5.0, -5.0, 0.5, 2.0, 2.0] and (c.e == 0).all()
    w = rr.where([True, False], x, y)
    assert w.v.tolist() == [1.0, 9.0] and w.e.tolist() == [0.1, 0.3]


def _strided_tree_sum_f32(x):
    """the device pattern: 256 threads add their strided elements, 64-lane shuffle tree, then the four wave sums left to right"""
    x = np.asarray(x, f32)
    acc = np.zeros(256, f32)
    for i in range(0, x.size, 256):
        part = x[i:i + 256]
        acc[:part.size] = acc[:part.size] + part
    w = acc.reshape(4, 64).copy()
    o = 32
    while o:
        w[:, :o] = w[:, :o] + w[:, o:2 * o]
        o //= 2
    return f32(f32(f32(w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0])


@pytest.mark.parametrize("n", [1, 31, 256, 257, 513, 3000])
def test_sum_bound_covers_the_strided_tree_and_the_sequential_sum(n):
    rng = np.random.RandomState(n)
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(f32)
    s = rr.sum_(x)
    assert s.v == x.astype(np.float64).sum()
    assert math.isclose(s.e, math.ceil(math.log2(n) + n / 256 + 2) * U * np.abs(x).astype(np.float64).sum(), rel_tol=1e-12)
    assert inside(_strided_tree_sum_f32(x), s, ("tree", n), 1.0) <= 1.0
    seq = f32(0)
    for v in x[:40]:
        seq = f32(seq + v)
    q = rr.sum_(x[:40], sequential=True)
    assert math.isclose(q.e, (min(n, 40) - 1) * U * np.abs(x[:40]).astype(np.float64).sum(), rel_tol=1e-12, abs_tol=0.0)
    assert inside(seq, q, ("seq", n), 1.0) <= 1.0
    m = rr.sum_(BV(np.ones((3, 4)), np.full((3, 4), 0.5)), axis=1)
    assert m.v.tolist() == [4.0] * 3 and np.allclose(m.e, 2.0 + rr.sum_terms(4) * U * 4.0)


def test_ill_conditioned_chain_widens_its_own_bound():
    """log(1 - a^2 + 1e-6) at saturation: evaluated in fp32 step by step it stays inside the propagated bound, which is orders of
    magnitude wider than one rounding of the result there and collapses to it away from saturation"""
    a = np.array([0.0, 0.5, 0.999, 1.0 - 2.0 ** -12, 1.0 - 2.0 ** -20, 1.0 - 2.0 ** -24, 1.0], f32)
    ref = rr.log((1.0 - BV.exact(a) * BV.exact(a)) + 1e-6)
    got = np.log((f32(1) - a * a) + f32(1e-6))
    assert inside(got, ref, "log1ma2") <= FACTOR
    rel = ref.e / np.maximum(np.abs(ref.v), 1e-30)
    assert rel[1] < 32 * U and rel[5] > 1e3 * U and (np.diff(ref.e[:6]) > 0).all()


def test_ratio_semantics():
    ref = BV(np.array([1.0, 2.0, 0.0]), np.array([0.5, 0.0, 0.0]))
    assert rr.ratio(np.array([1.25, 2.0, 0.0]), ref) == 0.5
    assert rr.ratio(np.array([1.0, 2.0 + 1e-9, 0.0]), ref) == np.inf          # an exact expectation admits nothing
    assert rr.ratio(np.array([np.nan, 2.0, 0.0]), ref) == np.inf
    with pytest.raises(AssertionError):
        rr.holds(np.array([4.0, 2.0, 0.0]), ref, "x")
    worst = {}
    rr.holds(np.array([2.0, 2.0, 0.0]), ref, ("k", 1), worst)
    assert worst == {"k": 2.0}


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatements against the numpy oracle
# ---------------------------------------------------------------------------------------------------------------------------------
def _head(cache):
    return np.concatenate([cache["mu"], cache["ls_raw"]], axis=1).astype(f32)


@pytest.mark.parametrize("A, scale", [(1, 1.0), (3, 1.0), (17, 1.0), (32, 4.0)])
def test_tanh_sample_and_head_backward_against_the_oracle(A, scale):
    rng = np.random.RandomState(A)
    od, B, hid = 5, 64, [16, 16]
    net = synth.make_tanh_actor(rng, od, A, hid)
    net["dist_net.sigma.bias"] = (net["dist_net.sigma.bias"] + rng.uniform(-7, 3, A) * scale).astype(f32)      # both clamps are reached
    net["dist_net.mu.bias"] = (net["dist_net.mu.bias"] + rng.standard_normal(A) * scale).astype(f32)
    net["dist_net.sigma.weight"] = (net["dist_net.sigma.weight"] * f32(30.0)).astype(f32)                     # ... by some rows of every column
    obs, eps = rng.standard_normal((B, od)).astype(f32), rng.standard_normal((B, A)).astype(f32)
    a, logp, cache = nn.tanh_gauss_fwd(net, obs, eps)
    head = _head(cache)
    ra, rlogp = rr.tanh_sample(head[:, :A], head[:, A:], eps, act=a)
    inside(a, ra, ("a", A))
    inside(logp.ravel(), rlogp, ("logp", A))
    da = (rng.standard_normal((B, A)) / B).astype(f32)
    alpha = f32(0.7)
    grads = nn.tanh_gauss_bwd(net, cache, da, np.full((B, 1), alpha / f32(B), f32))
    dh = rr.head_bwd(da, head, eps, a, alpha, B)
    gate = (head[:, A:] >= -5) & (head[:, A:] <= 2)
    assert gate.any() and (~gate).any() and (dh.v[:, A:][~gate] == 0).all() and (dh.e[:, A:][~gate] == 0).all()
    inside(grads["dist_net.mu.bias"], rr.sum_(dh[:, :A], axis=0), ("dmu", A))
    inside(grads["dist_net.sigma.bias"], rr.sum_(dh[:, A:], axis=0), ("dls", A))


def test_min_route_matches_min2_grad_and_splits_ties():
    rng = np.random.RandomState(3)
    B = 37
    q = rng.standard_normal((2, B)).astype(f32)
    q[1, ::5] = q[0, ::5]
    g1, g2 = nn.min2_grad(q[0], q[1], np.full(B, -1.0 / B, f32))
    qmin, dqa = rr.min_route(q, B)
    assert np.array_equal(qmin, np.minimum(q[0], q[1]))
    inside(np.stack([g1, g2]), dqa, "min2")
    assert (dqa.v[:, ::5] == dqa.v[0, 0]).all() and math.isclose(dqa.v[0, 0], -0.5 / B)
    q3 = rng.standard_normal((5, B)).astype(f32)
    q3[3, 1] = q3[0, 1] = q3[:, 1].min() - 1
    _, d3 = rr.min_route(q3, B)
    assert np.allclose(d3.v.sum(axis=0), -1.0 / B) and ((d3.v != 0) == (q3 == q3.min(axis=0))).all()


@pytest.mark.parametrize("t", [1, 2, 1000, 10 ** 6 + 1])
def test_adam_and_polyak_against_the_oracle(t):
    rng = np.random.RandomState(t % 97)
    n = 301
    p, g = rng.standard_normal(n).astype(f32), (rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 1, n)).astype(f32)
    m0 = (0.1 * rng.standard_normal(n)).astype(f32) if t > 1 else np.zeros(n, f32)
    v0 = (0.01 * rng.uniform(size=n)).astype(f32) if t > 1 else np.zeros(n, f32)
    tgt = rng.standard_normal(n).astype(f32)
    params = {"w": p.copy()}
    opt = dict(step=t - 1, m={"w": m0.copy()}, v={"w": v0.copy()})
    nn.adam_step(params, {"w": g}, opt, 3e-4)
    old = {"w": tgt.copy()}
    nn.polyak(old, params, 0.005)
    rp, rm, rv, rt = rr.adam(p, m0, v0, g, 3e-4, 0.9, 0.999, 1e-8, t, tau=0.005, target=tgt, torch_scalars=True)
    inside(params["w"], rp, ("p", t)); inside(opt["m"]["w"], rm, ("m", t)); inside(opt["v"]["w"], rv, ("v", t)); inside(old["w"], rt, ("target", t))
    assert (rp.e < 1e-6).all()
    # the engine's Adam (fp32 hyper-parameters, 1 - beta exact for them) against torch's scalars: 1.3e-5 apart in exp_avg_sq, no more
    ep, em, ev = rr.adam(p, m0, v0, g, 3e-4, 0.9, 0.999, 1e-8, t)
    assert np.abs(ev.v - rv.v).max() <= 1.4e-5 * np.abs(rv.v).max() and np.abs(em.v - rm.v).max() <= 3e-7 * np.abs(rm.v).max() + 3e-8 * np.abs(g).max()
    assert np.abs(ep.v - rp.v).max() <= 1e-5 * 3e-4 * 40


def _raw(net, obs, wkey, bkey):
    Ws, bs = nn.backbone_layers(net)
    hs = nn.mlp_fwd(obs, Ws, bs)
    return (nn.mm(hs[-1], net[wkey].T) + net[bkey]).astype(f32)


@pytest.mark.parametrize("case", ["cql_tiny", "cql_tiny_lagrange", "cql_tiny_maxq", "cql_tiny_stoch_fixed_alpha"])
def test_cql_restatements_against_the_oracle(case):
    from helpers import cql_oracle_setup
    cfg, st, batches, noises = cql_oracle_setup(case)
    b, n = batches[0], noises[0]
    obs, act, nobs = b["observations"], b["actions"], b["next_observations"]
    B, A, N = obs.shape[0], act.shape[1], cfg["num_repeat_actions"]
    BN = B * N
    pre = clone_state({k: st[k] for k in ("actor", "critic1", "critic2", "critic1_old", "critic2_old")})
    la0, cla0 = float(st["log_alpha"][0]), float(st["cql_log_alpha"][0])
    alpha0 = ocql.current_alpha(st, cfg)
    res, aux = ocql.learn(st, cfg, b, n)
    # actor phase
    qa = np.stack([aux["q1a"].ravel(), aux["q2a"].ravel()])
    loss, _ = rr.actor_loss(qa, aux["logp"].ravel(), alpha0, B)
    inside(res["loss/actor"], loss, "loss/actor")
    if cfg["auto_alpha"]:
        al, p, m, v, na = rr.alpha_step(aux["logp"].ravel(), f32(la0), 0.0, 0.0, cfg["target_entropy"], cfg["alpha_lr"], 0.9, 0.999, 1e-8, 1, B, False)
        inside(res["loss/alpha"], al, "loss/alpha"); inside(st["log_alpha"][0], p, "log_alpha"); inside(res["alpha"], na, "alpha")
    alpha1 = ocql.current_alpha(st, cfg)
    # targets with the updated actor, the old critics
    rep = N if cfg["max_q_backup"] else 1
    tn = np.repeat(nobs, rep, axis=0)
    na_, nlogp, _ = nn.tanh_gauss_fwd(st["actor"], tn, n["eps_next"])
    qt = np.stack([nn.critic_fwd(pre[k], tn, na_)[0].ravel() for k in ("critic1_old", "critic2_old")])
    stoch = not cfg["max_q_backup"] and not cfg["deterministic_backup"]
    y = rr.td_target(qt, b["rewards"].ravel(), b["terminals"].ravel(), cfg["gamma"], rep, nlogp.ravel() if stoch else None, alpha1)
    inside(aux["target_q"].ravel(), y, "target_q")
    # conservative loss
    to = np.repeat(obs, N, axis=0)
    a_pi, lp_pi, _ = nn.tanh_gauss_fwd(st["actor"], to, n["eps_pi"])
    a_npi, lp_npi, _ = nn.tanh_gauss_fwd(st["actor"], np.repeat(nobs, N, axis=0), n["eps_next_pi"])
    e, cs, gate = rr.cql_alpha(f32(cla0))
    raws = []
    for ci, nm in enumerate(("critic1", "critic2")):
        q_all = np.concatenate([nn.critic_fwd(pre[nm], obs, act)[0].ravel()] + [nn.critic_fwd(pre[nm], to, x)[0].ravel() for x in (a_pi, a_npi, n["u_rand"])])
        assert np.array_equal(q_all[:B], aux[f"q{ci + 1}"].ravel())
        loss, raw, dq = rr.cql_loss(q_all, aux["target_q"].ravel(), lp_pi.ravel(), lp_npi.ravel(), B, BN, A, B, cfg["cql_weight"], cfg["temperature"],
                                    cfg["lagrange_threshold"], cs if cfg["with_lagrange"] else 1.0, cfg["with_lagrange"])
        raws.append(raw)
        inside(res[f"loss/critic{ci + 1}"], loss, ("loss", nm))
        inside(aux[f"{nm}_grads"]["last.bias"], rr.sum_(dq), ("sum dq", nm))
    if cfg["with_lagrange"]:
        l, cs_, p, m, v = rr.lagrange_step(raws[0], raws[1], f32(cla0), 0.0, 0.0, cfg["cql_alpha_lr"], 0.9, 0.999, 1e-8, 1)
        inside(res["loss/cql_alpha"], l, "loss/cql_alpha"); inside(res["cql_alpha"], cs_, "cql_alpha"); inside(st["cql_log_alpha"][0], p, "cql_log_alpha")


@pytest.mark.parametrize("cla", [20.0, -20.0])
def test_lagrange_clamp_gates_the_gradient(cla):
    e, cs, gate = rr.cql_alpha(f32(cla))
    raw = BV(np.array(3.0), np.array(1e-6))
    l, cs_, p, m, v = rr.lagrange_step(raw, raw, f32(cla), 0.0, 0.0, 3e-4, 0.9, 0.999, 1e-8, 1)
    if cla > 0:
        assert cs.v == 1e6 and cs.e == 0 and not gate and p.v == cla and m.v == 0 and v.v == 0
    else:
        assert gate and math.isclose(cs.v, math.exp(-20.0)) and p.v != cla


@pytest.mark.parametrize("case", ["iql_tiny", "iql_tiny_h3"])
def test_iql_restatements_against_the_oracle(case):
    from helpers import generic_oracle_setup
    mod, cfg, st, batches, _ = generic_oracle_setup("iql", case)
    b = batches[0]
    obs, act, nobs = b["observations"], b["actions"], b["next_observations"]
    B, A = act.shape
    pre = clone_state({k: st[k] for k in ("actor",)})
    res, aux = oiql.learn(st, cfg, b, None)
    # (the oracle keeps min(q_old); the routing of a min over two exact operands is exact either way)
    qo = np.stack([aux["q_old"].ravel(), aux["q_old"].ravel()])
    L, dv, qm = rr.iql_v_loss(qo, aux["v"].ravel(), B, cfg["expectile"])
    inside(res["loss/v"], L, "loss/v")
    inside(aux["critic_v_grads"]["last.bias"], rr.sum_(dv), "sum dv")
    v2 = np.concatenate([nn.critic_fwd(st["critic_v"], obs)[0].ravel(), nn.critic_fwd(st["critic_v"], nobs)[0].ravel()])
    y, ea = rr.iql_q_loss(v2, qm, b["rewards"].ravel(), b["terminals"].ravel(), B, cfg["gamma"], cfg["temperature"])
    inside(aux["target_q"].ravel(), y, "target_q"); inside(aux["exp_a"].ravel(), ea, "exp_a")
    Lq, dq = rr.td_loss(np.stack([aux["q1"].ravel(), aux["q2"].ravel()]), aux["target_q"].ravel(), B)
    inside([res["loss/q1"], res["loss/q2"]], Lq, "loss/q")
    inside(aux["critic_q1_grads"]["last.bias"], rr.sum_(dq[0]), "sum dq1")
    mraw = _raw(pre["actor"], obs, "dist_net.mu.weight", "dist_net.mu.bias")
    La, dm, gs = rr.iql_actor_loss(mraw, act, aux["exp_a"].ravel(), pre["actor"]["dist_net.sigma_param"], B)
    inside(res["loss/actor"], La, "loss/actor")
    inside(aux["actor_grads"]["dist_net.mu.bias"], rr.sum_(dm, axis=0), "sum dmraw")
    inside(aux["actor_grads"]["dist_net.sigma_param"].ravel(), gs, "g_sigma")


def test_td3bc_restatements_against_the_oracle():
    from helpers import generic_oracle_setup
    mod, cfg, st, batches, noises = generic_oracle_setup("td3bc", "td3bc_tiny")
    b, n = batches[0], noises[0]
    obs, act, nobs = b["observations"], b["actions"], b["next_observations"]
    B, A = act.shape
    pre = clone_state({k: st[k] for k in ("actor", "actor_old", "critic1_old", "critic2_old")})
    res, aux = otd3.learn(st, cfg, b, n)
    mraw_t = _raw(pre["actor_old"], nobs, "last.weight", "last.bias")
    na = rr.det_action(mraw_t, cfg["max_action"], n["eps_target"] * f32(4.0), cfg["policy_noise"], cfg["noise_clip"])       # x 4: the clip is reached
    assert (np.abs(na.v - np.tanh(mraw_t.astype(np.float64))) >= 0.5 - 1e-6).any()
    na = rr.det_action(mraw_t, cfg["max_action"], n["eps_target"], cfg["policy_noise"], cfg["noise_clip"])
    ora_na = np.clip(otd3.det_actor_fwd(pre["actor_old"], nobs, cfg["max_action"])[0]
                     + np.clip(n["eps_target"] * f32(cfg["policy_noise"]), -f32(cfg["noise_clip"]), f32(cfg["noise_clip"])), -1, 1).astype(f32)
    inside(ora_na, na, "a_next")
    qt = np.stack([nn.critic_fwd(pre[k], nobs, ora_na)[0].ravel() for k in ("critic1_old", "critic2_old")])
    inside(aux["target_q"].ravel(), rr.td_target(qt, b["rewards"].ravel(), b["terminals"].ravel(), cfg["gamma"]), "target_q")
    L, dq = rr.td_loss(np.stack([aux["q1"].ravel(), aux["q2"].ravel()]), aux["target_q"].ravel(), B)
    inside([res["loss/critic1"], res["loss/critic2"]], L, "loss/critic")
    inside(aux["critic2_grads"]["last.bias"], rr.sum_(dq[1]), "sum dq2")
    mraw = _raw(pre["actor"], obs, "last.weight", "last.bias")
    a_pi = rr.det_action(mraw, cfg["max_action"])
    a32 = otd3.det_actor_fwd(pre["actor"], obs, cfg["max_action"])[0]
    inside(a32, a_pi, "a_pi")
    La, dqpi = rr.td3_actor_loss(aux["q_pi"].ravel(), a32, act, cfg["alpha"], B, A)
    inside(res["loss/actor"], La, "loss/actor")
    # dQ/da of the oracle: from the actor's bias gradient it is not separable; check the BC part with dQ/da = 0 against the closed form
    dm = rr.td3_actor_bwd(np.zeros_like(a32), a32, act, cfg["max_action"], B, A)
    t = a32 / f32(cfg["max_action"])
    inside((f32(2) * (a32 - act) / f32(B * A) * f32(cfg["max_action"]) * (f32(1) - t * t)).astype(f32), dm, "dmraw bc")


@pytest.mark.parametrize("case", ["edac_tiny_eta0_det", "edac_tiny_maxq", "edac_tiny"])
def test_edac_restatements_against_the_oracle(case):
    from helpers import generic_oracle_setup
    mod, cfg, st, batches, noises = generic_oracle_setup("edac", case)
    b, n = batches[0], noises[0]
    obs, act, nobs = b["observations"], b["actions"], b["next_observations"]
    B, A = act.shape
    K = cfg["num_critics"]
    pre = clone_state({k: st[k] for k in ("actor", "critics_old")})
    alpha0 = f32(np.exp(st["log_alpha"][0]))
    res, aux = oedac.learn(st, cfg, b, n)
    _, logp, _ = nn.tanh_gauss_fwd(pre["actor"], obs, n["eps_actor"])
    qas = aux["qas"].reshape(K, B)
    loss, dqa = rr.actor_loss(qas, logp.ravel(), alpha0, B)
    inside(res["loss/actor"], loss, "loss/actor")
    assert np.allclose(dqa.v.sum(axis=0), -1.0 / B)
    al, p, m, v, na = rr.alpha_step(logp.ravel(), st["log_alpha"][0] * 0 + f32(-0.3), 0.0, 0.0, cfg["target_entropy"], cfg["alpha_lr"], 0.9, 0.999, 1e-8, 1, B, True)
    inside(res["loss/alpha"], al, "loss/alpha"); inside(res["alpha"], na, "alpha")
    rep = 10 if cfg["max_q_backup"] else 1
    tn = np.repeat(nobs, rep, axis=0)
    na_, nlogp, _ = nn.tanh_gauss_fwd(st["actor"], tn, n["eps_next"])
    qt = oedac.ens_fwd(pre["critics_old"], np.concatenate([tn, na_], axis=1))[0].reshape(K, B * rep)
    stoch = not cfg["max_q_backup"] and not cfg["deterministic_backup"]
    y = rr.td_target(qt, b["rewards"].ravel(), b["terminals"].ravel(), cfg["gamma"], rep, nlogp.ravel() if stoch else None, f32(res["alpha"]))
    inside(aux["target_q"].ravel(), y, "target_q")
    L, dq = rr.td_loss(aux["qs"].reshape(K, B), aux["target_q"].ravel(), B)
    if cfg["eta"] == 0:
        inside(res["loss/critics"], rr.sum_(L, sequential=True), "loss/critics")
    inside(aux["critics_grads"][f"model.{2 * len(cfg['hidden'])}.bias"].ravel(), rr.sum_(dq, axis=1), "sum dq")


def test_structural_errors_are_orders_of_magnitude_beyond_the_bar():
    """what the GPU module exists to catch, emulated in fp32: a dropped second trip of the 256-thread loop, a lane group that is too
    narrow, a gate that is off by one float, a tie that is not split"""
    rng = np.random.RandomState(9)
    B, A = 300, 17
    logp, qa = rng.standard_normal(B).astype(f32), rng.standard_normal((2, B)).astype(f32)
    loss, dqa = rr.actor_loss(qa, logp, f32(0.7), B)
    terms = f32(0.7) * logp - qa.min(axis=0)
    assert rr.ratio(terms.sum(dtype=f32) / f32(B), loss) <= FACTOR
    assert rr.ratio(terms[:256].sum(dtype=f32) / f32(B), loss) > 1e4                       # rows 256 .. 299 never added
    head = np.concatenate([rng.standard_normal((B, A)), rng.uniform(-4, 1, (B, A))], axis=1).astype(f32)
    eps = rng.standard_normal((B, A)).astype(f32)
    ls = head[:, A:]
    u = head[:, :A] + np.exp(ls) * eps
    a = np.tanh(u)
    term = (-((u - head[:, :A]) ** 2) / (f32(2) * np.exp(ls) ** 2) - ls - f32(rr.LOG_SQRT_2PI)) - np.log((f32(1) - a * a) + f32(1e-6))
    _, rl = rr.tanh_sample(head[:, :A], ls, eps, act=a)
    assert rr.ratio(term.sum(axis=1, dtype=f32), rl) <= FACTOR
    assert rr.ratio(term[:, :16].sum(axis=1, dtype=f32), rl) > 1e4                         # a 16-lane group for 17 actions
    head[0, A] = np.nextafter(f32(2), f32(9))
    dh = rr.head_bwd(rng.standard_normal((B, A)).astype(f32) / B, head, eps, a, f32(0.7), B)
    open_gate = rr.head_bwd(rng.standard_normal((B, A)).astype(f32) / B, np.where(head > 2, f32(2), head), eps, a, f32(0.7), B)
    assert dh.v[0, A] == 0 and dh.e[0, A] == 0 and open_gate.v[0, A] != 0 and rr.ratio(open_gate.v[0, A], dh[0, A]) == np.inf
    q = qa.copy()
    q[1, 0] = q[0, 0]
    _, d = rr.min_route(q, B)
    assert rr.ratio(f32(-1.0) / f32(B), d[0, 0]) > 1e4                                       # the whole seed on one of two tied critics
