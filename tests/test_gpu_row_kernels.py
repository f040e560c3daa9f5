"""GPU: the row kernels of csrc/kernels.h -- k_tanh_sample, k_actor_loss, k_head_bwd, k_cql_loss_rows, k_td_loss, k_iql_v_loss,
k_iql_q_loss, k_iql_actor_loss, k_det_action, k_td3_actor_loss, k_td3_actor_bwd, k_adam (with its fused Polyak sync) -- each against a
float64 restatement of the same operation ON THE ENGINE'S OWN OPERANDS, read back through ``debug_read`` after a real step, so that the
engine's own launch geometry and branch selection are what is tested.

Bar, for EVERY element of every result and for every metric:  |got - f64| <= 4 x (the first-order fp32 error bound that the restatement
propagates through its own arithmetic, tests/row_refs.py; proven against the numpy oracle in tests/test_row_refs_cpu.py).  The factor 4
is derived there, not measured.  A wrong lane group, a dropped trip of a strided loop, a mis-indexed row or a wrong gate is off by orders
of magnitude; rounding is not.

Shapes move one edge at a time from B = 32, A = 3, obs_dim = 5, one run, hidden [32, 32] (every launch then takes the tiled kernels and
the separate row kernels): B 1 .. 513 (second and third trip of the 256-thread loops, 1 .. 3 workgroups of k_cql_loss_rows and
k_head_bwd, the split-precision branch without a head scale above 256 rows), A 1 .. 32 (the 8-, 16- and 32-lane groups of
k_tanh_sample), obs_dim 1 / 5 / 31 (critic-input pitches), 3 runs with different nets and data per run, both precisions, max-Q and
stochastic backups, the Lagrange variant.  Hidden [256, 256] cases assert from the profile which launches ran: the fused actor phase
(no k_actor_loss / k_head_bwd launch; its loss, metrics and temperature step are held to the same restatements), B = 2080, where
k_head_bwd weighs unit-seed critic gradients with dqa itself, the same shape with ORL_FUSE_SMALL=0 / ORL_SMALL_FWD=0, and A = 9 (beyond what the few-rows
launches of the actor phase admit).  Value edges at B = 64, A = 17: a constant-head actor whose biases put the log-std on, next to and far
beyond both clamps and mu up to +-20 (saturated actions), tied critics, all-terminal / no-terminal batches, rewards of 1e3, IQL
advantages that reach the cap of 100 or underflow, TD3+BC noise beyond the clip and actions beyond max_action, a Lagrange multiplier
beyond its clamp.  Optimizer: k_adam and the Polyak sync on the engine's own summed gradient with non-zero moments at
t = 1, 2, 1000, 10^6 + 1 (TD3+BC with update_actor_freq = 3: the actor's own step count), batches small enough that every tensor has
at most two gradient slabs (their fp32 sum is then the rounded exact sum that ``debug_grads`` returns).

Measured worst |err| / bound over the whole module (MI355X; the bar is 4, a correct kernel is expected below 1; the module prints them):
    k_tanh_sample      action 0.68, logp 0.29
    k_actor_loss       loss 0.14, dqa 0.50, alpha loss 0.19, log_alpha 0.73 (moments 0.16 / 0.25), alpha 0.20
    k_head_bwd         dhead 0.73; on unit-seed gradients weighed with dqa (B = 2080) 0.57
    fused actor phase  (small_abwd) loss 0.15, alpha loss 0.13, log_alpha 0.73 (moments 0.16 / 0.16), alpha 0.19
    k_cql_loss_rows    target_q 0.86, loss 0.10, dq 0.57, cql_alpha 0.28, its loss 0.06, cql_log_alpha 0.38 (moments 0.03 / 0.04)
    k_td_loss          target_q 0.90, loss 0.23, dq 0.65
    k_iql_v_loss       loss 0.13, dv 0.45
    k_iql_q_loss       target_q 0.85, loss 0.21, dq 0.65, exp_a 0.60
    k_iql_actor_loss   loss 0.11, dmraw 0.51, g_sigma 0.13
    k_det_action       actor 0.35, target 1.00 (0.9961)
    k_td3_actor_loss   loss 0.07, dq 0.17
    k_td3_actor_bwd    dmraw 0.53
    k_adam             parameter 0.99, exp_avg 0.94, exp_avg_sq 0.76, Polyak target 0.66
Every figure sits below 1, i.e. inside the first-order bound itself, a factor 4 inside the bar.

Not covered here, with the reason: k_polyak (no schedule launches it: every Polyak sync rides in k_adam, which is covered);
k_adam's sum over more than two gradient slabs (the slabs cannot be read back one by one; their fp32 sum differs from the rounded
exact sum by an amount the summed gradient does not bound)."""
import numpy as np
import pytest

import row_refs as rr
import synth
import test_gpu_algos as ta
import test_gpu_cql as tc

pytestmark = pytest.mark.gpu
f32 = np.float32

WORST = {}            # kernel.result -> worst |err| / bound seen by this module


@pytest.fixture(scope="module", autouse=True)
def _figures():
    yield
    print("\nworst |got - f64| / bound per row-kernel result:", {k: round(v, 4) for k, v in sorted(WORST.items())})


def holds(got, ref, key, tag):
    return rr.holds(got, ref, (key,) + tuple(tag), WORST, key)


# ---------------------------------------------------------------------------------------------------------------------------------
# engines at ad-hoc shapes
# ---------------------------------------------------------------------------------------------------------------------------------
NETS = {"cql": tc.NETS, **ta.NET_IDS, "mcq": dict(tc.NETS, vae_enc=7, vae_dec=8)}


class Ctx:
    pass


def _state(algo, rng, od, A, hid, K, Z=None, vae_hidden=None):
    st = {}
    if algo in ("cql", "mcq"):
        st["actor"] = synth.make_tanh_actor(rng, od, A, hid)
        st["critic1"], st["critic2"] = synth.make_critic(rng, od + A, hid), synth.make_critic(rng, od + A, hid)
        st["critic1_old"], st["critic2_old"] = synth._perturbed(rng, st["critic1"]), synth._perturbed(rng, st["critic2"])
        if algo == "mcq":        # one state_dict (e1, e2, mean, log_std | d1, d2, d3): the engine's encoder and decoder nets each take their tensors
            st["vae_enc"] = st["vae_dec"] = st["behavior_policy"] = synth.make_vae(rng, od, A, vae_hidden, Z)
    elif algo == "edac":
        st["actor"] = synth.make_tanh_actor(rng, od, A, hid)
        c = ta._strip_saved(synth.make_ensemble_critic(rng, od + A, hid, K))
        last = f"model.{2 * len(hid)}.weight"
        c[last] = synth._uniform(rng, c[last].shape, 0.1)
        st["critics"], st["critics_old"] = c, synth._perturbed(rng, c)
    elif algo == "iql":
        st["actor"] = synth.make_gauss_actor(rng, od, A, hid)
        st["critic_q1"], st["critic_q2"] = synth.make_critic(rng, od + A, hid), synth.make_critic(rng, od + A, hid)
        st["critic_v"] = synth.make_critic(rng, od, hid)
        st["critic_q1_old"], st["critic_q2_old"] = synth._perturbed(rng, st["critic_q1"]), synth._perturbed(rng, st["critic_q2"])
    else:
        st["actor"] = synth.make_det_actor(rng, od, A, hid)
        st["critic1"], st["critic2"] = synth.make_critic(rng, od + A, hid), synth.make_critic(rng, od + A, hid)
        st["actor_old"] = synth._perturbed(rng, st["actor"])
        st["critic1_old"], st["critic2_old"] = synth._perturbed(rng, st["critic1"]), synth._perturbed(rng, st["critic2"])
    return st


def inputs(algo, B=32, A=3, od=5, R=1, hidden=(32, 32), seed=0, N=2, K=4, Z=6, vae_hidden=24, mutate=None, **over):
    """nets, batch and noise of every run of a case (host arrays only: the CPU tests run the oracle on the same inputs)"""
    c = Ctx()
    c.algo, c.B, c.A, c.od, c.R, c.N, c.K, c.hidden = algo, B, A, od, R, N, (K if algo == "edac" else 2), list(hidden)
    c.Z, c.vae_hidden = Z, vae_hidden
    c.XP = (od + A + 3) // 4 * 4
    c.maxq = bool(over.get("max_q_backup", 0))
    c.rep = (N if algo == "cql" else 10) if c.maxq else 1
    c.sts, c.batches, c.noises = [], [], []
    for r in range(R):
        rng = np.random.RandomState(7919 * seed + 31 * r + B + 64 * A)
        c.sts.append(_state(algo, rng, od, A, c.hidden, K, Z, vae_hidden))
        c.batches.append(synth.make_batch(rng, B, od, A))
        if algo == "cql":
            c.noises.append(synth.make_cql_noise(rng, B, N, A, max_q_backup=c.maxq))
        elif algo == "edac":
            c.noises.append(synth.make_sac_noise(rng, B, A, rows_next=B * c.rep))
        elif algo == "td3bc":
            c.noises.append(synth.make_td3_noise(rng, B, A))
        elif algo == "mcq":      # the reference's draw order (oracle/mcq.py)
            c.noises.append({k: rng.standard_normal(s).astype(f32) for k, s in (("eps_vae", (B, Z)), ("eps_next", (B, A)), ("z_ood", (2 * B * N, Z)),
                                                                                ("eps_ood", (2 * B, A)), ("eps_actor", (B, A)))})
        else:
            c.noises.append({})
    if mutate:
        mutate(c)
    return c


def make(algo, B=32, A=3, od=5, R=1, precision=0, hidden=(32, 32), seed=0, N=2, K=4, env=None, monkeypatch=None, mutate=None,
         log_alpha=-0.3, cql_log_alpha=0.2, Z=6, vae_hidden=24, **over):
    from offlinerlkit import _engine
    c = inputs(algo, B=B, A=A, od=od, R=R, hidden=hidden, seed=seed, N=N, K=K, Z=Z, vae_hidden=vae_hidden, mutate=mutate, **over)
    cfg = dict(obs_dim=od, act_dim=A, hidden=c.hidden, batch_size=B, n_runs=R, precision=precision)
    if algo == "cql":
        cfg.update(num_repeat_actions=N, target_entropy=-float(A))
    elif algo == "edac":
        cfg.update(num_critics=K, eta=0.0, target_entropy=-float(A))
    elif algo == "mcq":
        cfg.update(num_repeat_actions=N, vae_latent=Z, vae_hidden=vae_hidden, target_entropy=-float(A))
    cfg.update(over)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    try:
        c.eng = _engine.Engine(_engine.default_config(algo, **cfg))      # (a shape the config check admits must build: a refusal is a finding)
    finally:
        for k in (env or {}):
            monkeypatch.delenv(k, raising=False)
    c.cfg = c.eng.cfg
    for r in range(R):
        for nm, nid in NETS[algo].items():
            c.eng.set_net(r, nid, c.sts[r][nm])
        if algo in ("cql", "edac", "mcq"):
            c.eng.set_scalar(r, _engine.SCALAR_LOG_ALPHA, log_alpha)
        if algo == "cql":
            c.eng.set_scalar(r, _engine.SCALAR_CQL_LOG_ALPHA, cql_log_alpha)
    c.eng.profile_enable(True)
    return c


NOISE_KEYS = {"cql": ("eps_actor", "eps_next", "u_rand", "eps_pi", "eps_next_pi"), "edac": ("eps_actor", "eps_next"), "td3bc": ("eps_target",), "iql": (),
              "mcq": ("eps_vae", "eps_next", "z_ood", "eps_ood", "eps_actor")}
SC = ("LOG_ALPHA", "LOG_ALPHA_M", "LOG_ALPHA_V", "CQL_LOG_ALPHA", "CQL_LOG_ALPHA_M", "CQL_LOG_ALPHA_V", "ALPHA", "LAST_ACTOR_LOSS")


def scalars(c, r):
    from offlinerlkit import _engine
    return {k: c.eng.get_scalar(r, getattr(_engine, "SCALAR_" + k)) for k in SC}


def step(c):
    """one step on the case's inputs; returns (metrics [R][nm], the scalars of every run before the step, the step count before it)"""
    pre = [scalars(c, r) for r in range(c.R)]
    t0 = c.eng.step_count()
    batch = {k: np.stack([b[k] for b in c.batches]) for k in c.batches[0]}
    noise = [np.stack([n[k] for n in c.noises]) for k in NOISE_KEYS[c.algo]]
    return c.eng.step(batch, noise), pre, t0


def launched(c):
    return {row["name"] for row in c.eng.profile_table()}


def metric(c, m, r, name):
    return m[r][c.eng.metric_names.index(name)]


# ---------------------------------------------------------------------------------------------------------------------------------
# the checks, one per schedule phase; T(name) reads a tap of run r
# ---------------------------------------------------------------------------------------------------------------------------------
def check_sample(c, head, rows, eps, act, logp, tag):
    A = c.A
    assert np.isfinite(act).all() and np.isfinite(logp).all(), tag
    ra, rl = rr.tanh_sample(head[rows, :A], head[rows, A:], eps, act=act)
    holds(act, ra, "tanh_sample.action", tag)
    holds(logp, rl, "tanh_sample.logp", tag)


def check_sac_actor(c, r, m, pre, t0, fused, tag):
    from offlinerlkit import _engine
    B, A, od, K, cfg = c.B, c.A, c.od, c.K, c.cfg
    T = lambda name: c.eng.debug_read(r, name)
    head, logp = T("head").reshape(B, 2 * A), T("logp_a")
    xa = T("xa").reshape(B, c.XP)[:, od:od + A]
    eps = c.noises[r]["eps_actor"]
    check_sample(c, head, np.arange(B), eps, xa, logp, tag + ("actor",))
    # fused == True: the one-launch actor backward (small_abwd) computed the loss, the metrics and the temperature step from the same
    # operands -- held to the same restatement under its own name; it stores neither dqa nor dhead
    # fused == "unit_seed": the one-launch critic pass left UNIT-seed gradients dQ_c / da in dxa, k_actor_loss and k_head_bwd are
    # their own launches and k_head_bwd weighs the gradients with the stored dqa itself
    k = "small_abwd" if fused is True else "actor_loss"
    alpha0 = pre["ALPHA"] if cfg.auto_alpha else cfg.alpha
    qa = np.stack([T("q1a"), T("q2a")]) if c.algo == "cql" else T("qas").reshape(K, B)
    loss, dqa = rr.actor_loss(qa, logp, alpha0, B)
    holds(metric(c, m, r, "loss/actor"), loss, k + ".loss", tag)
    if fused is not True:
        dqa_got = T("dqa").reshape(K, B)
        holds(dqa_got, dqa, "actor_loss.dqa", tag)
    if cfg.auto_alpha:
        al, p, am, av, na = rr.alpha_step(logp, f32(pre["LOG_ALPHA"]), f32(pre["LOG_ALPHA_M"]), f32(pre["LOG_ALPHA_V"]), cfg.target_entropy, cfg.alpha_lr,
                                          cfg.adam_beta1, cfg.adam_beta2, cfg.adam_eps, t0 + 1, B, c.algo == "edac")
        post = scalars(c, r)
        holds(metric(c, m, r, "loss/alpha"), al, k + ".alpha_loss", tag)
        holds(metric(c, m, r, "alpha"), na, k + ".alpha", tag)
        holds(post["LOG_ALPHA"], p, k + ".log_alpha", tag)
        holds(post["LOG_ALPHA_M"], am, k + ".log_alpha_m", tag)
        holds(post["LOG_ALPHA_V"], av, k + ".log_alpha_v", tag)
        holds(post["ALPHA"], na, k + ".alpha", tag)
    if fused is True:
        return
    da = rr.action_grad(T("dxa").reshape(K, B, A), dqa_got if fused == "unit_seed" else None)
    dh = rr.head_bwd(da, head, eps, xa, alpha0, B)
    got = T("dhead").reshape(B, 2 * A)
    assert np.isfinite(got).all(), tag
    holds(got, dh, "head_bwd.dhead_unit_seed" if fused == "unit_seed" else "head_bwd.dhead", tag)


def check_cql_critics(c, r, m, pre, t0, tag):
    B, A, od, N, cfg = c.B, c.A, c.od, c.N, c.cfg
    T = lambda name: c.eng.debug_read(r, name)
    BN, Bt, rep = B * N, B * c.rep, c.rep
    Mc = B + 3 * BN
    n, b = c.noises[r], c.batches[r]
    head2 = T("head2").reshape(2 * B, 2 * A)
    xt = T("xt").reshape(Bt, c.XP)[:, od:od + A]
    xc = T("xc").reshape(Mc, c.XP)[:, od:od + A]
    lpn, lpp, lpnp = T("logp_next"), T("logp_pi"), T("logp_npi")
    check_sample(c, head2, B + np.arange(Bt) // rep, n["eps_next"], xt, lpn, tag + ("next",))
    check_sample(c, head2, np.arange(BN) // N, n["eps_pi"], xc[B:B + BN], lpp, tag + ("pi",))
    check_sample(c, head2, B + np.arange(BN) // N, n["eps_next_pi"], xc[B + BN:B + 2 * BN], lpnp, tag + ("next_pi",))
    assert np.array_equal(xc[:B], b["actions"]) and np.array_equal(xc[B + 2 * BN:], n["u_rand"]), tag
    post = scalars(c, r)
    alpha1 = post["ALPHA"] if cfg.auto_alpha else cfg.alpha
    stoch = not cfg.max_q_backup and not cfg.deterministic_backup
    y = rr.td_target(np.stack([T("qt1"), T("qt2")]), b["rewards"].ravel(), b["terminals"].ravel(), cfg.gamma, rep, lpn if stoch else None, alpha1)
    tq = T("target_q")
    holds(tq, y, "cql_loss.target_q", tag)
    cs = rr.cql_alpha(f32(pre["CQL_LOG_ALPHA"]))[1] if cfg.with_lagrange else 1.0
    raws = []
    for ci in (1, 2):
        loss, raw, dq = rr.cql_loss(T(f"q{ci}_all"), tq, lpp, lpnp, B, BN, A, B, cfg.cql_weight, cfg.temperature, cfg.lagrange_threshold, cs, bool(cfg.with_lagrange))
        raws.append(raw)
        holds(metric(c, m, r, f"loss/critic{ci}"), loss, "cql_loss.loss", tag + (ci,))
        holds(T(f"dq{ci}"), dq, "cql_loss.dq", tag + (ci,))
    if cfg.with_lagrange:
        l, cs_, p, lm, lv = rr.lagrange_step(raws[0], raws[1], f32(pre["CQL_LOG_ALPHA"]), f32(pre["CQL_LOG_ALPHA_M"]), f32(pre["CQL_LOG_ALPHA_V"]),
                                             cfg.cql_alpha_lr, cfg.adam_beta1, cfg.adam_beta2, cfg.adam_eps, t0 + 1)
        holds(metric(c, m, r, "loss/cql_alpha"), l, "cql_loss.cql_alpha_loss", tag)
        holds(metric(c, m, r, "cql_alpha"), cs_, "cql_loss.cql_alpha", tag)
        holds(post["CQL_LOG_ALPHA"], p, "cql_loss.cql_log_alpha", tag)
        holds(post["CQL_LOG_ALPHA_M"], lm, "cql_loss.cql_log_alpha_m", tag)
        holds(post["CQL_LOG_ALPHA_V"], lv, "cql_loss.cql_log_alpha_v", tag)


def check_edac_critics(c, r, m, pre, t0, tag):
    B, A, od, K, cfg, rep = c.B, c.A, c.od, c.K, c.cfg, c.rep
    T = lambda name: c.eng.debug_read(r, name)
    Bt = B * rep
    n, b = c.noises[r], c.batches[r]
    head2 = T("head2").reshape(B, 2 * A)
    xt = T("xt").reshape(Bt, c.XP)[:, od:od + A]
    lpn = T("logp_next")
    check_sample(c, head2, np.arange(Bt) // rep, n["eps_next"], xt, lpn, tag + ("next",))
    alpha1 = scalars(c, r)["ALPHA"] if cfg.auto_alpha else cfg.alpha
    use_alpha = not cfg.max_q_backup and not cfg.deterministic_backup
    y = rr.td_target(T("qts").reshape(K, Bt), b["rewards"].ravel(), b["terminals"].ravel(), cfg.gamma, rep, lpn if use_alpha else None, alpha1)
    tq = T("target_q")
    holds(tq, y, "td_loss.target_q", tag)
    L, dq = rr.td_loss(T("qs").reshape(K, B), tq, B)
    holds(T("dqs").reshape(K, B), dq, "td_loss.dq", tag)
    holds(metric(c, m, r, "loss/critics"), rr.sum_(L, sequential=True), "td_loss.loss", tag)      # (eta = 0: the TD part is the whole metric)


def check_iql(c, r, m, actor_before, tag):
    B, A, cfg = c.B, c.A, c.cfg
    T = lambda name: c.eng.debug_read(r, name)
    b = c.batches[r]
    L, dv, qm = rr.iql_v_loss(np.stack([T("qo1"), T("qo2")]), T("v"), B, cfg.expectile)
    holds(metric(c, m, r, "loss/v"), L, "iql_v_loss.loss", tag)
    holds(T("dv"), dv, "iql_v_loss.dv", tag)
    qmin = T("qmin")
    assert np.array_equal(qmin, qm), tag
    y, ea = rr.iql_q_loss(T("v2"), qmin, b["rewards"].ravel(), b["terminals"].ravel(), B, cfg.gamma, cfg.iql_temperature)
    tq, exp_a = T("target_q"), T("exp_a")
    assert np.isfinite(exp_a).all() and (exp_a <= 100.0).all() and (exp_a >= 0).all(), tag
    holds(tq, y, "iql_q_loss.target_q", tag)
    holds(exp_a, ea, "iql_q_loss.exp_a", tag)
    Lq, dq = rr.td_loss(np.stack([T("q1"), T("q2")]), tq, B)
    holds([metric(c, m, r, "loss/q1"), metric(c, m, r, "loss/q2")], Lq, "iql_q_loss.loss", tag)
    holds(np.stack([T("dq1"), T("dq2")]), dq, "iql_q_loss.dq", tag)
    La, dm, gs = rr.iql_actor_loss(T("mraw").reshape(B, A), b["actions"], exp_a, actor_before["dist_net.sigma_param"], B)
    holds(metric(c, m, r, "loss/actor"), La, "iql_actor_loss.loss", tag)
    holds(T("dmraw").reshape(B, A), dm, "iql_actor_loss.dmraw", tag)
    holds(c.eng.debug_grads(r, NETS["iql"]["actor"])["dist_net.sigma_param"].ravel(), gs, "iql_actor_loss.g_sigma", tag)


def check_td3bc(c, r, m, actor_step, last_loss, tag):
    B, A, od, cfg = c.B, c.A, c.od, c.cfg
    T = lambda name: c.eng.debug_read(r, name)
    b, n = c.batches[r], c.noises[r]
    xt = T("xt").reshape(B, c.XP)[:, od:od + A]
    assert (np.abs(xt) <= cfg.max_action).all(), tag
    holds(xt, rr.det_action(T("mraw_t").reshape(B, A), cfg.max_action, n["eps_target"], cfg.policy_noise, cfg.noise_clip), "det_action.target", tag)
    y = rr.td_target(np.stack([T("qt1"), T("qt2")]), b["rewards"].ravel(), b["terminals"].ravel(), cfg.gamma)
    tq = T("target_q")
    holds(tq, y, "td_loss.target_q", tag)
    L, dq = rr.td_loss(np.stack([T("q1"), T("q2")]), tq, B)
    holds([metric(c, m, r, "loss/critic1"), metric(c, m, r, "loss/critic2")], L, "td_loss.loss", tag)
    holds(np.stack([T("dq1"), T("dq2")]), dq, "td_loss.dq", tag)
    if not actor_step:
        assert metric(c, m, r, "loss/actor") == last_loss, (tag, "a critic-only step reports the last actor loss")
        return
    xa = T("xa").reshape(B, c.XP)[:, od:od + A]
    holds(xa, rr.det_action(T("mraw").reshape(B, A), cfg.max_action), "det_action.actor", tag)
    La, dqpi = rr.td3_actor_loss(T("q_pi"), xa, b["actions"], cfg.td3bc_alpha, B, A)
    holds(metric(c, m, r, "loss/actor"), La, "td3_actor_loss.loss", tag)
    holds(T("dqpi"), rr.BV(np.full(B, dqpi.v), np.full(B, dqpi.e)), "td3_actor_loss.dq", tag)
    holds(T("dmraw").reshape(B, A), rr.td3_actor_bwd(T("dxa").reshape(B, A), xa, b["actions"], cfg.max_action, B, A), "td3_actor_bwd.dmraw", tag)


SEPARATE = {"tanh_sample", "actor_loss", "head_bwd"}
FUSED = {"actor.bwd_fused", "critic_a.qgrad"}


def run_case(algo, fused=False, expect=None, absent=None, **kw):
    """build, step once (TD3+BC: an actor step, then a critic-only step), check every run; returns the case for further assertions"""
    c = make(algo, **kw)
    try:
        tag = (algo, c.B, c.A, c.od, c.R, kw.get("precision", 0))
        actor_before = [c.eng.get_net(r, 0) for r in range(c.R)]
        m, pre, t0 = step(c)
        names = launched(c)
        for r in range(c.R):
            assert np.isfinite(m[r]).all(), (tag, r, m[r])
            if algo in ("cql", "edac"):
                check_sac_actor(c, r, m, pre[r], t0, fused, tag + (r,))
                (check_cql_critics if algo == "cql" else check_edac_critics)(c, r, m, pre[r], t0, tag + (r,))
            elif algo == "iql":
                check_iql(c, r, m, actor_before[r], tag + (r,))
            else:
                check_td3bc(c, r, m, True, None, tag + (r,))
        if algo in ("cql", "edac"):
            want = expect if expect is not None else (FUSED if fused is True else SEPARATE)
            gone = absent if absent is not None else ((SEPARATE - {"tanh_sample"}) if fused is True else FUSED)
            assert want <= names and not (gone & names), (tag, sorted(names))
        elif algo == "iql":
            assert {"iql_v_loss", "iql_q_loss", "iql_actor_loss"} <= names, sorted(names)
        else:
            assert {"det_action", "td_loss", "td3_actor_loss", "td3_actor_bwd"} <= names, sorted(names)
            last = [metric(c, m, r, "loss/actor") for r in range(c.R)]
            m2, _, _ = step(c)                                   # update_actor_freq = 2: the second step trains the critics only
            for r in range(c.R):
                check_td3bc(c, r, m2, False, last[r], tag + (r, "critic-only"))
            assert "td3_report" in launched(c)
        return c
    except BaseException:
        c.eng.close()
        raise


def run(algo, **kw):
    run_case(algo, **kw).eng.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# shape sweep
# ---------------------------------------------------------------------------------------------------------------------------------
CQL_SHAPES = [
    dict(), dict(B=1), dict(B=31, N=3), dict(B=255), dict(B=257), dict(B=300, N=3), dict(B=513),          # k_cql_loss_rows on 1, 1, 1, 1, 2, 2, 3 workgroups
    dict(A=1), dict(A=8), dict(A=9), dict(A=16), dict(A=17), dict(A=32), dict(od=1), dict(od=31), dict(R=3),
    dict(B=257, A=17), dict(precision=1), dict(B=257, A=17, precision=1), dict(B=300, precision=1, N=3),
    dict(B=31, N=3, max_q_backup=1), dict(B=257, deterministic_backup=0, auto_alpha=0, alpha=0.2), dict(B=300, with_lagrange=1),
    dict(B=64, A=17, with_lagrange=1, deterministic_backup=0, R=2),
]


def _id(d):
    return "-".join(f"{k}{v}" for k, v in d.items()) or "base"


@pytest.mark.parametrize("kw", CQL_SHAPES, ids=_id)
def test_cql_row_kernels(kw):
    run("cql", **kw)


@pytest.mark.parametrize("kw", [dict(), dict(B=1, A=32), dict(B=31, max_q_backup=1), dict(B=257, A=17), dict(B=513), dict(R=3), dict(A=9, od=31),
                                dict(B=300, precision=1), dict(B=255, deterministic_backup=1), dict(B=64, A=16, auto_alpha=0, alpha=0.2)], ids=_id)
def test_edac_row_kernels(kw):
    run("edac", **kw)


@pytest.mark.parametrize("kw", [dict(), dict(B=1), dict(B=31, A=8), dict(B=257, A=17), dict(B=513, A=1), dict(R=3), dict(B=300, precision=1),
                                dict(od=31, A=32), dict(B=255, od=1, A=9)], ids=_id)
def test_iql_row_kernels(kw):
    run("iql", **kw)


@pytest.mark.parametrize("kw", [dict(), dict(B=1), dict(B=31, A=8), dict(B=257, A=17), dict(B=513, A=32), dict(R=3), dict(B=300, precision=1),
                                dict(od=1, A=9), dict(B=255, od=31, A=16)], ids=_id)
def test_td3bc_row_kernels(kw):
    run("td3bc", **kw)


@pytest.mark.parametrize("env, fused, expect, absent", [
    ({}, True, FUSED | {"actor", "actor2"}, SEPARATE),                                   # sampling in the forward's epilogue, fused actor phase
    ({"ORL_FUSE_SMALL": "0"}, False, SEPARATE | {"actor", "critic_a"}, FUSED),           # one-launch forwards, every row kernel its own launch
    ({"ORL_SMALL_FWD": "0"}, False, SEPARATE, FUSED | {"actor", "critic_a"}),            # tiled / weight-stationary launches only
], ids=["fused", "fuse_small_0", "small_fwd_0"])
@pytest.mark.parametrize("precision", [0, 1])
def test_cql_row_kernels_behind_the_few_rows_launches(monkeypatch, env, fused, expect, absent, precision):
    """hidden [256, 256], where the one-launch forward and the fused actor phase apply: the profile says which launches ran"""
    run("cql", hidden=(256, 256), B=64, R=2, precision=precision, env=env, monkeypatch=monkeypatch, fused=fused, expect=expect, absent=absent)


def test_cql_head_backward_weighs_unit_seed_gradients_when_the_fused_actor_backward_does_not_apply():
    """hidden [256, 256], B = 2080 = 65 row groups, one more than the fused actor backward takes (64), and 4160 critic rows, which the
    one-launch critic forward + unit-seed backward still takes (8192): k_actor_loss's dqa then feeds nothing but k_head_bwd, which
    forms da = sum_c dqa[c][b] dxa[c][b] itself -- the only shape class of the four algorithms that reaches that branch"""
    run("cql", hidden=(256, 256), B=2080, fused="unit_seed", expect={"critic_a.qgrad", "actor_loss", "head_bwd"}, absent={"actor.bwd_fused"})


def test_cql_nine_actions_at_hidden_256_take_the_separate_row_kernels():
    """2 A = 18 head outputs are beyond the one-launch forward (16) and 9 action columns beyond its unit-seed backward (8): the critic
    pass is still one launch, sampling, loss and head backward are their own"""
    run("cql", hidden=(256, 256), B=32, A=9, expect=SEPARATE | {"critic_a"}, absent=FUSED | {"actor", "actor2"})


# ---------------------------------------------------------------------------------------------------------------------------------
# value edges (B = 64, A = 17, precision 0)
# ---------------------------------------------------------------------------------------------------------------------------------
def _next(x, to):
    return float(np.nextafter(f32(x), f32(to)))


LS_TABLE = [-5.0, _next(-5, -9), _next(-5, 9), 2.0, _next(2, -9), _next(2, 9), -20.0, 20.0, 0.0]
MU_TABLE = [0.0, 0.5, -0.5, 3.0, -3.0, 9.0, -9.0, 20.0, -20.0]


def _constant_head(c):
    A = c.A
    for st, n in zip(c.sts, c.noises):
        a = st["actor"]
        a["dist_net.mu.weight"][:] = 0
        a["dist_net.sigma.weight"][:] = 0
        a["dist_net.sigma.bias"][:] = [LS_TABLE[j % 9] for j in range(A)]
        a["dist_net.mu.bias"][:] = [MU_TABLE[(j + 4 * (j // 9)) % 9] for j in range(A)]
        for k in ("eps_actor", "eps_next"):
            n[k][:5] = np.array([0.0, 1.0, -1.0, 4.0, -4.0], f32)[:, None]


@pytest.mark.parametrize("algo", ["cql", "edac"])
def test_constant_head_actor_on_and_beyond_both_clamps(algo):
    c = run_case(algo, B=64, A=17, mutate=_constant_head)
    try:
        B, A = c.B, c.A
        head = c.eng.debug_read(0, "head").reshape(B, 2 * A)
        assert np.array_equal(head[:, A:], np.broadcast_to(np.array([LS_TABLE[j % 9] for j in range(A)], f32), (B, A)))
        dh = c.eng.debug_read(0, "dhead").reshape(B, 2 * A)
        gated = (head[0, A:] < -5) | (head[0, A:] > 2)
        assert gated.sum() == 8 and (dh[:, A:][:, gated] == 0).all() and (dh[:, A:][:, ~gated] != 0).any(axis=0).all()
        xa = c.eng.debug_read(0, "xa").reshape(B, c.XP)[:, c.od:c.od + A]
        assert (np.abs(xa) == 1.0).any() and (np.abs(xa) <= 1.0).all()            # saturated actions: only the 1e-6 term is left in the Jacobian
        assert np.isfinite(c.eng.debug_read(0, "logp_a")).all() and np.isfinite(dh).all()
    finally:
        c.eng.close()


def _tie(c):
    for st in c.sts:
        if c.algo == "cql":
            st["critic2"] = {k: v.copy() for k, v in st["critic1"].items()}
        else:
            for k, v in st["critics"].items():
                v[:] = v[0]


def test_tied_twin_critics_split_the_seed_evenly():
    c = run_case("cql", B=64, A=17, mutate=_tie)
    try:
        assert np.array_equal(c.eng.debug_read(0, "q1a"), c.eng.debug_read(0, "q2a"))
        assert (c.eng.debug_read(0, "dqa") == f32(-1.0) / f32(64) / f32(2)).all()
    finally:
        c.eng.close()


def test_tied_ensemble_members_share_the_seed():
    """K = 4 equal members: the seeds of a row sum to -1/B and sit on members at the minimum only (the reference's min(dim = 0) sends the
    whole seed to one index: no more than both semantics share is asserted)"""
    c = run_case("edac", B=64, A=17, mutate=_tie)
    try:
        qa, dqa = c.eng.debug_read(0, "qas").reshape(4, 64), c.eng.debug_read(0, "dqa").reshape(4, 64)
        assert (qa == qa[0]).all()
        assert (dqa.astype(np.float64).sum(axis=0) == float(f32(-1.0) / f32(64))).all() and ((dqa != 0) == (qa == qa.min(axis=0))).all()
    finally:
        c.eng.close()


def _batch_edge(kind):
    def f(c):
        for b in c.batches:
            if kind == "terminal":
                b["terminals"][:] = 1
            elif kind == "alive":
                b["terminals"][:] = 0
            else:
                b["rewards"][:] = 1e3 * np.sign(b["rewards"] + f32(0.1))
    return f


@pytest.mark.parametrize("algo, kw, kind", [("cql", dict(deterministic_backup=0), "terminal"), ("cql", dict(deterministic_backup=0), "alive"),
                                           ("cql", dict(deterministic_backup=0), "reward1e3"), ("edac", {}, "alive"), ("edac", {}, "terminal"),
                                           ("iql", {}, "reward1e3"), ("iql", {}, "terminal"), ("td3bc", {}, "terminal"), ("td3bc", {}, "reward1e3")],
                         ids=lambda v: v if isinstance(v, str) else "")
def test_all_terminal_no_terminal_and_large_rewards(algo, kw, kind):
    run(algo, B=64, A=17, mutate=_batch_edge(kind), **kw)


@pytest.mark.parametrize("shift", [50.0, -50.0])
def test_iql_advantage_weights_at_the_cap_and_underflowing(shift):
    def mutate(c):
        for st in c.sts:
            for k in ("critic_q1_old", "critic_q2_old"):
                st[k]["last.bias"] = (st[k]["last.bias"] + f32(shift)).astype(f32)
    c = run_case("iql", B=64, A=17, mutate=mutate)
    try:
        ea = c.eng.debug_read(0, "exp_a")
        assert (ea == (100.0 if shift > 0 else 0.0)).all(), ea
    finally:
        c.eng.close()


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_td3bc_noise_beyond_the_clip_and_actions_beyond_max_action(sign):
    def mutate(c):
        for st, n in zip(c.sts, c.noises):
            n["eps_target"][:] = sign * 5.0
            n["eps_target"][1::2] *= -1
            st["actor_old"]["last.bias"] = (st["actor_old"]["last.bias"] + f32(sign * 5.0)).astype(f32)
    c = run_case("td3bc", B=64, A=17, mutate=mutate)
    try:
        xt = c.eng.debug_read(0, "xt").reshape(64, c.XP)[:, c.od:c.od + 17]
        assert (xt[0::2] == sign).all() and (np.abs(xt[1::2] - sign * (1.0 - 0.5)) < 0.05).all()
    finally:
        c.eng.close()


@pytest.mark.parametrize("auto_alpha", [1, 0])
@pytest.mark.parametrize("cla", [20.0, -20.0])
def test_cql_lagrange_multiplier_beyond_and_far_below_its_clamp(cla, auto_alpha):
    from offlinerlkit import _engine
    c = run_case("cql", B=64, A=17, with_lagrange=1, cql_log_alpha=cla, auto_alpha=auto_alpha, alpha=0.2, deterministic_backup=0)
    try:
        after = c.eng.get_scalar(0, _engine.SCALAR_CQL_LOG_ALPHA)
        if cla > 0:          # exp(20) > 1e6: the multiplier is 1e6, the clamp passes no gradient, Adam's moments stay 0: nothing moves
            assert after == cla and c.eng.get_scalar(0, _engine.SCALAR_CQL_LOG_ALPHA_M) == 0.0
        else:
            assert after != cla
    finally:
        c.eng.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# optimizer: k_adam + the fused Polyak sync on the engine's own gradient
# ---------------------------------------------------------------------------------------------------------------------------------
def _flat(eng, net, d):
    from offlinerlkit import _engine
    return _engine._flatten(eng.net_tensors(net), d, eng.net_floats(net))


def _plan(c, t0):
    """[(net, target or None, lr, Adam's step number)] of the step that follows step count t0"""
    cfg, ids = c.cfg, NETS[c.algo]
    if c.algo == "cql":
        return [(ids["actor"], None, cfg.actor_lr, t0 + 1), (ids["critic1"], ids["critic1_old"], cfg.critic_lr, t0 + 1), (ids["critic2"], ids["critic2_old"], cfg.critic_lr, t0 + 1)]
    if c.algo == "edac":
        return [(ids["actor"], None, cfg.actor_lr, t0 + 1), (ids["critics"], ids["critics_old"], cfg.critic_lr, t0 + 1)]
    if c.algo == "iql":
        return [(ids["critic_v"], None, cfg.critic_v_lr, t0 + 1), (ids["critic_q1"], ids["critic_q1_old"], cfg.critic_lr, t0 + 1),
                (ids["critic_q2"], ids["critic_q2_old"], cfg.critic_lr, t0 + 1), (ids["actor"], None, cfg.actor_lr, t0 + 1)]
    f = cfg.update_actor_freq
    actor_step = t0 % f == 0
    plan = [(ids["critic1"], ids["critic1_old"] if actor_step else None, cfg.critic_lr, t0 + 1), (ids["critic2"], ids["critic2_old"] if actor_step else None, cfg.critic_lr, t0 + 1)]
    return plan + ([(ids["actor"], ids["actor_old"], cfg.actor_lr, t0 // f + 1)] if actor_step else [])


@pytest.mark.parametrize("algo, kw", [("cql", {}), ("edac", {}), ("iql", {}), ("td3bc", dict(update_actor_freq=3))], ids=["cql", "edac", "iql", "td3bc_freq3"])
def test_adam_and_polyak_on_the_engines_own_gradient(algo, kw):
    """obs_dim 5, act_dim 3, hidden [32, 32]: tensor groups end off multiples of four, so both the 16-byte path and the single-element
    path of k_adam run; B = 8 keeps every gradient in one slab, so the gradient that ``debug_grads`` returns is the one k_adam read.
    The engine's Adam is Adam for the fp32 betas its configuration holds (row_refs.adam_consts); exp_avg_sq is also held to within
    2e-5 relative of torch's own scalars (1 - 0.999 -> fp32(0.001), 1.3e-5 above 1 - fp32(0.999)), so that the gap cannot widen unnoticed"""
    c = make(algo, B=8, **kw)
    eng, cfg = c.eng, c.cfg
    rng = np.random.RandomState(5)
    try:
        every = sorted(set(NETS[algo].values()))
        for t0 in (0, 1, 999, 10 ** 6):
            plan = _plan(c, t0)
            for net, _, _, _ in _plan(c, 0):
                n = eng.net_floats(net)
                eng.set_adam_state(0, net, (1e-3 * rng.standard_normal(n)).astype(f32), (1e-6 * rng.uniform(0.01, 1.0, n)).astype(f32))
            eng.set_step_count(t0)
            before = {net: _flat(eng, net, eng.get_net(0, net)) for net in every}
            mom = {net: eng.adam_state(0, net) for net, _, _, _ in _plan(c, 0)}
            step(c)
            trained = {p[0] for p in plan} | {p[1] for p in plan if p[1] is not None}
            for net, tgt, lr, t in plan:
                g = _flat(eng, net, eng.debug_grads(0, net))
                assert np.isfinite(g).all() and (g != 0).mean() > 0.2, (algo, net, t0)
                ref = rr.adam(before[net], mom[net][0], mom[net][1], g, lr, cfg.adam_beta1, cfg.adam_beta2, cfg.adam_eps, t,
                              tau=cfg.tau if tgt is not None else None, target=before[tgt] if tgt is not None else None)
                m1, v1 = eng.adam_state(0, net)
                tag = (algo, net, t0)
                holds(_flat(eng, net, eng.get_net(0, net)), ref[0], "adam.param", tag)
                holds(m1, ref[1], "adam.exp_avg", tag)
                holds(v1, ref[2], "adam.exp_avg_sq", tag)
                dec = lambda x: float(np.format_float_positional(f32(x), unique=True))      # the decimal hyper-parameter the fp32 field came from
                tv = rr.adam(before[net], mom[net][0], mom[net][1], g, dec(lr), dec(cfg.adam_beta1), dec(cfg.adam_beta2), dec(cfg.adam_eps), t, torch_scalars=True)[2]
                assert (np.abs(v1 - tv.v) <= 2e-5 * np.abs(tv.v) + rr.FACTOR * tv.e).all(), (tag, "exp_avg_sq against torch's scalars")
                if tgt is not None:
                    holds(_flat(eng, tgt, eng.get_net(0, tgt)), ref[3], "adam.polyak_target", tag)
            for net in every:                                 # what the step does not train or sync keeps its bits (TD3+BC's critic-only steps)
                if net not in trained:
                    assert np.array_equal(_flat(eng, net, eng.get_net(0, net)), before[net]), (algo, net, t0)
    finally:
        eng.close()
