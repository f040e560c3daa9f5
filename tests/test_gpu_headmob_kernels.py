"""GPU: the four schedules tests/test_gpu_row_kernels.py and tests/test_gpu_mcq_edac_kernels.py leave out -- k_rcsl_loss (RCSL),
k_rcslg_head (Gaussian RCSL), k_autoreg_head / k_autoreg_draw (the autoregressive policy), k_mobile_assemble / k_lcb_penalty /
k_mobile_td_loss (MOBILE) -- and the dynamic-scale kernels grad_scale_publish / k_grad_scale of every schedule, each against its float64
restatement (tests/row_refs.py) ON THE ENGINE'S OWN OPERANDS, read back through ``debug_read`` after one real step, so that the engine's
own launch geometry and host dispatch are what is tested.

Bar, for EVERY element of every result and for every metric: |got - f64| <= 4 x the first-order fp32 bound the restatement propagates
through its own arithmetic (proven against float64 autograd and the numpy oracles, with planted defects, in
tests/test_headmob_refs_cpu.py); exact equality where the operation rounds nothing: copies (input matrices, batch slots, expanded rows,
observation columns), selections (``lcb_q`` = min(ql1, ql2), the clamp ends of the log-variance), zeros (padding rows, padding columns,
shut gates, one-hot columns after the last draw, real rows of the penalty) and the power-of-two scales.

Cases (tests/headmob_cases.py), one edge at a time, hidden [32, 32], precision 0; each family's base case also at precision 1 and 2.
  k_rcsl_loss       from B = 32, A = 3, obs_dim 5: B 1 / 85 / 86 (B A = 255 / 258) / 257, A 1 / 32, three runs; ordered-epoch steps with 1 valid
                    row, B - 1 valid rows and interleaved padding: dpred exactly 0 on padding rows, ``rcsl_x`` and the batch slots byte-exact
                    against the gathered rows (k_rcsl_prepare<RI_ORDER>; a padding row reads dataset row 0).
  k_rcslg_head      from B = 32, A = 3: A 1 / 5 / 17 / 31 / 32 (1, 1, 3, 8, 9 head gradients per thread), B 1 / 63 / 64 / 65 / 129, A = 32 with
                    B 65 / 129 (full 2048-element chunks), three runs, the same padding patterns plus a padding row inside the first chunk
                    and the only valid row in the last chunk of B = 129.  Value edges at B = 64, A = 17 with W_sigma = 0: the raw
                    log-variance on, one ulp inside / outside and far beyond -5 and 2 (the taps equal the clamp ends exactly, the sigma
                    gradients are exactly 0 where the gate is shut), mu - a up to +-20 at log-variance -5.  The head gradients come
                    through ``debug_grads``: slab 0 only, so its "rounded exact sum" is the kernel's own value.  dmu / ds are not
                    stored by the kernel: they are held through dz and the four head gradients, which are sums of nothing else.
                    The gate is taken from the clamped tap: strictly inside (-5, 2) it is the raw value; on an end the gate is open
                    only where the float64 raw value is the end within its bound (row_refs.rcslg_head).
  k_autoreg_head    from B = 16, A = 2: A 1 / 3 / 32, B 1 / 8 / 86 (M = 258 at A = 3) / 257 at A = 1, three runs, padding through the ordered epoch
                    (every one of the A expanded rows of a padded batch row has dz == 0, and no other row does); ``ar_x`` / ``ar_target``
                    byte-exact on every step, the padded ones included.  Value edges with a constant tail: both outputs exactly 0,
                    logstd -8 (pre-activation -800) and +8, targets 50 and 5000 away from the mean.
  k_autoreg_draw    n 1 / 255 / 257, A 1 / 2 / 32, three runs, host eps: the last pass's column od + A - 1 of ``ar_sx`` is held to the
                    restatement on ``ar_sz`` / ``ar_seps``; after the call the observation columns are byte-exact, every one-hot and
                    every padding column exactly 0; at A = 1 that is the whole sample.  Earlier columns at A > 1 stay with the 1e-5-of-
                    scale oracle test of tests/test_gpu_autoreg.py (their tails are overwritten by the later passes).
  MOBILE            from B = 16, S = 3, E = 3, real_rows = 4, obs_dim 5: E 2 / 64 (LCB_MAX_E), S 1 / 5, B 1 / 257 (S E = 2), real_rows 0 / B,
                    obs_dim 1 / 31, B 255 / 513 for k_mobile_td_loss, deterministic backup, fixed / learnt alpha, penalty_coef 0 / 7,
                    three runs; samples identical across elites (penalty exactly 0), all-terminal / no-terminal batches, rewards of
                    -1e3 (y exactly 0 on every row) and +1e3, tied target critics.  ``xs`` and the observation / padding columns of
                    ``xl`` byte-exact against the samples handed to orl_engine_set_next_samples; ``lcb_q`` == min(ql1, ql2).  Only
                    finite inputs: the health flag is not driven.
  dynamic scale     precision 1 and 2: the ``gscale`` tap (this run's slots of the last step, in the schedule's order -- written down
                    next to orl_debug_read in csrc/engine.hip) equals row_refs.pow2_scale(max |seed|) of the tapped seed, exactly, with
                    max |seed| * scale in [8, 16): the four seed kernels above (1.0 on an all-zero seed: RCSL, Gaussian RCSL, MOBILE; the
                    autoregressive seed cannot be all zero -- d logstd = 1 - d^2 and d mean ~ d do not vanish together), and the seed
                    kernels the two earlier modules drive: k_head_bwd, k_cql_loss_rows (it takes the maximum before the last
                    multiply-divide of dq, two roundings apart from the stored entries: both neighbours must agree), k_td_loss,
                    k_td3_actor_loss (lambda / B), k_td3_actor_bwd, k_iql_v_loss / q_loss / actor_loss, k_edac_gamma.  k_grad_scale
                    itself: CQL at B = 513 (``actor.bwd.gscale`` in the profile; dhead: 513 x 6), EDAC's tail weights (a seed per member),
                    three backward passes of MCQ (dm3, dehead, dq [2][3B]) and MOBILE's dhead at B = 257, all asserted from the profile.

Every tap used is live after the step: each workspace is its own allocation; the backward passes read their seeds (``dpred``, ``dz``,
``ar_dz``, ``dq``) without scaling them in place; MOBILE's actor phase, which follows the critics, has its own buffers and writes none of
``ql``, ``xs``, ``xl``, ``logp_l``, ``lcb_q``, ``penalty``, ``qt``, ``q``, ``dq``, ``logp_next``, ``target_q``; the sampling workspaces are
registered by orl_autoreg_sample itself, for the call's n rows.  The head of k_rcslg_head's reference is the case's own pre-step
parameters (the step ends with their Adam update); the temperature of k_mobile_td_loss is the one the step began with.

Measured worst |err| / bound over the whole module (MI355X; the bar is 4, a correct kernel is expected below 1; the module prints them):
    k_rcsl_loss        loss 0.16, dpred 0.55; padding rows, rcsl_x and the batch slots exact
    k_rcslg_head       mu 0.67, logvar 0.75, loss 0.10, dz 0.38, head gradients mu.weight 0.11 / mu.bias 0.09 / sigma.weight 0.09 / sigma.bias 0.08;
                       clamp ends, shut gates and padding rows exact
    k_autoreg_head     out 0.94, loss 0.16, dz 0.49; padding rows, ar_x / ar_target exact
    k_autoreg_draw     drawn action 0.53; observation, one-hot and padding columns exact
    k_mobile_assemble  exact
    k_lcb_penalty      penalty 0.12 (the kernel sums in double: it sits far inside the fp32 bound); lcb_q, real rows, identical elites exact
    k_mobile_td_loss   target_q 0.77, loss 0.14, dq 0.68; the clamp at 0 exact
    grad_scale_publish (every seed kernel named above) and k_grad_scale: every slot equal to pow2_scale of its seed (0)
Every figure sits below 1, i.e. inside the first-order bound itself, a factor 4 inside the bar.  No kernel or dispatch defect was found."""
import numpy as np
import pytest

import autoreg_oracle as aorc
import headmob_cases as hc
import mcq_edac_cases as mc
import row_refs as rr
import test_gpu_row_kernels as rk

pytestmark = pytest.mark.gpu
f32 = np.float32
KEYS = ("rcsl_", "rcslg_", "autoreg_", "mobile_", "lcb_", "grad_scale")
ALGO = {"rcsl": "rcsl", "rcslg": "rcsl_gauss", "autoreg": "autoreg"}
NET = 0
MOBILE_NETS = {"actor": 0, "critic1": 1, "critic2": 2, "critic1_old": 3, "critic2_old": 4}


@pytest.fixture(scope="module", autouse=True)
def _figures():
    yield
    print("\nworst |got - f64| / bound per supervised-head / MOBILE / dynamic-scale result (0: exact):",
          {k: round(v, 4) for k, v in sorted(rk.WORST.items()) if k.startswith(KEYS)})


holds = rk.holds


def exact(cond, key, tag):
    """an equality the operation owes exactly: recorded as ratio 0 in the summary"""
    assert cond, (key,) + tuple(tag)
    rk.WORST[key] = max(rk.WORST.get(key, 0.0), 0.0)


def check_scale(c, r, slot, seed, key, tag, count=None, neighbours=False):
    """slot ``slot`` of the ``gscale`` tap equals pow2_scale(max |seed|) exactly and puts the largest entry into [8, 16)"""
    gs = c.eng.debug_read(r, "gscale")
    if c.eng.cfg.precision == 0:
        assert gs.size == 0, (tag, gs)
        return
    assert count is None or gs.size == count, (tag, gs)
    a = float(np.abs(np.asarray(seed, f32)).max(initial=0.0))
    want = rr.pow2_scale(a)
    if neighbours:              # the kernel's maximum is two roundings apart from the stored entries: it decides unless a power of two lies between
        assert rr.pow2_scale(a * (1 - 4 * rr.U)) == want == rr.pow2_scale(a * (1 + 4 * rr.U)), (tag, "max |seed| sits on a power of two", a)
    exact(float(gs[slot]) == want, key, tag + ("gscale", float(gs[slot]), want, a))
    assert a == 0.0 or 8.0 <= a * want < 16.0, (tag, a, want)
    assert a > 0.0 or want == 1.0, tag


# ---------------------------------------------------------------------------------------------------------------------------------
# the supervised families
# ---------------------------------------------------------------------------------------------------------------------------------
def make_sup(family, **kw):
    from offlinerlkit import _engine
    c = hc.inputs(family, **kw)
    cfg = dict(obs_dim=c.od, act_dim=c.A, hidden=c.hidden, batch_size=c.B, n_runs=c.R, precision=c.precision, actor_lr=3e-4)
    cfg.update(c.over)
    c.eng = _engine.Engine(_engine.default_config(ALGO[family], **cfg))
    for r in range(c.R):
        c.eng.set_net(r, NET, c.nets[r])
    c.eng.profile_enable(True)
    c.buf = None
    return c


def step_sup(c):
    """one step: orl_step on the rows (every row valid), or -- a padded case -- one step of an ordered epoch over a dataset that holds the
    rows of every run, run r's order naming its own rows and -1 for padding.  Returns (metrics [R], the rows each run's step saw)"""
    from offlinerlkit import _engine
    if c.pad is None:
        batch = dict(observations=np.stack([b["observations"] for b in c.rows]), actions=np.stack([b["actions"] for b in c.rows]))
        if c.family != "autoreg":
            batch["rewards"] = np.stack([b["rtgs"] for b in c.rows])
        return np.asarray(c.eng.step(batch, []))[:, 0], c.rows
    data = {k: np.concatenate([b[k] for b in c.rows]) for k in c.rows[0]}
    n = len(data["observations"])
    c.buf = _engine.DeviceBuffer(c.od, c.A)
    c.buf.load(data["observations"], data["actions"], data["observations"], data["rtgs"].reshape(n), np.zeros(n, f32))
    c.eng.attach_buffer(c.buf)
    order = np.stack([np.where(c.valid[r], r * c.B + np.arange(c.B), -1) for r in range(c.R)]).astype(np.int64)
    m, _ = c.eng.learn_epoch(order)
    seen = [{k: v[np.where(order[r] < 0, 0, order[r])] for k, v in data.items()} for r in range(c.R)]      # padding reads dataset row 0
    return m[:, 0], seen


def check_slots(c, r, seen, tag):
    """the batch slots hold the gathered rows byte for byte (k_rcsl_prepare / k_autoreg_prepare, RI_ORDER on a padded case)"""
    T = lambda name: c.eng.debug_read(r, name)
    exact(T("b_obs").reshape(c.B, c.od).tobytes() == seen["observations"].tobytes() and T("b_act").reshape(c.B, c.A).tobytes() == seen["actions"].tobytes(),
          f"{c.family}_prepare.slots", tag)


def check_rcsl(c, r, loss, seen, tag):
    B, A, od = c.B, c.A, c.od
    T = lambda name: c.eng.debug_read(r, name)
    v = c.valid[r]
    check_slots(c, r, seen, tag)
    exact(T("rcsl_x").reshape(B, od + 1).tobytes() == np.concatenate([seen["observations"], seen["rtgs"]], axis=1).tobytes(), "rcsl_prepare.x", tag)
    pred, act, dp = T("pred").reshape(B, A), T("b_act").reshape(B, A), T("dpred").reshape(B, A)
    L, rdp = rr.rcsl_loss(pred, act, v)
    holds(loss, L, "rcsl_loss.loss", tag)
    holds(dp, rdp, "rcsl_loss.dpred", tag)
    exact((dp[~v] == 0).all(), "rcsl_loss.dpred_padding", tag)
    check_scale(c, r, 0, dp, "grad_scale_publish.rcsl_loss", tag, count=1)


def check_rcslg(c, r, loss, seen, tag):
    B, A, od = c.B, c.A, c.od
    T = lambda name: c.eng.debug_read(r, name)
    v = c.valid[r]
    check_slots(c, r, seen, tag)
    exact(T("rcsl_x").reshape(B, od + 1).tobytes() == np.concatenate([seen["observations"], seen["rtgs"]], axis=1).tobytes(), "rcsl_prepare.x", tag)
    z, act, mu, lv, dz = (T(n).reshape(B, A) for n in ("z", "b_act", "mu", "logvar", "dz"))
    assert np.isfinite(dz).all() and lv.min() >= -5.0 and lv.max() <= 2.0, tag
    ref = rr.rcslg_head(z, act, c.nets[r], v, logvar32=lv)
    holds(mu, ref["mu"], "rcslg_head.mu", tag)
    holds(lv, ref["logvar"], "rcslg_head.logvar", tag)
    holds(loss, ref["loss"], "rcslg_head.loss", tag)
    holds(dz, ref["dz"], "rcslg_head.dz", tag)
    exact((dz[~v] == 0).all(), "rcslg_head.dz_padding", tag)
    g = c.eng.debug_grads(r, NET)
    for k in rr.RG_HEAD:
        holds(g[k].reshape(ref["grads"][k].shape), ref["grads"][k], "rcslg_head.g_" + k.split(".", 1)[1], tag)
    check_scale(c, r, 0, dz, "grad_scale_publish.rcslg_head", tag, count=1)
    return ref, lv, g


def check_autoreg(c, r, loss, seen, tag):
    B, A, od = c.B, c.A, c.od
    M = A * B
    T = lambda name: c.eng.debug_read(r, name)
    v = c.valid[r]
    check_slots(c, r, seen, tag)
    x, t = aorc.expand(seen["observations"], seen["actions"])
    tt = T("ar_target").reshape(M)
    # (value equality for ar_x: the oracle's masked action columns hold -0.0 where it multiplied a negative action by 0, the kernel writes +0)
    exact(np.array_equal(T("ar_x").reshape(M, od + 2 * A), x) and tt.tobytes() == t.tobytes(), "autoreg_prepare.x_target", tag)
    z, out, dz = T("ar_z").reshape(M, 2), T("ar_out").reshape(M, 2), T("ar_dz").reshape(M, 2)
    assert np.isfinite(out).all() and np.isfinite(dz).all(), tag
    rout, L, rdz = rr.autoreg_head(z, tt, A, v)
    holds(out, rout, "autoreg_head.out", tag)
    holds(loss, L, "autoreg_head.loss", tag)
    holds(dz, rdz, "autoreg_head.dz", tag)
    pad_m = ~np.tile(v, A)                                  # expanded row m = j B + b belongs to batch row m % B
    exact((dz[pad_m] == 0).all() and (dz[~pad_m] != 0).any(axis=1).all(), "autoreg_head.dz_padding", tag)
    check_scale(c, r, 0, dz, "grad_scale_publish.autoreg_head", tag, count=1)
    return z, out, dz


CHECK = {"rcsl": check_rcsl, "rcslg": check_rcslg, "autoreg": check_autoreg}
LAUNCH = {"rcsl": {"rcsl_prepare", "rcsl_loss"}, "rcslg": {"rcsl_prepare", "rcslg_head"}, "autoreg": {"autoreg_prepare", "autoreg_head"}}


def run_sup(family, **kw):
    c = make_sup(family, **kw)
    try:
        tag = (family, hc.case_id(kw))
        loss, seen = step_sup(c)
        assert LAUNCH[family] <= rk.launched(c), sorted(rk.launched(c))
        assert not any(n.endswith(".gscale") for n in rk.launched(c)), "the seed kernel publishes its own scale: no k_grad_scale launch"
        out = []
        for r in range(c.R):
            assert np.isfinite(loss[r]), (tag, r, loss)
            out.append(CHECK[family](c, r, loss[r], seen[r], tag + (r,)))
        return c, out
    except BaseException:
        c.eng.close()
        raise


@pytest.mark.parametrize("kw", hc.RCSL_SHAPES, ids=hc.case_id)
def test_rcsl_loss(kw):
    run_sup("rcsl", **kw)[0].eng.close()


@pytest.mark.parametrize("kw", hc.RCSLG_SHAPES, ids=hc.case_id)
def test_rcslg_head(kw):
    run_sup("rcslg", **kw)[0].eng.close()


def test_rcslg_head_on_and_beyond_both_clamp_ends():
    c, out = run_sup("rcslg", **hc.RCSLG_EDGES[0])
    try:
        ref, lv, g = out[0]
        B, A = c.B, c.A
        raw = np.array([hc.LV_TABLE[j % 9] for j in range(A)], f32)
        exact(np.array_equal(lv, np.broadcast_to(np.clip(raw, f32(-5), f32(2)), (B, A))), "rcslg_head.clamp_ends", ("edges",))
        shut = (raw < -5) | (raw > 2)
        gb, gw = g["dist_net.sigma.bias"].ravel(), g["dist_net.sigma.weight"].reshape(A, A)
        exact(shut.sum() == 8 and (gb[shut] == 0).all() and (gw[shut] == 0).all() and (gb[~shut] != 0).all(), "rcslg_head.shut_gate", ("edges",))
        assert np.array_equal(ref["gate"], np.broadcast_to(~shut, (B, A)))
        act = c.eng.debug_read(0, "b_act").reshape(B, A)
        d = c.eng.debug_read(0, "mu").reshape(B, A) - act
        assert d[:, 0].max() > 19.0 and d[:, 9].min() < -19.0
    finally:
        c.eng.close()


@pytest.mark.parametrize("kw", hc.AUTOREG_SHAPES, ids=hc.case_id)
def test_autoreg_head(kw):
    run_sup("autoreg", **kw)[0].eng.close()


@pytest.mark.parametrize("kw", hc.AUTOREG_EDGES, ids=hc.case_id)
def test_autoreg_head_value_edges(kw):
    c, res = run_sup("autoreg", **kw)
    try:
        z, out, dz = res[0]
        name = kw["mutate"].__name__
        b_mean, b_ls = (float(x) for x in name[5:-1].split(","))
        assert (z == np.array([b_mean, b_ls], f32)).all(), name
        if name == "tail(0,0)":
            assert (out == 0).all()
        elif b_ls == -800.0:
            assert (out[:, 1] == f32(0.01) * f32(-800.0)).all()
    finally:
        c.eng.close()


@pytest.mark.parametrize("kw", hc.DRAW_SHAPES, ids=hc.case_id)
def test_autoreg_draw(kw):
    from offlinerlkit import _engine
    c = hc.draw_inputs(**kw)
    n, A, od = c.n, c.A, c.od
    XP = (od + 2 * A + 3) // 4 * 4
    eng = _engine.Engine(_engine.default_config("autoreg", obs_dim=od, act_dim=A, hidden=c.hidden, batch_size=c.B, n_runs=c.R, precision=0))
    try:
        for r in range(c.R):
            eng.set_net(r, NET, c.nets[r])
        act = eng.autoreg_sample(c.sobs, c.seps)
        for r in range(c.R):
            tag = ("draw", hc.case_id(kw), r)
            sx, sz, se = eng.debug_read(r, "ar_sx").reshape(n, XP), eng.debug_read(r, "ar_sz").reshape(n, 2), eng.debug_read(r, "ar_seps").reshape(n, A)
            assert se.tobytes() == c.seps[r].tobytes(), tag
            exact(sx[:, :od].tobytes() == c.sobs[r].tobytes(), "autoreg_draw.obs_columns", tag)
            exact((sx[:, od + A:].view(np.uint32) == 0).all(), "autoreg_draw.onehot_and_padding", tag)
            assert np.array_equal(act[r], sx[:, od:od + A]) and np.isfinite(act[r]).all(), tag
            holds(sx[:, od + A - 1], rr.autoreg_draw(sz, se[:, A - 1]), "autoreg_draw.action", tag)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# MOBILE
# ---------------------------------------------------------------------------------------------------------------------------------
def make_mobile(**kw):
    from offlinerlkit import _engine
    c = hc.mobile_inputs(**kw)
    cfg = dict(obs_dim=c.od, act_dim=c.A, hidden=c.hidden, batch_size=c.B, n_runs=c.R, precision=c.precision, target_entropy=-float(c.A),
               mobile_num_samples=c.S, mobile_num_elites=c.E, mobile_real_rows=c.real_rows)
    cfg.update(c.over)
    c.eng = _engine.Engine(_engine.default_config("mobile", **cfg))
    for r in range(c.R):
        for nm, nid in MOBILE_NETS.items():
            c.eng.set_net(r, nid, c.sts[r][nm])
        c.eng.set_scalar(r, _engine.SCALAR_LOG_ALPHA, -0.3)
    c.eng.profile_enable(True)
    return c


def check_mobile(c, r, m, alpha0, tag):
    B, A, od, S, E, M, cfg = c.B, c.A, c.od, c.S, c.E, c.M, c.eng.cfg
    T = lambda name: c.eng.debug_read(r, name)
    OP, XP = (od + 3) // 4 * 4, (od + A + 3) // 4 * 4
    b, smp = c.batches[r], c.samples[r]
    # ---- k_mobile_assemble ----
    xs, xl = T("xs").reshape(M, OP), T("xl").reshape(M, XP)
    exact(xs[:, :od].tobytes() == smp.tobytes() and xl[:, :od].tobytes() == smp.tobytes(), "mobile_assemble.obs_columns", tag)
    exact((xs[:, od:].view(np.uint32) == 0).all() and (xl[:, od + A:].view(np.uint32) == 0).all(), "mobile_assemble.padding", tag)
    assert (np.abs(xl[:, od:od + A]) <= 1.0).all() and np.isfinite(T("logp_l")).all(), tag
    # ---- k_lcb_penalty ----
    ql = np.stack([T("ql1"), T("ql2")])
    qmin, rpen = rr.lcb_penalty(ql, B, S, E, c.real_rows)
    exact(np.array_equal(T("lcb_q"), qmin), "lcb_penalty.qmin", tag)
    pen = T("penalty")
    holds(pen, rpen, "lcb_penalty.penalty", tag)
    exact((pen[:c.real_rows] == 0).all(), "lcb_penalty.real_rows", tag)
    # ---- k_mobile_td_loss (the critics come first: the temperature is the one the step began with) ----
    alpha = alpha0 if cfg.auto_alpha else cfg.alpha
    q, qt = np.stack([T("q1"), T("q2")]), np.stack([T("qt1"), T("qt2")])
    lp = None if cfg.deterministic_backup else T("logp_next")
    tq, dq = T("target_q"), np.stack([T("dq1"), T("dq2")])
    args = (q, qt, b["rewards"].ravel(), b["terminals"].ravel(), pen, cfg.gamma, cfg.penalty_coef, B)
    y, _, _ = rr.mobile_td_loss(*args, logp_next=lp, alpha=alpha)
    holds(tq, y, "mobile_td_loss.target_q", tag)
    assert (tq >= 0).all(), tag
    _, L, rdq = rr.mobile_td_loss(*args, logp_next=lp, alpha=alpha, stored=tq)
    holds(rk.metric(c, m, r, "loss/critic"), L, "mobile_td_loss.loss", tag)
    holds(dq, rdq, "mobile_td_loss.dq", tag)
    check_scale(c, r, 0, dq, "grad_scale_publish.mobile_td_loss", tag, count=2)
    # (dhead: k_head_bwd's own scale while it is one workgroup per run, a k_grad_scale launch beyond)
    assert (B > 256 and cfg.precision > 0) == ("actor.bwd.gscale" in rk.launched(c)), sorted(rk.launched(c))
    check_scale(c, r, 1, T("dhead"), "grad_scale_publish.head_bwd" if B <= 256 else "grad_scale.k_grad_scale", tag)
    return pen, tq, qt, dq


MOBILE_LAUNCHES = {"lcb.assemble", "lcb.penalty", "td_loss"}


def run_mobile(**kw):
    from offlinerlkit import _engine
    c = make_mobile(**kw)
    try:
        tag = ("mobile", hc.case_id(kw))
        alpha0 = [c.eng.get_scalar(r, _engine.SCALAR_ALPHA) for r in range(c.R)]
        c.eng.set_next_samples(np.stack(c.samples))
        batch = {k: np.stack([b[k] for b in c.batches]) for k in c.batches[0]}
        m = c.eng.step(batch, [np.stack([n[k] for n in c.noises]) for k in ("eps_lcb", "eps_next", "eps_actor")])
        assert MOBILE_LAUNCHES <= rk.launched(c), sorted(rk.launched(c))
        out = []
        for r in range(c.R):
            assert np.isfinite(m[r]).all(), (tag, r, m[r])
            out.append(check_mobile(c, r, m, alpha0[r], tag + (r,)))
        return c, out
    except BaseException:
        c.eng.close()
        raise


@pytest.mark.parametrize("kw", hc.MOBILE_SHAPES, ids=hc.case_id)
def test_mobile_kernels(kw):
    run_mobile(**kw)[0].eng.close()


@pytest.mark.parametrize("kw", hc.MOBILE_EDGES, ids=hc.case_id)
def test_mobile_value_edges(kw):
    c, out = run_mobile(**kw)
    try:
        pen, tq, qt, dq = out[0]
        name = kw["mutate"].__name__
        if name == "identical_elites":
            exact((pen == 0).all(), "lcb_penalty.identical_elites", (name,))
        elif name == "reward-1e3":
            exact((tq == 0).all(), "mobile_td_loss.clamp_at_0", (name,))
        elif name == "reward+1e3":
            assert (tq > 900).all()
        elif name == "terminal":
            b = c.batches[0]
            want = np.maximum(b["rewards"].ravel() - f32(c.eng.cfg.penalty_coef) * pen, f32(0))
            assert np.array_equal(tq, want), "a terminal row's target is its penalised reward, clamped"
        elif name == "tied_targets":
            assert np.array_equal(qt[0], qt[1])
    finally:
        c.eng.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# the dynamic scale of a split-precision backward pass
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [1, 2])
def test_an_all_zero_seed_gets_scale_one(precision):
    c, _ = run_sup("rcsl", mutate=hc.zero_seed_rcsl, precision=precision)
    assert (c.eng.debug_read(0, "dpred") == 0).all() and c.eng.debug_read(0, "gscale").tolist() == [1.0]
    c.eng.close()
    c, _ = run_sup("rcslg", mutate=hc.zero_seed_rcslg, precision=precision)
    assert (c.eng.debug_read(0, "dz") == 0).all() and c.eng.debug_read(0, "gscale").tolist() == [1.0]
    c.eng.close()
    c, _ = run_mobile(**dict(hc.ZERO_SEED_MOBILE, precision=precision))
    assert (c.eng.debug_read(0, "dq1") == 0).all() and (c.eng.debug_read(0, "dq2") == 0).all() and c.eng.debug_read(0, "gscale")[0] == 1.0
    c.eng.close()


def _gscale_names(c):
    return {n for n in rk.launched(c) if n.endswith(".gscale")}


@pytest.mark.parametrize("precision", [1, 2])
@pytest.mark.parametrize("algo, kw", [("cql", dict()), ("cql", dict(B=513)), ("edac", dict()), ("edac", dict(mc.EDAC_BASE)), ("iql", dict()), ("td3bc", dict()),
                                      ("mcq", dict(mc.MCQ_BASE))], ids=["cql", "cql_B513", "edac", "edac_eta1", "iql", "td3bc", "mcq"])
def test_scales_of_the_seed_kernels_of_the_other_schedules(algo, kw, precision):
    """the slots in each schedule's order (csrc/engine.hip, next to orl_debug_read) against the tapped seeds"""
    c = rk.make(algo, precision=precision, **kw)
    try:
        rk.step(c)
        B, K = c.B, c.K
        T = lambda name: c.eng.debug_read(0, name)
        tag = (algo, B, precision)
        names = _gscale_names(c)
        if algo == "cql":
            if B <= 256:
                assert not names, names
                check_scale(c, 0, 0, T("dhead"), "grad_scale_publish.head_bwd", tag, count=2)
            else:            # more than one workgroup of k_head_bwd: the scale comes from a k_grad_scale launch over dhead [513 x 6]
                assert names == {"actor.bwd.gscale"}, names
                check_scale(c, 0, 0, T("dhead"), "grad_scale.k_grad_scale", tag, count=2)
            check_scale(c, 0, 1, np.concatenate([T("dq1"), T("dq2")]), "grad_scale_publish.cql_loss_rows", tag, neighbours=True)
        elif algo == "edac":
            eta = c.eng.cfg.eta > 0
            check_scale(c, 0, 0, T("dhead"), "grad_scale_publish.head_bwd", tag, count=4 if eta else 2)
            check_scale(c, 0, 1, T("dqs"), "grad_scale_publish.td_loss", tag)
            if eta:
                assert names == {"edac.delta.gscale"}, names
                check_scale(c, 0, 2, c.sts[0]["critics"][f"model.{2 * len(c.hidden)}.weight"], "grad_scale.k_grad_scale", tag)
                check_scale(c, 0, 3, T("gamma"), "grad_scale_publish.edac_gamma", tag)
        elif algo == "iql":
            assert not names, names
            check_scale(c, 0, 0, T("dv"), "grad_scale_publish.iql_v_loss", tag, count=3)
            check_scale(c, 0, 1, np.concatenate([T("dq1"), T("dq2")]), "grad_scale_publish.iql_q_loss", tag)
            check_scale(c, 0, 2, T("dmraw"), "grad_scale_publish.iql_actor_loss", tag)
        elif algo == "td3bc":
            assert not names, names
            check_scale(c, 0, 0, np.concatenate([T("dq1"), T("dq2")]), "grad_scale_publish.td_loss", tag, count=3)
            check_scale(c, 0, 1, T("dqpi"), "grad_scale_publish.td3_actor_loss", tag)
            check_scale(c, 0, 2, T("dmraw"), "grad_scale_publish.td3_actor_bwd", tag)
            rk.step(c)                                                         # a critic-only step hands out one slot
            check_scale(c, 0, 0, np.concatenate([T("dq1"), T("dq2")]), "grad_scale_publish.td_loss", tag + ("critic-only",), count=1)
        else:
            assert names == {"vae.dec.bwd.gscale", "vae.enc.bwd.gscale", "critic.bwd.gscale"}, names
            check_scale(c, 0, 0, T("dm3"), "grad_scale.k_grad_scale", tag + ("dm3",), count=4)
            check_scale(c, 0, 1, T("dehead"), "grad_scale.k_grad_scale", tag + ("dehead",))
            check_scale(c, 0, 2, T("dq"), "grad_scale.k_grad_scale", tag + ("dq",))
            check_scale(c, 0, 3, T("dhead"), "grad_scale_publish.head_bwd", tag + ("dhead",))
    finally:
        c.eng.close()


def test_precision_0_hands_out_no_scale():
    c, _ = run_sup("rcsl")
    assert c.eng.debug_read(0, "gscale").size == 0
    c.eng.close()
