"""GPU: the two kernel families tests/test_gpu_row_kernels.py leaves out -- MCQ's k_vae_latent, k_vae_loss, k_vae_head_bwd,
k_clamp_latent, k_mcq_loss, the ``rep = N`` use of k_assemble and the out-of-distribution use of k_det_action; EDAC's k_edac_gamma and
k_edac_t0 (eta > 0) -- each against its float64 restatement (tests/row_refs.py) ON THE ENGINE'S OWN OPERANDS, read back through
``debug_read`` after one real step, so that the engine's own launch geometry and host dispatch are what is tested.

Bar, for EVERY element of every result and for every metric: |got - f64| <= 4 x the first-order fp32 bound the restatement propagates
through its own arithmetic (proven against the numpy oracle, with planted defects, in tests/test_mcq_edac_refs_cpu.py).  The one
exception is t_0 where the TILED GEMM makes it (A > 8, or a first hidden width that is no multiple of four): that launch rounds its
operands to the engine's precision, and is held to C(precision) x the sum of the absolute values of the same terms, the bar of
tests/test_gpu_backward_f64.py.  k_edac_t0 itself is plain fp32 FMAs in every precision and is held to the factor-4 bar in all three.

Cases (tests/mcq_edac_cases.py), one edge at a time.  MCQ from B = 32, A = 3, obs_dim = 5, Z = 6, N = 3: B 1 / 43 / 129 / 257, A 1 / 4 / 32,
Z 1 / 5 / 7 / 64 (decoder-input rows with and without padding columns: those are asserted zero, the observation columns byte-exact, with
``row / N`` for the out-of-distribution rows), N 1 / 10, max_action 0.5 / 2.5, lambda 0.7 / 1 / 0 (the config check admits both ends),
fixed and learnt temperature, three runs with different nets, data and noise, precision 0 and 1.  Value edges at B = 64, Z = 8: a
constant-head encoder with the raw log-std on, one ulp inside / outside and far beyond both ends of [-4, 15] and means up to +-20;
latents on and beyond +-0.5; all-terminal / no-terminal batches; tied target critics; rewards of 1e3; decoder outputs saturated so
that dm3 is exactly 0.  EDAC from B = 32, A = 3, K = 4, hidden [32, 32], eta = 1: B 1 / 7 / 9 / 33 / 257, A 1 / 7 / 8 (vector) and 9 / 32
(tiled), first hidden width 32 / 256 / 260 / 512 (vector) and 30 (tiled), K 2 / 3, eta 5, three runs, precisions 0 / 1 / 2.  Every case
asserts from the engine (tap ``"edac.t0_path"``) which launch made t_0 and where it took the ReLU mask from: packed bits are reachable
only with a first hidden width that is a multiple of 128 (256, 512 here; both launches are covered with them), the stored activation
everywhere else; the reference's mask is the engine's own (``debug_read_bits("ch0")`` resp. tap ``"ch0"``).  Value edges at B = 64,
A = 6: a member whose first layer is dead (its g is exactly 0: gamma must be finite and inside the bar -- the ``nrm > 0`` guard -- and
its t_0 exactly 0), two members with identical parameters, a member with g rows of 1e-6 resp. 1e3.

Every tap used is live after the step: each workspace is its own allocation and no later launch of either schedule writes ``ehead``,
``vstd``, ``xd``, ``m3``, ``dm3``, ``dxd``, ``dehead``, ``xdo``, ``m3o``, ``qt``, ``qto``, ``q``, ``dq``, ``logp_next`` (MCQ: the backward passes
read their seeds without scaling them in place; the actor phase has its own buffers) or ``g``, ``gamma``, ``tt0``, ``ch0`` (EDAC).  The
critic weights of t_0's reference are the case's own pre-step parameters (the step ends with their Adam update).

Measured worst |err| / bound over the whole module (MI355X; the bar is 4, a correct kernel is expected below 1; the module prints them):
    k_vae_latent       std 0.67, z 0.95
    k_vae_loss         loss 0.07, dm3 0.39
    k_vae_head_bwd     dehead 0.99 (0.9888)
    k_clamp_latent     exact (0); the observation and padding columns of xd / xdo byte-exact
    k_det_action       out-of-distribution actions 0.56
    k_mcq_loss         target_q 0.53, target_ood exact (0), dq 0.61, losses 0.14
    k_edac_gamma       gamma 0.20, TD part + eta L_g of loss/critics 0.09
    k_edac_t0          vector kernel 0.97 in all three precisions; tiled fallback 0.10 of C(precision) x abs-sum
Every figure sits below 1, i.e. inside the first-order bound itself, a factor 4 inside the bar.  t_0 launches seen: both launches with
both mask sources.

The dynamic-scale kernels k_grad_scale / grad_scale_publish of these two schedules are held by tests/test_gpu_headmob_kernels.py (tap ``"gscale"``)."""
import numpy as np
import pytest

import mcq_edac_cases as mc
import row_refs as rr
import test_gpu_row_kernels as rk
from test_gpu_backward_f64 import bound as tiled_bound
from test_gpu_grads import _unpack_bits

pytestmark = pytest.mark.gpu
f32 = np.float32
KEYS = ("vae_", "clamp_latent", "det_action.ood", "mcq_loss", "edac_")
PATHS = set()          # (k_edac_t0 made t_0, the mask came from packed bits) of every EDAC case run


@pytest.fixture(scope="module", autouse=True)
def _figures():
    yield
    print("\nworst |got - f64| / bound per MCQ / EDAC-diversity kernel result:",
          {k: round(v, 4) for k, v in sorted(rk.WORST.items()) if k.startswith(KEYS)})
    print("t_0 launches seen (vector kernel, mask from packed bits):", sorted(PATHS))


holds = rk.holds


# ---------------------------------------------------------------------------------------------------------------------------------
# MCQ
# ---------------------------------------------------------------------------------------------------------------------------------
def check_mcq(c, r, m, pre, tag):
    B, A, od, Z, N, cfg = c.B, c.A, c.od, c.Z, c.N, c.cfg
    T = lambda name: c.eng.debug_read(r, name)
    DP, BN2 = (od + Z + 3) // 4 * 4, 2 * B * N
    b, n = c.batches[r], c.noises[r]
    ma = cfg.max_action
    # ---- k_assemble (rep 1) + k_vae_latent ----
    ehead, vstd, xd = T("ehead").reshape(B, 2 * Z), T("vstd").reshape(B, Z), T("xd").reshape(B, DP)
    std, z = rr.vae_latent(ehead, n["eps_vae"])
    assert np.isfinite(vstd).all() and np.isfinite(xd).all(), tag
    holds(vstd, std, "vae_latent.std", tag)
    holds(xd[:, od:od + Z], z, "vae_latent.z", tag)
    assert xd[:, :od].tobytes() == b["observations"].tobytes() and (xd[:, od + Z:].view(np.uint32) == 0).all(), (tag, "xd obs / padding columns")
    # ---- k_vae_loss ----
    L, dm3 = rr.vae_loss(T("m3").reshape(B, A), b["actions"], ehead, vstd, ma, B, A, Z)
    holds(rk.metric(c, m, r, "loss/behavior_policy"), L, "vae_loss.loss", tag)
    holds(T("dm3").reshape(B, A), dm3, "vae_loss.dm3", tag)
    # ---- k_vae_head_bwd ----
    got = T("dehead").reshape(B, 2 * Z)
    assert np.isfinite(got).all(), tag
    holds(got, rr.vae_head_bwd(T("dxd").reshape(B, Z), ehead, vstd, n["eps_vae"], B, Z), "vae_head_bwd.dehead", tag)
    # ---- k_assemble (rep N) + k_clamp_latent + the OOD k_det_action ----
    xdo = T("xdo").reshape(BN2, DP)
    obs2 = np.concatenate([b["observations"], b["next_observations"]], axis=0)
    assert xdo[:, :od].tobytes() == obs2[np.arange(BN2) // N].tobytes() and (xdo[:, od + Z:].view(np.uint32) == 0).all(), (tag, "xdo obs / padding columns")
    holds(xdo[:, od:od + Z], rr.clamp_latent(n["z_ood"]), "clamp_latent.z", tag)
    sampled = T("sampled_actions").reshape(BN2, A)
    assert (np.abs(sampled) <= f32(ma)).all(), tag
    holds(sampled, rr.det_action(T("m3o").reshape(BN2, A), ma), "det_action.ood", tag)
    # ---- k_mcq_loss (the temperature is the one the step began with: the actor phase follows the critics) ----
    alpha = pre["ALPHA"] if cfg.auto_alpha else cfg.alpha
    q, qt, qto = T("q").reshape(2, 3 * B), T("qt").reshape(2, B), T("qto").reshape(2, BN2)
    assert np.array_equal(q[0, :B], T("q1")) and np.array_equal(q[0, B:], T("q1_ood")), tag
    tq, to = T("target_q"), T("target_ood")
    args = (q, qt, qto, b["rewards"].ravel(), b["terminals"].ravel(), T("logp_next"), alpha, cfg.gamma, cfg.mcq_lambda, B, N)
    y_in, y_ood, _, _ = rr.mcq_loss(*args)
    holds(tq, y_in, "mcq_loss.target_q", tag)
    holds(to, y_ood, "mcq_loss.target_ood", tag)
    _, _, dq, Lc = rr.mcq_loss(*args, stored=(tq, to))
    holds(T("dq").reshape(2, 3 * B), dq, "mcq_loss.dq", tag)
    holds([rk.metric(c, m, r, "loss/critic1"), rk.metric(c, m, r, "loss/critic2")], Lc, "mcq_loss.loss", tag)


MCQ_LAUNCHES = {"vae.assemble", "vae.latent", "vae.loss", "vae.head_bwd", "ood.assemble", "ood.latent", "ood.action", "mcq_loss"}


def run_mcq(**kw):
    c = rk.make("mcq", **mc.mcq_kw(kw))
    try:
        tag = ("mcq", mc.case_id(kw))
        m, pre, _ = rk.step(c)
        assert MCQ_LAUNCHES <= rk.launched(c), sorted(rk.launched(c))
        for r in range(c.R):
            assert np.isfinite(m[r]).all(), (tag, r, m[r])
            check_mcq(c, r, m, pre[r], tag + (r,))
        return c
    except BaseException:
        c.eng.close()
        raise


@pytest.mark.parametrize("kw", mc.MCQ_SHAPES, ids=mc.case_id)
def test_mcq_row_kernels(kw):
    run_mcq(**kw).eng.close()


@pytest.mark.parametrize("kw", mc.MCQ_EDGES, ids=mc.case_id)
def test_mcq_value_edges(kw):
    c = run_mcq(**kw)
    try:
        B, Z, od, name = c.B, c.Z, c.od, kw["mutate"].__name__
        T = lambda nm: c.eng.debug_read(0, nm)
        if name == "constant_head_encoder":
            ehead, deh = T("ehead").reshape(B, 2 * Z), T("dehead").reshape(B, 2 * Z)
            assert np.array_equal(ehead[:, Z:], np.broadcast_to(np.array(mc.LS_TABLE, f32), (B, Z)))
            gated = (ehead[0, Z:] < -4) | (ehead[0, Z:] > 15)
            assert gated.sum() == 4 and (deh[:, Z:][:, gated] == 0).all() and (deh[:, Z:][:, ~gated] != 0).all()
            vstd = T("vstd").reshape(B, Z)
            assert (vstd[:, [1, 6]] == vstd[:, [0]]).all() and (vstd[:, [5, 7]] == vstd[:, [3]]).all(), "beyond a clamp the std is the std at the clamp"
        elif name == "z_ood_on_and_beyond_the_clip":
            zc = T("xdo").reshape(2 * B * c.N, -1)[:16, od:od + Z]
            assert (np.abs(zc) <= 0.5).all() and (zc == 0.5).any() and (zc == -0.5).any() and (np.abs(zc) < 0.5).any()
        elif name == "tied_target_critics":
            qt, qto = T("qt").reshape(2, B), T("qto").reshape(2, -1)
            assert np.array_equal(qt[0], qt[1]) and np.array_equal(qto[0], qto[1])
        elif name == "saturated_decoder":
            assert (T("dm3") == 0).all() and (np.abs(T("sampled_actions")) == 1.0).all()
        elif name == "terminal":
            assert np.array_equal(T("target_q"), c.batches[0]["rewards"].ravel())
    finally:
        c.eng.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# EDAC's gradient-diversity term
# ---------------------------------------------------------------------------------------------------------------------------------
def check_edac_diversity(c, r, m, precision, vec, bits, tag, resolve=True):
    B, A, od, K, cfg = c.B, c.A, c.od, c.K, c.cfg
    N0 = c.hidden[0]
    T = lambda name: c.eng.debug_read(r, name)
    g, gam = T("g").reshape(K, B, A), T("gamma").reshape(K, B, A)
    assert np.isfinite(g).all() and np.isfinite(gam).all(), tag
    # ---- k_edac_gamma on the engine's own g ----
    ref, lg = rr.edac_gamma(g, cfg.eta, K, B)
    holds(gam, ref, "edac_gamma.gamma", tag)
    Ltd, _ = rr.td_loss(T("qs").reshape(K, B), T("target_q"), B)
    total = rr.sum_(Ltd, sequential=True) + lg
    holds(rk.metric(c, m, r, "loss/critics"), total, "edac_gamma.loss", tag)
    if resolve:      # the metric is TD part + eta L_g in one fp32 number: the case must resolve the share -- K for K - 1 moves it by |eta L_g| / K, which
        # has to stand four times clear of the bar (the value edges with Q-values of 1e3 do not, and are not asked to)
        assert abs(lg.v) / K > 4 * rr.FACTOR * total.e, (tag, "the diversity share of loss/critics is not resolved by the bound", lg.v, total.e)
    # ---- t_0 on the engine's own gamma and mask, the case's own first-layer action rows ----
    path = T("edac.t0_path")
    assert (bool(path[0]), bool(path[1])) == (vec, bits), (tag, "t0 launch / mask source", path, (vec, bits))
    PATHS.add((vec, bits))
    mask = _unpack_bits(c.eng.debug_read_bits(r, "ch0"), K, B, N0) if bits else T("ch0").reshape(K, B, N0) > 0
    assert mask.any(), tag
    w0a = c.sts[r]["critics"]["model.0.weight"][:, od:od + A, :]
    tt0 = T("tt0").reshape(K, B, N0)
    assert np.isfinite(tt0).all() and (tt0[~mask] == 0).all(), tag
    if vec:
        holds(tt0, rr.edac_t0(gam, w0a, mask), "edac_t0.vector", tag)
    else:
        t64 = np.einsum("kba,kaj->kbj", gam.astype(np.float64), w0a.astype(np.float64)) * mask
        a64 = np.einsum("kba,kaj->kbj", np.abs(gam).astype(np.float64), np.abs(w0a).astype(np.float64)) * mask
        ratio = float((np.abs(tt0 - t64) / (tiled_bound(precision) * a64 + 1e-30)).max())
        rk.WORST["edac_t0.tiled (C x abs-sum)"] = max(rk.WORST.get("edac_t0.tiled (C x abs-sum)", 0.0), ratio)
        assert ratio < 1.0, (tag, "tiled t0: |err| / (C * abs-sum)", ratio)
    return g, gam, tt0


def run_edac(**kw):
    full = mc.edac_kw(kw)
    vec, bits = mc.edac_expect(full)
    c = rk.make("edac", **full)
    try:
        tag = ("edac", mc.case_id(kw))
        m, _, _ = rk.step(c)
        assert {"edac_gamma", "edac.t0"} <= rk.launched(c), sorted(rk.launched(c))
        out = []
        for r in range(c.R):
            assert np.isfinite(m[r]).all(), (tag, r, m[r])
            out.append(check_edac_diversity(c, r, m, full.get("precision", 0), vec, bits, tag + (r,), resolve="mutate" not in kw))
        return c, out
    except BaseException:
        c.eng.close()
        raise


@pytest.mark.parametrize("kw", mc.EDAC_SHAPES, ids=mc.case_id)
def test_edac_diversity_kernels(kw):
    run_edac(**kw)[0].eng.close()


def test_edac_without_the_diversity_term_reports_no_t0_path():
    c = rk.make("edac", **dict(mc.EDAC_BASE, eta=0.0))
    try:
        rk.step(c)
        assert c.eng.debug_read(0, "edac.t0_path").tolist() == [-1.0, -1.0] and "edac.t0" not in rk.launched(c)
    finally:
        c.eng.close()


@pytest.mark.parametrize("kw", mc.EDAC_EDGES, ids=mc.case_id)
def test_edac_dead_member_twins_and_extreme_gradient_norms(kw):
    c, out = run_edac(**kw)
    try:
        g, gam, tt0 = out[0]
        scale = float(kw["mutate"].__name__.rsplit("_", 1)[1])
        assert (g[0] == 0).all() and np.isfinite(gam[0]).all() and (gam[0] != 0).any(), "the dead member: g exactly 0, gamma finite (the zero-norm guard)"
        assert (tt0[0] == 0).all(), "the dead member's mask is empty: t_0 exactly 0"
        assert np.array_equal(g[1], g[2]) and np.array_equal(gam[1], gam[2]) and np.array_equal(tt0[1], tt0[2]), "identical members"
        nrm = np.sqrt((g[3].astype(np.float64) ** 2).sum(axis=1))
        assert (nrm.max() < 1e-4) if scale < 1 else (nrm.max() > 1e2), (scale, nrm.max())
    finally:
        c.eng.close()
