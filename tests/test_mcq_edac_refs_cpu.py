"""CPU: the MCQ and EDAC-diversity restatements of tests/row_refs.py against the fp32 numpy oracle, before
tests/test_gpu_mcq_edac_kernels.py lets them judge a kernel.

(1) On the inputs of EVERY case of the GPU module (tests/mcq_edac_cases.py: shapes and value edges), the matching intermediates of
oracle/mcq.py and oracle/edac.py must lie inside the restatement's own bound at FACTOR -- the condition that the inputs are fair.  The
element-wise intermediates the oracle does not return come from a copy of its arithmetic (``vae_arith``, ``critic_arith``,
``gamma_arith``, ``t0_arith``), which is first shown to reproduce what the oracle does return bit for bit.
(2) Planted defects, applied to that copy, must exceed the bar -- by orders of magnitude."""
import numpy as np
import pytest

import mcq_edac_cases as mc
import row_refs as rr
import test_gpu_row_kernels as rk
from helpers import clone_state
from oracle import edac as oedac, mcq as omcq, nn
from row_refs import FACTOR

f32 = np.float32


def inside(got, ref, tag):
    r = rr.ratio(got, ref)
    assert r <= FACTOR, (tag, r)
    return r


def beyond(got, ref, tag, by=1e3):
    r = rr.ratio(got, ref)
    assert r > by, (tag, r)


# ---------------------------------------------------------------------------------------------------------------------------------
# copies of the oracle's arithmetic with switchable defects
# ---------------------------------------------------------------------------------------------------------------------------------
def vae_arith(vae, obs, act, eps, ma, defect=None):
    """oracle/mcq.py vae_update, forward and backward up to the encoder head's gradient (fp32)"""
    B, A = act.shape
    od = obs.shape[1]
    x = np.concatenate([obs, act], axis=1).astype(f32)
    eh = nn.mlp_fwd(x, [vae["e1.weight"], vae["e2.weight"]], [vae["e1.bias"], vae["e2.bias"]])
    mean = nn.mm(eh[-1], vae["mean.weight"].T) + vae["mean.bias"]
    ls_raw = nn.mm(eh[-1], vae["log_std.weight"].T) + vae["log_std.bias"]
    std = np.exp(np.clip(ls_raw, omcq.LS_MIN, omcq.LS_MAX))
    z = (mean + std * np.asarray(eps, f32)).astype(f32)
    u, dh, m3 = omcq.vae_decode(vae, obs, z, ma)
    if defect == "recon_without_max_action":
        u = np.tanh(m3).astype(f32)
    Z = mean.shape[1]
    recon = f32(((u - act) ** 2).mean(dtype=f32))
    klt = f32(1) + np.log(std * std) - mean * mean - std * std
    klm = f32(klt.sum(dtype=f32) / f32(B * A)) if defect == "kl_divisor_BA" else f32(klt.mean(dtype=f32))
    loss = f32(recon + f32(-0.5) * klm)
    du = (f32(2) * (u - act) / f32(B * A)).astype(f32)
    t = np.tanh(m3).astype(f32) if defect == "recon_without_max_action" else u / f32(ma)
    dm3 = (du * (f32(1) if defect == "dm3_without_max_action" else f32(ma)) * (f32(1) - t * t)).astype(f32)
    _, _, dy = nn.mlp_bwd(dh, [vae["d1.weight"], vae["d2.weight"]], nn.mm(dm3, vae["d3.weight"]), need_dx=True)
    dz = dy[:, od:]
    dmean = (dz + mean / f32(B * Z)).astype(f32)
    dls = (dz * std * np.asarray(eps, f32) + (std * std - f32(1)) / f32(B * Z)).astype(f32)
    lo = (ls_raw > omcq.LS_MIN) if defect == "gate_strict_at_-4" else (ls_raw >= omcq.LS_MIN)
    hi = (ls_raw < omcq.LS_MAX) if defect == "gate_strict_at_15" else (ls_raw <= omcq.LS_MAX)
    return dict(ehead=np.concatenate([mean, ls_raw], axis=1).astype(f32), std=std.astype(f32), z=z, m3=m3.astype(f32), loss=loss, dm3=dm3,
                dz=np.ascontiguousarray(dz, f32), dmean=dmean, dehead=np.concatenate([dmean, dls * (lo & hi)], axis=1).astype(f32))


def critic_arith(q, qt, qto, rew, term, lpn, alpha, gamma, lam, B, N, defect=None):
    """oracle/mcq.py learn, lines of the critic targets, losses and seeds (fp32).  q [2, 3B], qt [2, B], qto [2, 2BN]"""
    lam = f32(lam)
    nq = np.minimum(qt[0], qt[1]) - f32(alpha) * lpn
    y_in = (rew + f32(gamma) * (f32(1) - term) * nq).astype(f32)
    if defect == "max_over_N_with_stride_N-1":
        o = np.stack([qto[:, j * (N - 1):j * (N - 1) + N] for j in range(2 * B)], axis=1)
    else:
        o = qto.reshape(2, 2 * B, N)
    y_ood = (o.min(axis=2).max(axis=0) if defect == "min_max_swapped" else o.max(axis=2).min(axis=0)).astype(f32)
    w_in, w_ood = (f32(1) - lam, lam) if defect == "lambda_swapped" else (lam, f32(1) - lam)
    div = f32(B if defect == "ood_divisor_B" else 2 * B)
    losses, dqs = [], []
    for c in range(2):
        d_in, d_ood = q[c, :B] - y_in, q[c, B:] - y_ood
        l_in = f32((d_in[:256] ** 2).sum(dtype=f32) / f32(B)) if defect == "rows_from_256_dropped" else f32((d_in ** 2).mean(dtype=f32))
        l_ood = f32((d_ood ** 2).sum(dtype=f32) / div) if defect == "ood_divisor_B" else f32((d_ood ** 2).mean(dtype=f32))
        losses.append(f32(w_in * l_in + w_ood * l_ood))
        dqs.append(np.concatenate([(w_in * f32(2) * d_in / f32(B)).astype(f32), (w_ood * f32(2) * d_ood / div).astype(f32)]))
    return y_in, y_ood, np.stack(dqs), np.array(losses, f32)


def gamma_arith(g, eta, K, B, defect=None):
    """oracle/edac.py learn, lines of the diversity loss and of gamma = d(eta L_g) / dg (fp32).  g [K, B, A]"""
    eta = f32(eta)
    Kd = K if defect == "K_for_K-1" else K - 1
    nrm = np.sqrt((g * g).sum(axis=2, keepdims=True, dtype=f32)).astype(f32)
    nk = nrm + f32(1e-10)
    gh = g / nk
    S = gh.sum(axis=0, keepdims=True, dtype=f32)
    gram_off = (S * S).sum(axis=2, dtype=f32)[0] - (gh * gh).sum(axis=2, dtype=f32).sum(axis=0, dtype=f32)
    mean = f32(gram_off[:256].sum(dtype=f32) / f32(B)) if defect == "rows_from_256_dropped" else gram_off.mean(dtype=f32)
    grad_loss = f32(mean / f32(Kd))
    c = (eta * f32(2.0) / f32(Kd * B)) * (S - gh)
    safe = nrm if defect == "no_zero_norm_guard" else np.where(nrm > 0, nrm, f32(1))
    with np.errstate(invalid="ignore", divide="ignore"):
        gamma = (c / nk - g * ((g * c).sum(axis=2, keepdims=True, dtype=f32) / (nk * nk * safe))).astype(f32)
    return gamma, grad_loss, f32(eta * grad_loss)


def t0_arith(gamma, W0, od, A, mask, defect=None):
    """oracle/edac.py learn: t = (gamma W_0[action rows]) (.) m_0 (fp32).  W0 [K, od + A, N0], mask [K, B, N0]"""
    rows = W0[:, :A, :] if defect == "first_A_rows" else W0[:, od:od + A, :]
    if defect == "mask_of_the_next_member":
        mask = np.roll(mask, 1, axis=0)
    return (oedac._bmm(gamma, rows) * mask).astype(f32)


# ---------------------------------------------------------------------------------------------------------------------------------
# the oracle on a case's inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def mcq_oracle(c, r, kw):
    """one oracle step of run r: the oracle's results and, recomputed from the pre-step nets as the oracle does, the operands of the
    critic loss"""
    st = clone_state({k: c.sts[r][k] for k in ("actor", "critic1", "critic2", "critic1_old", "critic2_old", "behavior_policy")})
    pre = clone_state(st)
    st["log_alpha"] = np.array([-0.3], f32)
    cfg = omcq.default_cfg(c.od, c.A)
    cfg.update(hidden=c.hidden, vae_hidden=c.vae_hidden, latent_dim=c.Z, num_sampled_actions=c.N, lmbda=kw.get("mcq_lambda", 0.9),
               max_action=kw.get("max_action", 1.0), auto_alpha=bool(kw.get("auto_alpha", 1)), alpha=kw.get("alpha", 0.2))
    omcq.init_opt(st)
    b, n = c.batches[r], c.noises[r]
    res, aux = omcq.learn(st, cfg, b, n)
    obs, act, nobs = b["observations"], b["actions"], b["next_observations"]
    alpha = f32(np.exp(f32(-0.3))) if cfg["auto_alpha"] else f32(cfg["alpha"])
    na, nlogp, _ = nn.tanh_gauss_fwd(pre["actor"], nobs, n["eps_next"])
    s_in = np.concatenate([obs, nobs], axis=0)
    s_rep = np.repeat(s_in, c.N, axis=0)
    a_ood, _, _ = nn.tanh_gauss_fwd(pre["actor"], s_in, n["eps_ood"])
    qt = np.stack([nn.critic_fwd(pre[k], nobs, na)[0].ravel() for k in ("critic1_old", "critic2_old")])
    qto = np.stack([nn.critic_fwd(pre[k], s_rep, aux["sampled_actions"])[0].ravel() for k in ("critic1_old", "critic2_old")])
    q = np.stack([np.concatenate([nn.critic_fwd(pre[k], obs, act)[0].ravel(), nn.critic_fwd(pre[k], s_in, a_ood)[0].ravel()]) for k in ("critic1", "critic2")])
    ops = (q, qt, qto, b["rewards"].ravel(), b["terminals"].ravel(), nlogp.ravel(), alpha, cfg["gamma"], cfg["lmbda"], c.B, c.N)
    return cfg, pre, res, aux, ops


def check_mcq_case(kw):
    c = rk.inputs("mcq", **mc.mcq_kw(kw))
    B, A, Z = c.B, c.A, c.Z
    for r in range(c.R):
        cfg, pre, res, aux, ops = mcq_oracle(c, r, kw)
        b, n = c.batches[r], c.noises[r]
        ma = cfg["max_action"]
        v = vae_arith(pre["behavior_policy"], b["observations"], b["actions"], n["eps_vae"], ma)
        # the copy is the oracle's arithmetic: its loss, and the bias gradients that are plain sums of its element-wise results
        assert v["loss"] == f32(res["loss/behavior_policy"]), (kw, v["loss"], res["loss/behavior_policy"])
        g = aux["vae_grads"]
        assert np.array_equal(g["d3.bias"], v["dm3"].sum(axis=0, dtype=f32)) and np.array_equal(g["mean.bias"], v["dmean"].sum(axis=0, dtype=f32))
        assert np.array_equal(g["log_std.bias"], v["dehead"][:, Z:].sum(axis=0, dtype=f32))
        tag = ("mcq", mc.case_id(kw), r)
        std, z = rr.vae_latent(v["ehead"], n["eps_vae"])
        inside(v["std"], std, tag + ("std",)); inside(v["z"], z, tag + ("z",))
        L, dm3 = rr.vae_loss(v["m3"], b["actions"], v["ehead"], v["std"], ma, B, A, Z)
        inside(v["loss"], L, tag + ("vae loss",)); inside(v["dm3"], dm3, tag + ("dm3",))
        inside(v["dehead"], rr.vae_head_bwd(v["dz"], v["ehead"], v["std"], n["eps_vae"], B, Z), tag + ("dehead",))
        assert np.array_equal(rr.clamp_latent(n["z_ood"]).v, np.clip(n["z_ood"], f32(-0.5), f32(0.5)))
        y_in, y_ood, dq, Lc = critic_arith(*ops)
        assert np.array_equal(y_in, aux["target_q"].ravel()) and np.array_equal(y_ood, aux["target_q_ood"].ravel())
        assert Lc[0] == f32(res["loss/critic1"]) and Lc[1] == f32(res["loss/critic2"])
        ry_in, ry_ood, _, _ = rr.mcq_loss(*ops)
        inside(y_in, ry_in, tag + ("target_q",)); inside(y_ood, ry_ood, tag + ("target_ood",))
        _, _, rdq, rL = rr.mcq_loss(*ops, stored=(y_in, y_ood))
        inside(dq, rdq, tag + ("dq",)); inside(Lc, rL, tag + ("critic losses",))
        inside(aux["critic1_grads"]["last.bias"], rr.sum_(rdq[0, :B]) + rr.sum_(rdq[0, B:]), tag + ("sum dq",))
    return c


@pytest.mark.parametrize("kw", mc.MCQ_SHAPES + mc.MCQ_EDGES, ids=mc.case_id)
def test_mcq_oracle_is_inside_the_bounds_on_the_gpu_cases(kw):
    check_mcq_case(kw)


def test_oracle_mcq_honours_max_action():
    """every existing MCQ case has max_action = 1: the oracle must scale the reconstruction, its gradient and the decoded actions"""
    c = rk.inputs("mcq", **mc.mcq_kw(dict(max_action=2.5)))
    out = {ma: mcq_oracle(c, 0, dict(max_action=ma)) for ma in (1.0, 2.5)}
    s1, s25 = out[1.0][3]["sampled_actions"], out[2.5][3]["sampled_actions"]
    assert 2.0 < np.abs(s25).max() / np.abs(s1).max() < 3.0      # (the two decoders differ by one Adam step of 1e-3: the factor is 2.5 up to that)
    assert out[1.0][2]["loss/behavior_policy"] != out[2.5][2]["loss/behavior_policy"]
    assert not np.array_equal(out[1.0][3]["vae_grads"]["d3.bias"], out[2.5][3]["vae_grads"]["d3.bias"])


def edac_oracle(c, r, kw):
    st = clone_state({k: c.sts[r][k] for k in ("actor", "critics", "critics_old")})
    pre = clone_state(st)
    st["log_alpha"] = np.array([-0.3], f32)
    cfg = oedac.default_cfg(c.od, c.A)
    cfg.update(hidden=c.hidden, num_critics=c.K, eta=kw.get("eta", 1.0))
    oedac.init_opt(st)
    res, aux = oedac.learn(st, cfg, c.batches[r], c.noises[r])
    return cfg, pre, res, aux


def check_edac_case(kw):
    full = mc.edac_kw(kw)
    c = rk.inputs("edac", **full)
    K, B, A, od = c.K, c.B, c.A, c.od
    for r in range(c.R):
        cfg, pre, res, aux = edac_oracle(c, r, full)
        g = aux["g"]
        gamma, grad_loss, lg = gamma_arith(g, cfg["eta"], K, B)
        assert grad_loss == aux["grad_loss"], (kw, grad_loss, aux["grad_loss"])
        tag = ("edac", mc.case_id(kw), r)
        assert np.isfinite(gamma).all(), tag
        rgam, rlg = rr.edac_gamma(g, cfg["eta"], K, B)
        inside(gamma, rgam, tag + ("gamma",)); inside(lg, rlg, tag + ("eta L_g",))
        x = np.concatenate([c.batches[r]["observations"], c.batches[r]["actions"]], axis=1)
        mask = oedac.ens_fwd(pre["critics"], x)[1][1] > 0
        W0 = pre["critics"]["model.0.weight"]
        inside(t0_arith(gamma, W0, od, A, mask), rr.edac_t0(gamma, W0[:, od:od + A, :], mask), tag + ("t0",))
    return c


@pytest.mark.parametrize("kw", mc.EDAC_SHAPES + mc.EDAC_EDGES, ids=mc.case_id)
def test_edac_oracle_is_inside_the_bounds_on_the_gpu_cases(kw):
    check_edac_case(kw)


def test_edac_dispatch_expectations_of_the_cases():
    """the cases reach both t_0 launches, and the vector launch at every edge the issue names"""
    ex = {mc.case_id(kw): mc.edac_expect(mc.edac_kw(kw)) for kw in mc.EDAC_SHAPES}
    assert ex["A8"][0] and not ex["A9"][0] and not ex["A32"][0] and not ex["hidden(30, 32)"][0]
    assert ex["hidden(260, 32)"] == (True, False) and ex["hidden(256, 32)"] == (True, True) and ex["hidden(256, 32)-A9"] == (False, True)


# ---------------------------------------------------------------------------------------------------------------------------------
# planted defects
# ---------------------------------------------------------------------------------------------------------------------------------
def test_planted_vae_defects_are_beyond_the_bar():
    c = rk.inputs("mcq", **mc.mcq_kw(dict(B=64, Z=8, mutate=mc.constant_head_encoder)))
    b, n, vae = c.batches[0], c.noises[0], c.sts[0]["behavior_policy"]
    B, A, Z = c.B, c.A, c.Z
    run = lambda ma, defect=None: vae_arith(vae, b["observations"], b["actions"], n["eps_vae"], ma, defect)
    good = run(2.5)
    L, dm3 = rr.vae_loss(good["m3"], b["actions"], good["ehead"], good["std"], 2.5, B, A, Z)
    deh = rr.vae_head_bwd(good["dz"], good["ehead"], good["std"], n["eps_vae"], B, Z)
    inside(good["dm3"], dm3, "dm3"); inside(good["loss"], L, "loss"); inside(good["dehead"], deh, "dehead")
    beyond(run(2.5, "dm3_without_max_action")["dm3"], dm3, "max_action dropped from dm3")
    beyond(run(2.5, "recon_without_max_action")["dm3"], dm3, "max_action dropped from the reconstruction (dm3)")
    for d in ("gate_strict_at_15", "gate_strict_at_-4"):      # the column whose raw log-std sits exactly on the clamp loses its gradient: err / 0-free bound
        bad = run(2.5, d)["dehead"]
        col = Z + mc.LS_TABLE.index(15.0 if d.endswith("15") else -4.0)
        assert (bad[:, col] == 0).all() and (good["dehead"][:, col] != 0).all()
        beyond(bad, deh, d)
    # the loss: on an encoder whose std stays moderate (at exp(15) the KL term is 1e13 and hides the reconstruction)
    c = rk.inputs("mcq", **mc.mcq_kw(dict(B=43)))
    b, n, vae = c.batches[0], c.noises[0], c.sts[0]["behavior_policy"]
    run = lambda ma, defect=None: vae_arith(vae, b["observations"], b["actions"], n["eps_vae"], ma, defect)
    good = run(2.5)
    L, _ = rr.vae_loss(good["m3"], b["actions"], good["ehead"], good["std"], 2.5, c.B, c.A, c.Z)
    inside(good["loss"], L, "loss")
    beyond(run(2.5, "recon_without_max_action")["loss"], L, "max_action dropped from the reconstruction (loss)")
    beyond(run(2.5, "kl_divisor_BA")["loss"], L, "KL divisor B A")


def test_planted_mcq_loss_defects_are_beyond_the_bar():
    kw = dict(B=300, mcq_lambda=0.7)
    c = rk.inputs("mcq", **mc.mcq_kw(kw))
    ops = mcq_oracle(c, 0, kw)[4]
    y_in, y_ood, dq, Lc = critic_arith(*ops)
    ry_in, ry_ood, _, _ = rr.mcq_loss(*ops)
    _, _, rdq, rL = rr.mcq_loss(*ops, stored=(y_in, y_ood))
    inside(y_ood, ry_ood, "y_ood"); inside(dq, rdq, "dq"); inside(Lc, rL, "L")
    for d in ("max_over_N_with_stride_N-1", "min_max_swapped"):
        beyond(critic_arith(*ops, defect=d)[1], ry_ood, d)
    for d in ("ood_divisor_B", "lambda_swapped"):
        bad = critic_arith(*ops, defect=d)
        beyond(bad[2], rdq, d + " (dq)"); beyond(bad[3], rL, d + " (loss)")
    beyond(critic_arith(*ops, defect="rows_from_256_dropped")[3], rL, "rows >= 256 dropped from the strided sum")


def test_planted_edac_defects_are_beyond_the_bar():
    full = mc.edac_kw(dict(B=300, mutate=mc.dead_member_and_twins(1e4)))
    c = rk.inputs("edac", **full)
    cfg, pre, res, aux = edac_oracle(c, 0, full)
    K, B, A, od = c.K, c.B, c.A, c.od
    g = aux["g"]
    assert (g[0] == 0).all()
    gamma, _, lg = gamma_arith(g, 1.0, K, B)
    rgam, rlg = rr.edac_gamma(g, 1.0, K, B)
    inside(gamma, rgam, "gamma"); inside(lg, rlg, "lg")
    assert np.isfinite(rgam.v).all() and np.isfinite(rgam.e).all()
    bad = gamma_arith(g, 1.0, K, B, "no_zero_norm_guard")[0]
    assert np.isnan(bad[0]).all() and rr.ratio(bad, rgam) == np.inf                         # 0 / 0 on the dead member
    bad = gamma_arith(g, 1.0, K, B, "K_for_K-1")
    beyond(bad[0], rgam, "K for K - 1 (gamma)"); beyond(bad[2], rlg, "K for K - 1 (loss)")
    beyond(gamma_arith(g, 1.0, K, B, "rows_from_256_dropped")[2], rlg, "rows >= 256 dropped")
    x = np.concatenate([c.batches[0]["observations"], c.batches[0]["actions"]], axis=1)
    mask = oedac.ens_fwd(pre["critics"], x)[1][1] > 0
    W0 = pre["critics"]["model.0.weight"]
    rt = rr.edac_t0(gamma, W0[:, od:od + A, :], mask)
    inside(t0_arith(gamma, W0, od, A, mask), rt, "t0")
    assert (rt.v[0] == 0).all() and (rt.e[0] == 0).all()                                     # the dead member: an empty mask admits nothing but 0
    beyond(t0_arith(gamma, W0, od, A, mask, "mask_of_the_next_member"), rt, "mask of another member")
    beyond(t0_arith(gamma, W0, od, A, mask, "first_A_rows"), rt, "first A rows of W0 instead of the action rows")
