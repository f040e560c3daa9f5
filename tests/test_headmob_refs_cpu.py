"""CPU: the supervised-head, MOBILE and dynamic-scale restatements of tests/row_refs.py, proven before
tests/test_gpu_headmob_kernels.py lets them judge a kernel.  On the inputs of EVERY case of the GPU module (tests/headmob_cases.py):

(1) each restatement's value equals float64 torch autograd of the reference's formula on the same fp32 operands (equal up to float64
    rounding: 1e-11 relative of the result's scale -- a check of the algebra, not a bar on any kernel);
(2) the fp32 numpy oracles (tests/rcsl_oracle.py, rcsl_gauss_oracle.py, autoreg_oracle.py, mobile_oracle.py) lie inside the restatement's
    own bound at FACTOR -- the condition that the inputs are fair.  The element-wise intermediates an oracle does not return come from a
    copy of its arithmetic (``rcsl_arith``, ``gauss_arith``, ``autoreg_arith``, ``lcb_arith``, ``td_arith``: plain fp32 numpy), which is
    first shown to reproduce what the oracle does return bit for bit;
(3) planted defects, applied to that copy, exceed the bar."""
import math

import numpy as np
import pytest
import torch

import autoreg_oracle as aorc
import headmob_cases as hc
import mobile_oracle as morc
import rcsl_gauss_oracle as gorc
import rcsl_oracle as rorc
import row_refs as rr
from oracle import nn
from row_refs import FACTOR

f32 = np.float32
T64 = lambda a, grad=False: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


def inside(got, ref, tag):
    r = rr.ratio(got, ref)
    assert r <= FACTOR, (tag, r)
    return r


def beyond(got, ref, tag):
    r = rr.ratio(got, ref)
    assert r > FACTOR, (tag, r)
    return r


def same(ref, t, tag):
    """a restatement's value against float64 autograd: equal up to float64 rounding"""
    a = np.asarray(ref.v if isinstance(ref, rr.BV) else ref, np.float64)
    b = np.asarray(t.detach().numpy() if torch.is_tensor(t) else t, np.float64).reshape(a.shape)
    assert np.abs(a - b).max(initial=0.0) <= 1e-11 * max(1e-30, np.abs(b).max(initial=0.0)), (tag, np.abs(a - b).max(), np.abs(b).max())


# ---------------------------------------------------------------------------------------------------------------------------------
# RCSL
# ---------------------------------------------------------------------------------------------------------------------------------
def rcsl_arith(pred, act, valid, defect=None):
    """tests/rcsl_oracle.py learn: loss and seed (fp32)"""
    B, A = act.shape
    d = np.where(valid[:, None], pred - act, f32(0)).astype(f32)
    cnt = f32(B * A) if defect == "divisor_BA" else f32(int(valid.sum()) * A)
    return f32((d * d).sum(dtype=f32) / cnt), (f32(2) * d / cnt).astype(f32)


def check_rcsl_case(kw):
    c = hc.inputs("rcsl", **kw)
    for r in range(c.R):
        b, v = c.batches[r], c.valid[r]
        res, aux = rorc.learn(rorc.init_state(c.nets[r]), dict(lr=3e-4), b, v)
        pred, act = aux["pred"], b["actions"]
        L, dp = rcsl_arith(pred, act, v)
        assert L == f32(res["loss"]) and np.array_equal(dp, aux["dpred"]), kw
        tag = ("rcsl", hc.case_id(kw), r)
        rL, rdp = rr.rcsl_loss(pred, act, v)
        p = T64(pred, True)
        loss = ((p - T64(act)) ** 2)[torch.tensor(v)].mean()
        loss.backward()
        same(rL, loss, tag + ("loss",)); same(rdp, p.grad, tag + ("dpred",))
        inside(L, rL, tag + ("loss",)); inside(dp, rdp, tag + ("dpred",))
        assert (rdp.v[~v] == 0).all() and (rdp.e[~v] == 0).all()


@pytest.mark.parametrize("kw", hc.RCSL_SHAPES + [dict(mutate=hc.zero_seed_rcsl)], ids=hc.case_id)
def test_rcsl_loss_restatement_on_the_gpu_cases(kw):
    check_rcsl_case(kw)


# ---------------------------------------------------------------------------------------------------------------------------------
# Gaussian RCSL
# ---------------------------------------------------------------------------------------------------------------------------------
def gauss_arith(net, z, act, valid, defect=None):
    """tests/rcsl_gauss_oracle.py learn behind the latent: heads, loss, seeds, head gradients (fp32)"""
    B, A = act.shape
    v = valid[:, None]
    mu = (nn.mm(z, net["dist_net.mu.weight"].T) + net["dist_net.mu.bias"]).astype(f32)
    raw = (nn.mm(z, net["dist_net.sigma.weight"].T) + net["dist_net.sigma.bias"]).astype(f32)
    s = np.clip(raw, gorc.LO, gorc.HI).astype(f32)
    cnt = f32(B * A) if defect == "divisor_BA" else f32(int(valid.sum()) * A)
    d = np.where(v, mu - act, f32(0)).astype(f32)
    iv = np.exp(-s).astype(f32)
    q = (d * d * iv).astype(f32)
    loss = f32(q.sum(dtype=f32) / cnt + np.where(v, s, f32(0)).sum(dtype=f32) / cnt)
    dmu = (f32(2) * d * iv / cnt).astype(f32)
    is_open = ((raw > gorc.LO) & (raw < gorc.HI)) if defect == "exclusive_gate" else ((raw >= gorc.LO) & (raw <= gorc.HI))
    ds = np.where(v & is_open, (f32(1) - q) / cnt, f32(0)).astype(f32)
    keep = np.ones(B, bool)
    if defect == "chunk_last_row_dropped":
        keep[63] = False
    g = {"dist_net.mu.weight": nn.mm(dmu[keep].T, z[keep]), "dist_net.mu.bias": dmu[keep].sum(axis=0, dtype=f32),
         "dist_net.sigma.weight": nn.mm(ds[keep].T, z[keep]), "dist_net.sigma.bias": ds[keep].sum(axis=0, dtype=f32)}
    dz = (nn.mm(dmu, net["dist_net.mu.weight"]) + nn.mm(ds, net["dist_net.sigma.weight"])).astype(f32)
    return dict(mu=mu, raw=raw, logvar=s, loss=loss, dmu=dmu, ds=ds, dz=dz, grads=g)


def gauss_autograd(net, z, act, valid):
    zt = T64(z, True)
    h = {k: T64(net[k], True) for k in rr.RG_HEAD}
    mu = zt @ h["dist_net.mu.weight"].T + h["dist_net.mu.bias"]
    raw = zt @ h["dist_net.sigma.weight"].T + h["dist_net.sigma.bias"]
    mu.retain_grad(); raw.retain_grad()
    s = torch.clamp(raw, rr.RG_LO, rr.RG_HI)
    vt = torch.tensor(valid)
    loss = (((mu - T64(act)) ** 2) * torch.exp(-s))[vt].mean() + s[vt].mean()
    loss.backward()
    return dict(mu=mu, logvar=s, loss=loss, dmu=mu.grad, ds=raw.grad, dz=zt.grad, grads={k: h[k].grad for k in rr.RG_HEAD})


def gauss_operands(c, r):
    b, v, net = c.batches[r], c.valid[r], c.nets[r]
    res, aux = gorc.learn(gorc.init_state(net), dict(lr=3e-4), b, v)
    return b, v, net, res, aux


def check_gauss_case(kw):
    c = hc.inputs("rcslg", **kw)
    for r in range(c.R):
        b, v, net, res, aux = gauss_operands(c, r)
        z, act = aux["z"], b["actions"]
        a = gauss_arith(net, z, act, v)
        assert a["loss"] == f32(res["loss"]) and np.array_equal(a["dz"], aux["dz"]) and np.array_equal(a["mu"], aux["mu"]), kw
        assert all(np.array_equal(a["grads"][k], aux["grads"][k]) for k in rr.RG_HEAD), kw
        tag = ("rcslg", hc.case_id(kw), r)
        ref = rr.rcslg_head(z, act, net, v, raw32=a["raw"])
        t = gauss_autograd(net, z, act, v)
        for k in ("mu", "logvar", "loss", "dmu", "ds", "dz"):
            same(ref[k], t[k], tag + (k,))
            inside(a[k], ref[k], tag + (k,))
        for k in rr.RG_HEAD:
            same(ref["grads"][k], t["grads"][k], tag + (k,))
            inside(a["grads"][k], ref["grads"][k], tag + (k,))
        # the gate the GPU module has to take from the clamped value alone is the gate of the raw value
        assert np.array_equal(rr.rcslg_head(z, act, net, v, logvar32=a["logvar"])["gate"], ref["gate"]), tag
        for k in ("dmu", "ds", "dz"):
            assert (ref[k].v[~v] == 0).all() and (ref[k].e[~v] == 0).all(), tag
    return c


@pytest.mark.parametrize("kw", hc.RCSLG_SHAPES + hc.RCSLG_EDGES + [dict(mutate=hc.zero_seed_rcslg)], ids=hc.case_id)
def test_rcslg_head_restatement_on_the_gpu_cases(kw):
    c = check_gauss_case(kw)
    if kw.get("mutate") is hc.constant_sigma_head:
        b, v, net, res, aux = gauss_operands(c, 0)
        ref = rr.rcslg_head(aux["z"], b["actions"], net, v, raw32=aux["raw"])
        lv = np.array([hc.LV_TABLE[j % 9] for j in range(c.A)], f32)
        shut = (lv < -5) | (lv > 2)
        assert shut.sum() == 8 and (ref["ds"].v[:, shut] == 0).all() and (ref["ds"].e[:, shut] == 0).all() and (ref["ds"].v[:, ~shut] != 0).all()
        assert np.array_equal(ref["logvar"].v, np.broadcast_to(np.clip(lv, f32(-5), f32(2)).astype(np.float64), (c.B, c.A)))
        assert np.abs(ref["mu"].v - b["actions"]).max() > 19.0


# ---------------------------------------------------------------------------------------------------------------------------------
# the autoregressive head and draw
# ---------------------------------------------------------------------------------------------------------------------------------
def autoreg_arith(z, t, valid, A, defect=None):
    """tests/autoreg_oracle.py learn behind the tail pre-activation: out, loss, dz_tail (fp32)"""
    M = z.shape[0]
    B = M // A
    v = valid[np.arange(M) // A] if defect == "pad_by_m_over_A" else np.tile(valid, A)
    out = aorc.leaky(z)
    mean, ls = out[:, 0], out[:, 1]
    cnt = f32(int(valid.sum()) * A)
    inv_std = np.exp(-ls).astype(f32)
    d = ((t - mean) * inv_std).astype(f32)
    nll = (ls + f32(0.5) * d * d + aorc.HALF_LOG_2PI).astype(f32)
    loss = f32(np.where(v, nll, f32(0)).sum(dtype=f32) / cnt)
    dout = np.stack([np.where(v, -d * inv_std / cnt, f32(0)), np.where(v, (f32(1) - d * d) / cnt, f32(0))], axis=1).astype(f32)
    slope = f32(1) if defect == "slope_1" else aorc.SLOPE
    return out, loss, (dout * np.where(out > 0, f32(1), slope)).astype(f32)


def autoreg_operands(c, r):
    b, v = c.batches[r], c.valid[r]
    res, aux = aorc.learn(aorc.init_state(c.nets[r]), dict(lr=3e-4), b, v)
    return v, res, aux


def check_autoreg_case(kw):
    c = hc.inputs("autoreg", **kw)
    A = c.A
    for r in range(c.R):
        v, res, aux = autoreg_operands(c, r)
        z, t = aux["z_tail"], aux["target"]
        out, L, dz = autoreg_arith(z, t, v, A)
        assert L == f32(res["loss"]) and np.array_equal(out, aux["out"]) and np.array_equal(dz, aux["dz_tail"]), kw
        tag = ("autoreg", hc.case_id(kw), r)
        rout, rL, rdz = rr.autoreg_head(z, t, A, v)
        zt = T64(z, True)
        # (the reference's slope is the Python double 0.01; the fp32 kernels and oracle hold fp32(0.01): the restatement takes the latter)
        o = torch.where(zt > 0, zt, T64(f32(rr.LEAKY_SLOPE)) * zt)
        vm = torch.tensor(np.tile(v, A))
        loss = (o[:, 1] + 0.5 * ((T64(t) - o[:, 0]) * torch.exp(-o[:, 1])) ** 2 + rr.HALF_LOG_2PI)[vm].mean()
        loss.backward()
        same(rout, o, tag + ("out",)); same(rL, loss, tag + ("loss",)); same(rdz, zt.grad, tag + ("dz",))
        inside(out, rout, tag + ("out",)); inside(L, rL, tag + ("loss",)); inside(dz, rdz, tag + ("dz",))
        pad_m = ~np.tile(v, A)
        assert (rdz.v[pad_m] == 0).all() and (rdz.e[pad_m] == 0).all() and (rdz.v[~pad_m] != 0).any(axis=1).all(), tag
    return c


@pytest.mark.parametrize("kw", hc.AUTOREG_SHAPES + hc.AUTOREG_EDGES, ids=hc.case_id)
def test_autoreg_head_restatement_on_the_gpu_cases(kw):
    check_autoreg_case(kw)


def test_leaky_backward_at_exactly_zero_takes_the_slope_branch_as_torch_does():
    z = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.leaky_relu(z, 0.01).sum().backward()
    val, slope = rr.leaky(np.zeros(3, f32))
    assert (z.grad.numpy() == 0.01).all() and (slope.v == float(f32(0.01))).all() and (val.v == 0).all()


@pytest.mark.parametrize("kw", hc.DRAW_SHAPES, ids=hc.case_id)
def test_autoreg_draw_restatement_on_the_gpu_cases(kw):
    c = hc.draw_inputs(**kw)
    A, od, n = c.A, c.od, c.n
    for r in range(c.R):
        act = aorc.sample(c.nets[r], c.sobs[r], c.seps[r])
        # the last pass: its input holds a_<(A - 1) and the one-hot of A - 1
        x = np.concatenate([c.sobs[r], act, np.tile(np.eye(A, dtype=f32)[A - 1], (n, 1))], axis=1)
        x[:, od + A - 1] = 0
        zs = aorc.forward_rows(c.nets[r], x)[1][-1]
        got = (aorc.leaky(zs)[:, 0] + np.exp(aorc.leaky(zs)[:, 1]).astype(f32) * c.seps[r][:, A - 1]).astype(f32)
        assert np.array_equal(got, act[:, A - 1]), kw                  # the copy is the oracle's arithmetic
        ref = rr.autoreg_draw(zs, c.seps[r][:, A - 1])
        z64 = T64(zs)
        o = torch.where(z64 > 0, z64, T64(f32(rr.LEAKY_SLOPE)) * z64)
        same(ref, o[:, 0] + torch.exp(o[:, 1]) * T64(c.seps[r][:, A - 1]), ("draw", hc.case_id(kw), r))
        inside(got, ref, ("draw", hc.case_id(kw), r))


# ---------------------------------------------------------------------------------------------------------------------------------
# MOBILE
# ---------------------------------------------------------------------------------------------------------------------------------
def lcb_arith(ql, B, S, E, real_rows, defect=None):
    """tests/mobile_oracle.py lcb_from_samples behind the critics + the real-row mask of learn (fp32; the std in float64 as there)"""
    qmin = np.minimum(ql[0], ql[1]).astype(f32)
    q4 = qmin.reshape(S, E, B)
    m = q4[0] if defect == "no_mean_over_S" else q4.mean(axis=0, dtype=f32)
    pen = m.astype(np.float64).std(axis=0, ddof=0 if defect == "biased_std" else 1).astype(f32)
    pen[:real_rows] = 0
    return qmin, pen


def td_arith(q, qt, rew, term, pen, logp_next, alpha, gamma, coef, B, det, defect=None):
    """tests/mobile_oracle.py learn, the lines of the target, the loss and the seeds (fp32)"""
    next_q = np.minimum(qt[0], qt[1]).astype(f32)
    if not det:
        next_q = (next_q - (f32(alpha) * logp_next).astype(f32)).astype(f32)
    rp = (rew - (f32(coef) * pen).astype(f32)).astype(f32)
    raw = (rp + ((f32(gamma) * (f32(1) - term)).astype(f32) * next_q).astype(f32)).astype(f32)
    y = raw if defect == "y_unclamped" else np.where(raw < 0, f32(0), raw).astype(f32)
    loss = f32(((q - y[None]) ** 2).mean(dtype=f32))
    div = f32(B if defect == "dq_over_B" else 2 * B)
    return y, loss, (f32(2) * (q - y[None]) / div).astype(f32)


def mobile_operands(c, r, kw):
    """the oracle's penalty pass and the operands of the critic loss, from the case's pre-step nets"""
    st, b, n = c.sts[r], c.batches[r], c.noises[r]
    S, E, B, od = c.S, c.E, c.B, c.od
    smp = c.samples[r]
    pen_o, qmin_o = morc.lcb_from_samples(st, smp.reshape(S, E, B, od), n["eps_lcb"])
    a, _, _ = nn.tanh_gauss_fwd(st["actor"], smp, n["eps_lcb"])
    ql = np.stack([nn.critic_fwd(st[k], smp, a)[0].ravel() for k in ("critic1_old", "critic2_old")])
    na, nlogp, _ = nn.tanh_gauss_fwd(st["actor"], b["next_observations"], n["eps_next"])
    qt = np.stack([nn.critic_fwd(st[k], b["next_observations"], na)[0].ravel() for k in ("critic1_old", "critic2_old")])
    q = np.stack([nn.critic_fwd(st[k], b["observations"], b["actions"])[0].ravel() for k in ("critic1", "critic2")])
    alpha = f32(kw.get("alpha", 0.2)) if not kw.get("auto_alpha", 1) else f32(np.exp(st["log_alpha"][0]))
    return dict(pen_o=pen_o.ravel(), qmin_o=qmin_o.ravel(), ql=ql, qt=qt, q=q, logp_next=nlogp.ravel(), alpha=alpha,
                rew=b["rewards"].ravel(), term=b["terminals"].ravel(), det=bool(kw.get("deterministic_backup", 0)),
                coef=kw.get("penalty_coef", 1.0), gamma=0.99)


def check_mobile_case(kw):
    c = hc.mobile_inputs(**kw)
    S, E, B = c.S, c.E, c.B
    for r in range(c.R):
        o = mobile_operands(c, r, kw)
        tag = ("mobile", hc.case_id(kw), r)
        qmin, pen = lcb_arith(o["ql"], B, S, E, c.real_rows)
        unmasked = lcb_arith(o["ql"], B, S, E, 0)[1]
        assert np.array_equal(qmin, o["qmin_o"]) and np.array_equal(unmasked, o["pen_o"]), kw
        rq, rpen = rr.lcb_penalty(o["ql"], B, S, E, c.real_rows)
        assert np.array_equal(rq, qmin), tag
        tq = torch.minimum(T64(o["ql"][0]), T64(o["ql"][1])).reshape(S, E, B).mean(0).std(0)
        tq[:c.real_rows] = 0
        same(rpen, tq, tag + ("penalty",)); inside(pen, rpen, tag + ("penalty",))
        assert (rpen.v[:c.real_rows] == 0).all() and (rpen.e[:c.real_rows] == 0).all()
        lp = None if o["det"] else o["logp_next"]
        args = (o["q"], o["qt"], o["rew"], o["term"], pen, o["gamma"], o["coef"], B)
        ry, _, _ = rr.mobile_td_loss(*args, logp_next=lp, alpha=o["alpha"])
        y, L, dq = td_arith(o["q"], o["qt"], o["rew"], o["term"], pen, o["logp_next"], o["alpha"], o["gamma"], o["coef"], B, o["det"])
        _, rL, rdq = rr.mobile_td_loss(*args, logp_next=lp, alpha=o["alpha"], stored=y)
        qv = T64(o["q"], True)
        nq = torch.minimum(T64(o["qt"][0]), T64(o["qt"][1]))
        if lp is not None:
            nq = nq - float(o["alpha"]) * T64(lp)
        ty = torch.clamp((T64(o["rew"]) - float(f32(o["coef"])) * T64(pen)) + float(f32(o["gamma"])) * (1.0 - T64(o["term"])) * nq, min=0.0)
        same(ry, ty, tag + ("y",))
        loss = ((qv - T64(y)) ** 2).mean()
        loss.backward()
        same(rL, loss, tag + ("loss",)); same(rdq, qv.grad, tag + ("dq",))
        inside(y, ry, tag + ("y",)); inside(L, rL, tag + ("loss",)); inside(dq, rdq, tag + ("dq",))
    return c


@pytest.mark.parametrize("kw", hc.MOBILE_SHAPES + hc.MOBILE_EDGES + [hc.ZERO_SEED_MOBILE], ids=hc.case_id)
def test_mobile_restatements_on_the_gpu_cases(kw):
    c = check_mobile_case(kw)
    name = kw["mutate"].__name__ if "mutate" in kw else ""
    o = mobile_operands(c, 0, kw)
    if name == "identical_elites":
        assert (rr.lcb_penalty(o["ql"], c.B, c.S, c.E, c.real_rows)[1].v == 0).all()
    elif name == "reward-1e3":
        pen = lcb_arith(o["ql"], c.B, c.S, c.E, c.real_rows)[1]
        y = rr.mobile_td_loss(o["q"], o["qt"], o["rew"], o["term"], pen, o["gamma"], o["coef"], c.B, logp_next=o["logp_next"], alpha=o["alpha"])[0]
        assert (y.v == 0).all() and (y.e == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# the dynamic scale
# ---------------------------------------------------------------------------------------------------------------------------------
def test_pow2_scale_is_two_to_the_three_minus_floor_log2():
    vals = [1.0, 2.0, 0.5, 3.0, 1e-3, 1e3, 7.999, 8.0, 2.0 ** -20, 2.0 ** 20, float(np.nextafter(f32(1), f32(0))), float(np.nextafter(f32(1), f32(2))), 1.5e-7, 6.5e4]
    for a in vals:
        a = float(f32(a))
        s = rr.pow2_scale(a)
        assert s == 2.0 ** (3 - math.floor(math.log2(a))), a
        assert 8.0 <= a * s < 16.0, (a, s)
        assert float(f32(s)) == s
    for a in (0.0, float("inf"), float("nan"), -0.0):
        assert rr.pow2_scale(a) == 1.0


# ---------------------------------------------------------------------------------------------------------------------------------
# planted defects: each is beyond the bar on at least one case
# ---------------------------------------------------------------------------------------------------------------------------------
def test_planted_divisor_B_A_is_beyond_the_bar():
    c = hc.inputs("rcsl", pad="interleaved")
    b, v = c.batches[0], c.valid[0]
    pred = rorc.forward(c.nets[0], b["observations"], b["rtgs"])[0]
    rL, rdp = rr.rcsl_loss(pred, b["actions"], v)
    L, dp = rcsl_arith(pred, b["actions"], v)
    inside(L, rL, "loss"); inside(dp, rdp, "dpred")
    L, dp = rcsl_arith(pred, b["actions"], v, "divisor_BA")
    beyond(L, rL, "loss over B A"); beyond(dp, rdp, "dpred over B A")
    c = hc.inputs("rcslg", pad="one_pad")
    b, v, net, res, aux = gauss_operands(c, 0)
    ref = rr.rcslg_head(aux["z"], b["actions"], net, v, raw32=aux["raw"])
    bad = gauss_arith(net, aux["z"], b["actions"], v, "divisor_BA")
    for k in ("loss", "dmu", "ds", "dz"):
        beyond(bad[k], ref[k], "rcslg over B A: " + k)


def test_planted_dropped_chunk_row_and_exclusive_gate_are_beyond_the_bar():
    for kw in (dict(B=129), dict(A=32, B=129)):
        c = hc.inputs("rcslg", **kw)
        b, v, net, res, aux = gauss_operands(c, 0)
        ref = rr.rcslg_head(aux["z"], b["actions"], net, v, raw32=aux["raw"])
        bad = gauss_arith(net, aux["z"], b["actions"], v, "chunk_last_row_dropped")
        for k in rr.RG_HEAD:
            if k.startswith("dist_net.mu"):
                beyond(bad["grads"][k], ref["grads"][k], ("row 63 dropped", k))
        inside(bad["dz"], ref["dz"], "dz does not see the defect")
    c = hc.inputs("rcslg", **hc.RCSLG_EDGES[0])
    b, v, net, res, aux = gauss_operands(c, 0)
    ref = rr.rcslg_head(aux["z"], b["actions"], net, v, raw32=aux["raw"])
    good, bad = gauss_arith(net, aux["z"], b["actions"], v), gauss_arith(net, aux["z"], b["actions"], v, "exclusive_gate")
    on = [j for j in range(c.A) if hc.LV_TABLE[j % 9] in (-5.0, 2.0)]
    assert (bad["ds"][:, on] == 0).all() and (good["ds"][:, on] != 0).all()
    inside(good["ds"], ref["ds"], "ds")
    beyond(bad["ds"], ref["ds"], "exclusive gate (ds)")
    beyond(bad["grads"]["dist_net.sigma.bias"], ref["grads"]["dist_net.sigma.bias"], "exclusive gate (sigma.bias)")


def test_planted_leaky_slope_and_padding_map_are_beyond_the_bar():
    c = hc.inputs("autoreg", B=86, A=3, pad="interleaved")
    v, res, aux = autoreg_operands(c, 0)
    z, t = aux["z_tail"], aux["target"]
    assert (z < 0).any(axis=0).all() and (z > 0).any(axis=0).all()
    _, _, rdz = rr.autoreg_head(z, t, c.A, v)
    inside(autoreg_arith(z, t, v, c.A)[2], rdz, "dz")
    beyond(autoreg_arith(z, t, v, c.A, "slope_1")[2], rdz, "slope 1 on the negative branch")
    out, L, dz = autoreg_arith(z, t, v, c.A, "pad_by_m_over_A")
    beyond(dz, rdz, "padding mapped by m / A")
    beyond(L, rr.autoreg_head(z, t, c.A, v)[1], "padding mapped by m / A (loss)")


def test_planted_mobile_defects_are_beyond_the_bar():
    kw = dict()
    c = hc.mobile_inputs(**kw)
    o = mobile_operands(c, 0, kw)
    S, E, B = c.S, c.E, c.B
    _, rpen = rr.lcb_penalty(o["ql"], B, S, E, c.real_rows)
    inside(lcb_arith(o["ql"], B, S, E, c.real_rows)[1], rpen, "penalty")
    beyond(lcb_arith(o["ql"], B, S, E, c.real_rows, "biased_std")[1], rpen, "biased std")
    beyond(lcb_arith(o["ql"], B, S, E, c.real_rows, "no_mean_over_S")[1], rpen, "mean over S omitted")
    pen = lcb_arith(o["ql"], B, S, E, c.real_rows)[1]
    args = (o["q"], o["qt"], o["rew"], o["term"], pen, o["gamma"], o["coef"], B)
    ta = (o["q"], o["qt"], o["rew"], o["term"], pen, o["logp_next"], o["alpha"], o["gamma"], o["coef"], B, o["det"])
    y, L, dq = td_arith(*ta)
    _, rL, rdq = rr.mobile_td_loss(*args, logp_next=o["logp_next"], alpha=o["alpha"], stored=y)
    inside(dq, rdq, "dq")
    beyond(td_arith(*ta, defect="dq_over_B")[2], rdq, "dq over B")
    kw = dict(mutate=hc.batch_edge("reward-1e3"))
    c = hc.mobile_inputs(**kw)
    o = mobile_operands(c, 0, kw)
    pen = lcb_arith(o["ql"], B, S, E, c.real_rows)[1]
    ry = rr.mobile_td_loss(o["q"], o["qt"], o["rew"], o["term"], pen, o["gamma"], o["coef"], B, logp_next=o["logp_next"], alpha=o["alpha"])[0]
    ta = (o["q"], o["qt"], o["rew"], o["term"], pen, o["logp_next"], o["alpha"], o["gamma"], o["coef"], B, o["det"])
    inside(td_arith(*ta)[0], ry, "y")
    beyond(td_arith(*ta, defect="y_unclamped")[0], ry, "y left unclamped")


def test_planted_scale_exponent_off_by_one_is_rejected():
    for a in (1.0, 0.37, 5e-4, 12.0):
        s = rr.pow2_scale(a)
        for bad in (2.0 * s, 0.5 * s):
            assert beyond(bad, rr.BV(s), ("scale exponent off by one", a)) == np.inf
            assert not (8.0 <= float(f32(a)) * bad < 16.0)
